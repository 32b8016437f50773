// Hetero-center triplet loss for gfx950, all fp32 (Zhu et al., "Hetero-Center Loss", Neurocomputing 2020; Liu et al., "Parameter Sharing
// Exploration and Hetero-Center Triplet Loss", IEEE TMM 2020): P stacked query sides q [P*N, D] (one per non-vis modality) against the
// shared vis side g [Mg, D]; the triplet runs on the per-identity CENTRES of every side inside the batch.  The reference has no such
// loss; include/reid_hip.h (reid_hc_triplet_*) and DESIGN.md section 15 are the definition.
//
// The kernels here decode indices and call the pieces of triplet_mine.h (shared with triplet.hip and cross_triplet.hip; the list of
// pieces and callers is at its head); the entry points use its argument checks.
//
// Forward, launch 1 (hc_unit_kernel, normalize = 1 only): the unit rows of both sides (triplet::unit_row, as cross_triplet.hip).
// Forward, launch 2 (hc_lead_kernel): one workgroup per side (P q sides, then g).  leader(i) = the lowest valid row with row i's label
//   (an O(n^2) label compare, 64 candidates at a time per wave), the leaders numbered in ascending order by a workgroup scan -> lead [row] = centre slot or -1,
//   the slot's leader row and the side's centre count S, which never leaves the device.
// Forward, launch 3 (hc_centre_kernel): one wave per (side, slot): the members' rows added in ascending row order, one division by
//   float(count) per element.  The centres of pair p are stored COMPACT and contiguous in ws, U_p = [S_q[p] q centres | S_g g centres],
//   with their labels beside them; a g centre is computed once and stored into every pair's block.
// Forward, launch 4 (hc_mine_kernel): blockIdx = (pair, tile of 4 anchors); ONE call of triplet::mine_tile (triplet_mine.h, the loop of
//   triplet.hip) with A = C = U_p and self-exclusion, the row count S_q[p] + S_g read from ws.  The grid is sized for N + Mg centres;
//   workgroups behind the count leave, and the candidates walked are the S_q + S_g used ones.
// Forward, launch 5 (hc_refine_kernel): one wave per slot of the index space 0 .. N + Mg - 1 (q centre s -> s, g centre t -> N + t):
//   the two distances an active anchor keeps re-evaluated with an fp64 sum (triplet::refine_anchor), its compact indices mapped to the
//   index space; unused slots and inactive anchors get -1 / 0.
// Forward, launch 6 (hc_finalize_kernel): one workgroup per pair adds the anchors' losses in a fixed order in fp64
//   -> result [P, 4] = {L_p, flag_p, n_q, n_g}.
// Backward, launch 1 (hc_bwd_centre_kernel): gather form, one wave per centre: its own two terms as an anchor, then the anchors of U_p
//   in ascending order that chose it; a g centre runs over p ascending.  -> the centre-space gradients in ws.
// Backward, launch 2 (hc_bwd_rows_kernel): one wave per output row: G_centre(lead) / float(count), then the projection through the
//   normalisation exactly as xt_bwd_kernel.
// No atomics anywhere: two runs give the same bits in every output.  Nothing is allocated, synchronised or read back.
#include "triplet_mine.h"

namespace {

using namespace triplet;

constexpr int LT = 1024;                 // threads of hc_lead_kernel
constexpr int MAXN = MAX_ROWS;           // rows per side (checked by triplet::check_dims)

inline int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// ws (floats), R = P N + Mg rows, U = N + Mg slots of a pair's union:
//   unit rows R D | centres P U D (compact per pair) | centre gradients R D (slot order: pair p's q slots at p N, g slots at P N) |
//   centre labels P U int64 | compact d_ap, d_an 2 P U | compact idx_p, idx_n 2 P U int32 | anchor losses P U |
//   1 / max(|x|, eps) R | |x| R | leader row of a slot R int32 | centre counts S_q[0..P), S_g: P + 1 int32
struct Ws {
    int64_t unit, cen, grad, clab, cd, cidx, closs, inv, norm, srow, S, total;
    Ws(int64_t P, int64_t N, int64_t Mg, int64_t D) {
        const int64_t R = P * N + Mg, PU = P * (N + Mg);
        unit = 0; cen = unit + R * D; grad = cen + PU * D; clab = grad + R * D; cd = clab + 2 * up4(PU); cidx = cd + 2 * PU;
        closs = cidx + 2 * PU; inv = closs + PU; norm = inv + R; srow = norm + R; S = srow + R; total = up4(S + P + 1);
    }
};

// rows [0, PN) are q rows, rows [PN, PN + Mg) are g rows; one wave per row.  (The same body as cross_triplet.hip's xt_unit_kernel.)
__global__ __launch_bounds__(256) void hc_unit_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ g, int ldg, int PN,
                                                      int Mg, int D, float eps, float* __restrict__ unit, float* __restrict__ inv_out,
                                                      float* __restrict__ norm_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= PN + Mg) return;
    unit_row(row < PN ? q + (size_t)row * ldq : g + (size_t)(row - PN) * ldg, D, eps, unit + (size_t)row * D, inv_out + row, norm_out + row,
             threadIdx.x & 63);
}

// One workgroup per side.  lead / srow are indexed from the side's first row (p N for q side p, P N for g).
__global__ __launch_bounds__(LT) void hc_lead_kernel(const int64_t* __restrict__ q_label, const int64_t* __restrict__ g_label,
                                                     const uint8_t* __restrict__ q_valid, const uint8_t* __restrict__ g_valid, int P, int N,
                                                     int Mg, int* __restrict__ lead, int* __restrict__ srow, int* __restrict__ S) {
    __shared__ int s_leader[MAXN];       // the leader ROW of a row, -1 for an invalid row
    __shared__ uint16_t s_slot[MAXN];    // the slot of a leader row
    __shared__ int s_scan[LT];
    const int tid = threadIdx.x, side = blockIdx.x;
    const bool is_q = side < P;
    const int n = is_q ? N : Mg, off = is_q ? side * N : P * N;
    const int64_t* lab = is_q ? q_label : g_label;
    const uint8_t* val = is_q ? (q_valid ? q_valid + off : nullptr) : g_valid;
    // The rows of a wave are 64 consecutive ones, so its candidates j run over one range: 64 at a time, one coalesced load per lane, then
    // handed round with readlane (a per-lane loop over j with a break is one load latency per step).  The loop over the wave's rows is
    // wave-uniform: every lane takes part in the ballots and is read by the readlanes.
    const int lane = tid & 63;
    for (int ib = tid & ~63; ib < n; ib += LT) {
        const int i = ib + lane, ic = min(i, n - 1);
        const int hi = min(n, ib + 64);
        const bool ok = i < n && (!val || val[ic]);
        const int64_t l = lab[ic];
        const int l_lo = (int)l, l_hi = (int)(l >> 32);
        int lr = -1;
        for (int j0 = 0; j0 < hi; j0 += 64) {
            const int jj = min(j0 + lane, n - 1);
            const int64_t lj = lab[jj];
            const unsigned long long vmask = __ballot(j0 + lane < n && (!val || val[jj]));
            const int lj_lo = (int)lj, lj_hi = (int)(lj >> 32);
            unsigned long long hit = 0;                              // bit k: row j0 + k has my label
#pragma unroll
            for (int k = 0; k < 64; ++k)
                if (__builtin_amdgcn_readlane(lj_lo, k) == l_lo && __builtin_amdgcn_readlane(lj_hi, k) == l_hi) hit |= 1ull << k;
            hit &= vmask;                                            // ... and is a valid row
            if (i - j0 < 63) hit &= (2ull << max(i - j0, 0)) - 1;    // rows up to i only
            if (lr < 0 && hit) lr = j0 + __builtin_ctzll(hit);
        }
        if (i < n) s_leader[i] = ok ? lr : -1;
    }
    __syncthreads();
    const int chunk = (n + LT - 1) / LT, b = tid * chunk, e = min(b + chunk, n);
    int cnt = 0;
    for (int i = b; i < e; ++i) cnt += s_leader[i] == i;
    s_scan[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < LT; o <<= 1) {                               // inclusive scan over the threads' leader counts
        const int v = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int slot = s_scan[tid] - cnt;
    for (int i = b; i < e; ++i)
        if (s_leader[i] == i) { s_slot[i] = (uint16_t)slot; srow[off + slot] = i; ++slot; }
    if (tid == 0) S[side] = s_scan[LT - 1];
    __syncthreads();
    for (int i = tid; i < n; i += LT) {
        const int lr = s_leader[i];
        lead[off + i] = lr >= 0 ? (int)s_slot[lr] : -1;
    }
}

// slot w of [0, P N + Mg) -> its side, the slot within the side and the side's row count
struct Slot {
    bool is_q; int p, s, n, off;
    __device__ Slot(int w, int P, int N, int Mg) {
        is_q = w < P * N; p = is_q ? w / N : P; s = is_q ? w % N : w - P * N; n = is_q ? N : Mg; off = is_q ? p * N : P * N;
    }
};

// one wave per (side, slot)
__global__ __launch_bounds__(256) void hc_centre_kernel(Sides sd, const int64_t* __restrict__ q_label, const int64_t* __restrict__ g_label,
                                                        int P, int N, int Mg, int D, const int* __restrict__ lead,
                                                        const int* __restrict__ srow, const int* __restrict__ S, float* __restrict__ cen,
                                                        int64_t* __restrict__ clab, int* __restrict__ count, int64_t* __restrict__ clabel) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= P * N + Mg) return;
    const Slot t(w, P, N, Mg);
    if (t.s >= S[t.p]) {                                             // behind the side's centre count
        if (lane == 0) { count[w] = 0; clabel[w] = 0; }
        return;
    }
    const float* x = t.is_q ? sd.q + (size_t)t.off * sd.ldq : sd.g;
    const int ld = t.is_q ? sd.ldq : sd.ldg;
    const int r0 = srow[w];
    f32x4 acc[NV];
    zero_acc(acc);
    int cnt = 0;
    for (int b = r0 & ~63; b < t.n; b += 64) {                       // the members in ascending row order (the leader is the first)
        const int a = b + lane;
        unsigned long long hit = __ballot(a < t.n && lead[t.off + a] == t.s);
        while (hit) {
            const int r = b + __builtin_ctzll(hit);
            hit &= hit - 1;
            ++cnt;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c = 4 * lane + 256 * v;
                if (c < D) acc[v] = acc[v] + *(const f32x4*)(x + (size_t)r * ld + c);
            }
        }
    }
    const float fc = (float)cnt;
    const int64_t label = (t.is_q ? q_label : g_label)[r0];
    const int U = N + Mg;
    for (int p = t.is_q ? t.p : 0; p < (t.is_q ? t.p + 1 : P); ++p) {          // a g centre goes into every pair's block
        const size_t k = (size_t)p * U + (t.is_q ? t.s : S[p] + t.s);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = 4 * lane + 256 * v;
            if (c < D) *(f32x4*)(cen + k * D + c) = acc[v] / fc;
        }
        if (lane == 0) clab[k] = label;
    }
    if (lane == 0) { count[w] = cnt; clabel[w] = label; }
}

// cd [2, P U] = d_ap | d_an, cidx [2, P U] = idx_p | idx_n, closs [P U]: compact, pair p at p U
__global__ __launch_bounds__(256) void hc_mine_kernel(const float* __restrict__ cen, const int64_t* __restrict__ clab,
                                                      const int* __restrict__ S, int P, int U, int D, float margin, float* __restrict__ cd,
                                                      int* __restrict__ cidx, float* __restrict__ closs) {
    const int tiles = (U + TA - 1) / TA;
    const int p = blockIdx.x / tiles, a0 = (blockIdx.x % tiles) * TA;
    const int n = S[p] + S[P];                                       // the centres of U_p: a device value, uniform over the workgroup
    if (a0 >= n) return;
    const size_t o = (size_t)p * U;
    const Rows u{cen + o * D, D, clab + o, nullptr, n};
    const size_t PU = (size_t)P * U;
    mine_tile(u, u, a0, a0, D, margin, cd + o, cd + PU + o, cidx + o, cidx + PU + o, closs + o);      // a centre is no positive of itself
}

// One wave per slot (p, u) of the index space.  d [2, P U] and idx [2, P U] are the callers' arrays.
__global__ __launch_bounds__(256) void hc_refine_kernel(const float* __restrict__ cen, const int* __restrict__ S, int P, int N, int Mg, int D,
                                                        float margin, float* __restrict__ cd, const int* __restrict__ cidx,
                                                        float* __restrict__ closs, float* __restrict__ d, int* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int U = N + Mg, PU = P * U;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= PU) return;
    const int p = w / U, u = w % U;
    const int sq = S[p], n = sq + S[P];
    const int k = u < N ? (u < sq ? u : -1) : (u - N < S[P] ? sq + u - N : -1);      // the compact slot, -1: unused
    int jp = -1, jn = -1;
    if (k >= 0) { jp = cidx[p * U + k]; jn = cidx[PU + p * U + k]; }
    if (jp < 0 || jp >= n || jn < 0 || jn >= n) {                    // unused or not active
        if (lane == 0) { d[w] = 0.f; d[PU + w] = 0.f; idx[w] = -1; idx[PU + w] = -1; }
        return;
    }
    const float* c = cen + (size_t)p * U * D;
    const float* xa = c + (size_t)k * D;
    float dp, dn;                                                    // (lane 0's)
    refine_anchor(xa, c, D, jp, jn, D, lane, dp, dn);
    if (lane == 0) {
        cd[p * U + k] = dp; cd[PU + p * U + k] = dn;
        closs[p * U + k] = row_loss_of(dp - dn, margin);
        d[w] = dp; d[PU + w] = dn;
        idx[w] = jp < sq ? jp : N + jp - sq; idx[PU + w] = jn < sq ? jn : N + jn - sq;
    }
}

// one workgroup per pair: thread t adds anchors t, t + 256, ... in fp64, the 256 sums are added in index order (the tail of
// triplet_finalize_kernel and xt_finalize_kernel, with one sum and two counts)
__global__ __launch_bounds__(256) void hc_finalize_kernel(const float* __restrict__ closs, const int* __restrict__ cidx,
                                                          const int* __restrict__ S, int P, int U, float* __restrict__ result) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[2][256];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int sq = S[p], n = sq + S[P];
    double s = 0.0;
    int cq = 0, cg = 0;
    for (int k = tid; k < n; k += 256)
        if (cidx[p * U + k] >= 0) { s += (double)closs[p * U + k]; if (k < sq) ++cq; else ++cg; }
    s_sum[tid] = s; s_cnt[0][tid] = cq; s_cnt[1][tid] = cg;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        int c[2] = {0, 0};
        for (int u = 0; u < 256; ++u) { t += s_sum[u]; c[0] += s_cnt[0][u]; c[1] += s_cnt[1][u]; }
        const int na = c[0] + c[1];
        result[4 * p + 0] = na > 0 ? (float)(t / (double)na) : 0.f;
        result[4 * p + 1] = na > 0 ? 1.f : 0.f;
        result[4 * p + 2] = (float)c[0];
        result[4 * p + 3] = (float)c[1];
    }
}

// one wave per (side, slot): the centre-space gradient of the slot's centre -> grad [P N + Mg, D] in slot order
__global__ __launch_bounds__(256) void hc_bwd_centre_kernel(const float* __restrict__ cen, const int* __restrict__ S, int P, int N, int Mg,
                                                            int D, float margin, const float* __restrict__ cd, const int* __restrict__ cidx,
                                                            const float* __restrict__ result, const float* __restrict__ gscale,
                                                            float* __restrict__ grad) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= P * N + Mg) return;
    const Slot t(w, P, N, Mg);
    if (t.s >= S[t.p]) return;                                       // nobody reads the gradient of an unused slot
    const int U = N + Mg, PU = P * U;
    f32x4 xi[NV], acc[NV];
    zero_acc(acc);
    for (int p = t.is_q ? t.p : 0; p < (t.is_q ? t.p + 1 : P); ++p) {
        const int sq = S[p], n = sq + S[P];
        const int k = t.is_q ? t.s : sq + t.s;
        const float* c = cen + (size_t)p * U * D;
#pragma unroll
        for (int v = 0; v < NV; ++v) {                                // (a g centre holds the same bits in every pair's block)
            const int col = 4 * lane + 256 * v;                      // (triplet::load_row and store_row, written out in this kernel)
            xi[v] = col < D ? *(const f32x4*)(c + (size_t)k * D + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float cn = gscale[p] / fmaxf(result[4 * p + 2] + result[4 * p + 3], 1.f);
        const int* ip = cidx + p * U; const float* dp = cd + p * U;
        add_own(acc, xi, k, c, D, n, ip, ip + PU, dp, dp + PU, cn, margin, lane, D);
        add_chosen_by(acc, xi, k, c, D, n, ip, ip + PU, dp, dp + PU, cn, margin, lane, D);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int col = 4 * lane + 256 * v;
        if (col < D) *(f32x4*)(grad + (size_t)w * D + col) = acc[v];
    }
}

// one wave per output row: rows [0, P N) of dq, then rows [0, Mg) of dg
__global__ __launch_bounds__(256) void hc_bwd_rows_kernel(Sides sd, int P, int N, int Mg, int D, int normalize, float eps,
                                                          const int* __restrict__ lead, const int* __restrict__ count,
                                                          const float* __restrict__ grad, const float* __restrict__ inv,
                                                          const float* __restrict__ norm, float* __restrict__ dq, int lddq,
                                                          float* __restrict__ dg, int lddg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int PN = P * N;
    if (row >= PN + Mg) return;
    const bool is_q = row < PN;
    const int off = is_q ? (row / N) * N : PN;                       // the side's first row = its first slot
    float* o = is_q ? dq + (size_t)row * lddq : dg + (size_t)(row - PN) * lddg;
    const int slot = lead[row];
    f32x4 acc[NV];
    zero_acc(acc);
    if (slot >= 0) {                                                 // (an invalid row belongs to no centre: zeros)
        const float fc = (float)count[off + slot];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = 4 * lane + 256 * v;
            if (c < D) acc[v] = *(const f32x4*)(grad + (size_t)(off + slot) * D + c) / fc;
        }
        if (normalize) {
            if (norm[row] >= eps) {                                  // dx = (G - x^ (x^ . G)) / max(|x|, eps); the same block as in
                                                                     // cross_triplet.hip's xt_bwd_kernel, which has x^ in registers already
                const float* xr = is_q ? sd.q + (size_t)row * sd.ldq : sd.g + (size_t)(row - PN) * sd.ldg;
                f32x4 xi[NV];
                float dot = 0.f;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int c = 4 * lane + 256 * v;
                    xi[v] = c < D ? *(const f32x4*)(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
                    dot += xi[v][0] * acc[v][0] + xi[v][1] * acc[v][1] + xi[v][2] * acc[v][2] + xi[v][3] * acc[v][3];
                }
                dot = wave_sum(dot);
                const float iv = inv[row];
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] = (acc[v] - xi[v] * dot) * iv;
            } else {                                                 // x / norm.clamp_min(eps) is linear in x there: dx = G / eps
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] = acc[v] / eps;
            }
        }
    }
    store_row(o, acc, lane, D);
}

}  // namespace

extern "C" int64_t reid_hc_triplet_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D) {
    if (int rc = check_dims("reid_hc_triplet_ws_floats", P, N, Mg, D)) return rc;
    return Ws(P, N, Mg, D).total;
}

extern "C" int reid_hc_triplet_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label,
                                   const int64_t* g_label, const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N,
                                   int32_t Mg, int32_t D, float margin, int32_t normalize, float eps, int32_t* lead, int32_t* count,
                                   int64_t* clabel, float* d, int32_t* idx, float* ws, float* result, void* stream) {
    const char* who = "reid_hc_triplet_fwd";
    REID_CHECK_ARG(q && g && q_label && g_label && lead && count && clabel && d && idx && ws && result, "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, Mg, D, ldg, "ldg")) return rc;
    if (int rc = check_scalars(who, margin, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(ws), "%s: q, g or ws is not 16-byte aligned", who);
    const Ws w(P, N, Mg, D);
    hipStream_t s = (hipStream_t)stream;
    const int PN = P * N, R = PN + Mg, U = N + Mg;
    int* S = (int*)(ws + w.S);
    int* srow = (int*)(ws + w.srow);
    int64_t* clab = (int64_t*)(ws + w.clab);
    int* cidx = (int*)(ws + w.cidx);
    Sides sd{q, ldq, g, ldg};
    if (normalize) {
        hipLaunchKernelGGL(hc_unit_kernel, dim3((R + 3) / 4), dim3(256), 0, s, q, ldq, g, ldg, PN, Mg, D, eps, ws + w.unit, ws + w.inv,
                           ws + w.norm);
        REID_CHECK_LAUNCH("reid_hc_triplet_fwd(unit rows)");
        sd = Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D};
    }
    hipLaunchKernelGGL(hc_lead_kernel, dim3(P + 1), dim3(LT), 0, s, q_label, g_label, q_valid, g_valid, P, N, Mg, lead, srow, S);
    REID_CHECK_LAUNCH("reid_hc_triplet_fwd(leaders)");
    hipLaunchKernelGGL(hc_centre_kernel, dim3((R + 3) / 4), dim3(256), 0, s, sd, q_label, g_label, P, N, Mg, D, lead, srow, S, ws + w.cen, clab,
                       count, clabel);
    REID_CHECK_LAUNCH("reid_hc_triplet_fwd(centres)");
    hipLaunchKernelGGL(hc_mine_kernel, dim3(P * ((U + TA - 1) / TA)), dim3(256), 0, s, ws + w.cen, clab, S, P, U, D, margin, ws + w.cd, cidx,
                       ws + w.closs);
    REID_CHECK_LAUNCH("reid_hc_triplet_fwd(mine)");
    hipLaunchKernelGGL(hc_refine_kernel, dim3((P * U + 3) / 4), dim3(256), 0, s, ws + w.cen, S, P, N, Mg, D, margin, ws + w.cd, cidx,
                       ws + w.closs, d, idx);
    REID_CHECK_LAUNCH("reid_hc_triplet_fwd(refine)");
    hipLaunchKernelGGL(hc_finalize_kernel, dim3(P), dim3(256), 0, s, ws + w.closs, cidx, S, P, U, result);
    REID_CHECK_LAUNCH("reid_hc_triplet_fwd(finalize)");
    return REID_OK;
}

extern "C" int reid_hc_triplet_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, int32_t P, int32_t N, int32_t Mg, int32_t D,
                                   float margin, int32_t normalize, float eps, const int32_t* lead, const int32_t* count, float* ws,
                                   const float* result, const float* gscale, float* dq, int32_t lddq, float* dg, int32_t lddg,
                                   void* stream) {
    const char* who = "reid_hc_triplet_bwd";
    REID_CHECK_ARG(q && g && lead && count && ws && result && gscale && dq && dg, "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, Mg, D, ldg, "ldg")) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, lddq, "lddq")) return rc;
    if (int rc = check_ld(who, Mg, D, lddg, "lddg")) return rc;
    if (int rc = check_scalars(who, margin, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(ws) && aligned16(dq) && aligned16(dg),
                   "%s: q, g, ws, dq or dg is not 16-byte aligned", who);
    const Ws w(P, N, Mg, D);
    hipStream_t s = (hipStream_t)stream;
    const int PN = P * N, R = PN + Mg;
    const int* S = (const int*)(ws + w.S);
    float* grad = ws + w.grad;
    const Sides sd = normalize ? Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D} : Sides{q, ldq, g, ldg};
    hipLaunchKernelGGL(hc_bwd_centre_kernel, dim3((R + 3) / 4), dim3(256), 0, s, ws + w.cen, S, P, N, Mg, D, margin, ws + w.cd,
                       (const int*)(ws + w.cidx), result, gscale, grad);
    REID_CHECK_LAUNCH("reid_hc_triplet_bwd(centres)");
    hipLaunchKernelGGL(hc_bwd_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, s, sd, P, N, Mg, D, normalize, eps, lead, count, grad, ws + w.inv,
                       ws + w.norm, dq, lddq, dg, lddg);
    REID_CHECK_LAUNCH("reid_hc_triplet_bwd(rows)");
    return REID_OK;
}
