// Cross-modal batch-hard triplet loss for gfx950, all fp32: P stacked query sides q [P*N, D] (one per non-vis modality) against the
// shared vis side g [Mg, D], mined in both directions (Ye et al., AGW 2021; mining of Hermans et al. 2017).  The reference has no
// such loss; include/reid_hip.h (reid_cross_triplet_*) and DESIGN.md section 14 are the definition.
//
// The kernels here decode indices and call the pieces of triplet_mine.h (shared with triplet.hip and hc_triplet.hip; the list of
// pieces and callers is at its head); the entry points use its argument checks.
//
// Forward, launch 1 (xt_unit_kernel, normalize = 1 only): the unit rows x * (1 / max(|x|, eps)) of BOTH sides, once and not once per
//   pair, into ws, with 1 / max(|x|, eps) and |x| beside them; one wave per row (triplet::unit_row).
// Forward, launch 2 (xt_fwd_kernel): blockIdx = (pair, direction, tile of 4 anchors).  Direction q->g: anchors are q rows of pair p,
//   candidates the g rows; g->q: the other way round, indices pair-local.  Both are ONE call of triplet::mine_tile (triplet_mine.h, the
//   loop of csrc/triplet.hip) with the two sides swapped; nothing is excluded as "self" (row i of q and row i of g are one person in
//   two modalities: a legitimate positive).
// Forward, launch 3 (xt_refine_kernel): one wave per anchor re-evaluates the two distances it keeps with an fp64 sum
//   (triplet::refine_anchor).
// Forward, launch 4 (xt_finalize_kernel): one workgroup per pair adds the row losses of either direction in a fixed order in fp64
//   -> result [P, 4] = {L_p, flag_p, n_qg, n_gq}.
// Backward (xt_bwd_kernel): gather form, one wave per output row of dq and dg.  The unit-space gradient G of q row (p, i): its own two
//   terms as an anchor, then every g anchor of pair p in ascending order that chose i; of g row j, for p ascending: its own two terms
//   as an anchor of pair p, then the q anchors of pair p in ascending order that chose j.  The projection through the normalisation
//   is in the same kernel: dx = (G - x^ (x^ . G)) / max(|x|, eps) with x^ . G a wave reduction (G / eps where |x| < eps).
// No atomics anywhere: two runs give the same bits in every output.  Nothing is allocated, synchronised or read back.
#include "triplet_mine.h"

namespace {

using namespace triplet;

// ws (floats): unit rows (P N + Mg) D | 1 / max(|x|, eps) (P N + Mg) | |x| (P N + Mg) | row losses: q->g P N, g->q P Mg
struct Ws {
    int64_t unit, inv, norm, loss_q, loss_g, total;
    Ws(int64_t P, int64_t N, int64_t Mg, int64_t D) {
        const int64_t R = P * N + Mg;
        unit = 0; inv = R * D; norm = inv + R; loss_q = norm + R; loss_g = loss_q + P * N; total = loss_g + P * Mg;
    }
};

// rows [0, PN) are q rows, rows [PN, PN + Mg) are g rows; one wave per row (triplet::unit_row).  (The same body as hc_triplet.hip's
// hc_unit_kernel.)
__global__ __launch_bounds__(256) void xt_unit_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ g, int ldg, int PN,
                                                      int Mg, int D, float eps, float* __restrict__ unit, float* __restrict__ inv_out,
                                                      float* __restrict__ norm_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= PN + Mg) return;
    unit_row(row < PN ? q + (size_t)row * ldq : g + (size_t)(row - PN) * ldg, D, eps, unit + (size_t)row * D, inv_out + row, norm_out + row,
             threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void xt_fwd_kernel(Sides s, const int64_t* __restrict__ q_label, const int64_t* __restrict__ g_label,
                                                     const uint8_t* __restrict__ q_valid, const uint8_t* __restrict__ g_valid, int P, int N,
                                                     int Mg, int D, float margin, float* __restrict__ q_d, int* __restrict__ q_idx,
                                                     float* __restrict__ g_d, int* __restrict__ g_idx, float* __restrict__ loss_q,
                                                     float* __restrict__ loss_g) {
    const int tq = (N + TA - 1) / TA, tg = (Mg + TA - 1) / TA;
    const int p = blockIdx.x / (tq + tg), t = blockIdx.x % (tq + tg);
    const Rows qs{s.q + (size_t)p * N * s.ldq, s.ldq, q_label, q_valid ? q_valid + p * N : nullptr, N};
    const Rows gs{s.g, s.ldg, g_label, g_valid, Mg};
    const bool qg = t < tq;                                          // uniform over the workgroup; ONE call: one LDS image
    const int n = qg ? N : Mg;                                       // anchors of this direction per pair
    float* d = (qg ? q_d : g_d) + p * n;                             // [2, P n]: d_ap | d_an
    int* ix = (qg ? q_idx : g_idx) + p * n;
    mine_tile(qg ? qs : gs, qg ? gs : qs, (qg ? t : t - tq) * TA, NO_SELF, D, margin, d, d + P * n, ix, ix + P * n,
              (qg ? loss_q : loss_g) + p * n);
}

// One wave per anchor of either direction: the two distances the anchor keeps, re-evaluated from the same rows with an fp64 sum and
// rounded once (triplet::refine_anchor: why), and its row loss from them.
__global__ __launch_bounds__(256) void xt_refine_kernel(Sides s, int P, int N, int Mg, int D, float margin, float* __restrict__ q_d,
                                                        const int* __restrict__ q_idx, float* __restrict__ g_d,
                                                        const int* __restrict__ g_idx, float* __restrict__ loss_q,
                                                        float* __restrict__ loss_g) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= P * (N + Mg)) return;
    const bool qg = w < P * N;
    const int r = qg ? w : w - P * N, n = qg ? N : Mg, nc = qg ? Mg : N;             // r = p n + a: the anchor's slot in [P, n]
    const int p = r / n, a = r % n;
    const float* xa = qg ? s.q + ((size_t)p * N + a) * s.ldq : s.g + (size_t)a * s.ldg;
    const float* xc = qg ? s.g : s.q + (size_t)p * N * s.ldq;                        // the candidates' rows
    const int ldc = qg ? s.ldg : s.ldq;
    float* d = qg ? q_d : g_d;
    const int* ix = qg ? q_idx : g_idx;
    const int jp = ix[r], jn = ix[P * n + r];
    if (jp < 0 || jp >= nc || jn < 0 || jn >= nc) return;                            // not active: the zeros stay
    float dp, dn;                                                                    // (lane 0's)
    refine_anchor(xa, xc, ldc, jp, jn, D, lane, dp, dn);
    if (lane == 0) {
        d[r] = dp; d[P * n + r] = dn;
        (qg ? loss_q : loss_g)[r] = row_loss_of(dp - dn, margin);
    }
}

// one workgroup per pair: thread t adds rows t, t + 256, ... of a direction in fp64, the 256 sums are added in index order (the tail
// of triplet_finalize_kernel and hc_finalize_kernel, with two sums and two counts)
__global__ __launch_bounds__(256) void xt_finalize_kernel(const float* __restrict__ loss_q, const float* __restrict__ loss_g,
                                                          const int* __restrict__ q_idx, const int* __restrict__ g_idx, int N, int Mg,
                                                          float* __restrict__ result) {
    __shared__ double s_sum[2][256];
    __shared__ int s_cnt[2][256];
    const int tid = threadIdx.x, p = blockIdx.x;
    for (int dir = 0; dir < 2; ++dir) {
        const int n = dir ? Mg : N;
        const float* rl = dir ? loss_g + (size_t)p * Mg : loss_q + (size_t)p * N;
        const int* ip = dir ? g_idx + (size_t)p * Mg : q_idx + (size_t)p * N;
        double s = 0.0;
        int c = 0;
        for (int r = tid; r < n; r += 256)
            if (ip[r] >= 0) { s += (double)rl[r]; ++c; }
        s_sum[dir][tid] = s; s_cnt[dir][tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double t[2] = {0.0, 0.0};
        int c[2] = {0, 0};
        for (int dir = 0; dir < 2; ++dir)
            for (int u = 0; u < 256; ++u) { t[dir] += s_sum[dir][u]; c[dir] += s_cnt[dir][u]; }
        const double L = 0.5 * (t[0] / (double)(c[0] > 0 ? c[0] : 1) + t[1] / (double)(c[1] > 0 ? c[1] : 1));
        const bool any = c[0] + c[1] > 0;
        result[4 * p + 0] = any ? (float)L : 0.f;
        result[4 * p + 1] = any ? 1.f : 0.f;
        result[4 * p + 2] = (float)c[0];
        result[4 * p + 3] = (float)c[1];
    }
}

// one wave per output row: rows [0, P N) of dq, then rows [0, Mg) of dg
__global__ __launch_bounds__(256) void xt_bwd_kernel(Sides s, const uint8_t* __restrict__ q_valid, const uint8_t* __restrict__ g_valid, int P,
                                                     int N, int Mg, int D, float margin, int normalize, float eps,
                                                     const float* __restrict__ q_d, const int* __restrict__ q_idx,
                                                     const float* __restrict__ g_d, const int* __restrict__ g_idx,
                                                     const float* __restrict__ inv, const float* __restrict__ norm,
                                                     const float* __restrict__ result, const float* __restrict__ gscale,
                                                     float* __restrict__ dq, int lddq, float* __restrict__ dg, int lddg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int PN = P * N;
    if (row >= PN + Mg) return;
    const bool is_q = row < PN;
    const int me = is_q ? row % N : row - PN;                        // pair-local index
    const float* xr = is_q ? s.q + (size_t)row * s.ldq : s.g + (size_t)me * s.ldg;
    float* o = is_q ? dq + (size_t)row * lddq : dg + (size_t)me * lddg;
    const bool valid = is_q ? (!q_valid || q_valid[row]) : (!g_valid || g_valid[me]);
    f32x4 xi[NV], acc[NV];
    load_row(xi, xr, lane, D, valid);
    zero_acc(acc);
    if (valid) {                                                     // (an invalid row is no anchor and nobody's choice: zeros)
        for (int p = is_q ? row / N : 0; p < (is_q ? row / N + 1 : P); ++p) {
            // c = gscale[p] * 0.5 * l' / max(1, n) with n the active anchors of the ANCHOR's direction
            const float cq = gscale[p] * 0.5f / fmaxf(result[4 * p + 2], 1.f), cg = gscale[p] * 0.5f / fmaxf(result[4 * p + 3], 1.f);
            // "mine": the direction in which this row is an anchor; "theirs": the one whose anchors (rows of the other side) may have chosen it
            const int n_mine = is_q ? N : Mg, n_theirs = is_q ? Mg : N;
            const float* xo = is_q ? s.g : s.q + (size_t)p * N * s.ldq;                   // the other side's rows
            const int ldo = is_q ? s.ldg : s.ldq;
            const int* mi = (is_q ? q_idx : g_idx) + p * n_mine; const float* md = (is_q ? q_d : g_d) + p * n_mine;
            const int* ti = (is_q ? g_idx : q_idx) + p * n_theirs; const float* td = (is_q ? g_d : q_d) + p * n_theirs;
            add_own(acc, xi, me, xo, ldo, n_theirs, mi, mi + P * n_mine, md, md + P * n_mine, is_q ? cq : cg, margin, lane, D);
            add_chosen_by(acc, xi, me, xo, ldo, n_theirs, ti, ti + P * n_theirs, td, td + P * n_theirs, is_q ? cg : cq, margin, lane, D);
        }
        if (normalize) {
            const int r = is_q ? row : PN + me;
            if (norm[r] >= eps) {                                    // dx = (G - x^ (x^ . G)) / max(|x|, eps); the same block as in
                float dot = 0.f;                                     // hc_triplet.hip's hc_bwd_rows_kernel
#pragma unroll
                for (int v = 0; v < NV; ++v) dot += xi[v][0] * acc[v][0] + xi[v][1] * acc[v][1] + xi[v][2] * acc[v][2] + xi[v][3] * acc[v][3];
                dot = wave_sum(dot);
                const float iv = inv[r];
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

extern "C" int64_t reid_cross_triplet_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D) {
    if (int rc = check_dims("reid_cross_triplet_ws_floats", P, N, Mg, D)) return rc;
    return Ws(P, N, Mg, D).total;
}

extern "C" int reid_cross_triplet_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label,
                                      const int64_t* g_label, const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N,
                                      int32_t Mg, int32_t D, float margin, int32_t normalize, float eps, float* q_d, int32_t* q_idx,
                                      float* g_d, int32_t* g_idx, float* ws, float* result, void* stream) {
    const char* who = "reid_cross_triplet_fwd";
    REID_CHECK_ARG(q && g && q_label && g_label && q_d && q_idx && g_d && g_idx && ws && result, "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, Mg, D, ldg, "ldg")) return rc;
    if (int rc = check_scalars(who, margin, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(ws), "%s: q, g or ws is not 16-byte aligned", who);
    const Ws w(P, N, Mg, D);
    hipStream_t s = (hipStream_t)stream;
    const int PN = P * N;
    Sides sd{q, ldq, g, ldg};
    if (normalize) {
        hipLaunchKernelGGL(xt_unit_kernel, dim3((PN + Mg + 3) / 4), dim3(256), 0, s, q, ldq, g, ldg, PN, Mg, D, eps, ws + w.unit, ws + w.inv,
                           ws + w.norm);
        REID_CHECK_LAUNCH("reid_cross_triplet_fwd(unit rows)");
        sd = Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D};
    }
    const int tiles = (N + TA - 1) / TA + (Mg + TA - 1) / TA;
    hipLaunchKernelGGL(xt_fwd_kernel, dim3(P * tiles), dim3(256), 0, s, sd, q_label, g_label, q_valid, g_valid, P, N, Mg, D, margin, q_d, q_idx,
                       g_d, g_idx, ws + w.loss_q, ws + w.loss_g);
    REID_CHECK_LAUNCH("reid_cross_triplet_fwd(mine)");
    hipLaunchKernelGGL(xt_refine_kernel, dim3((P * (N + Mg) + 3) / 4), dim3(256), 0, s, sd, P, N, Mg, D, margin, q_d, q_idx, g_d, g_idx,
                       ws + w.loss_q, ws + w.loss_g);
    REID_CHECK_LAUNCH("reid_cross_triplet_fwd(refine)");
    hipLaunchKernelGGL(xt_finalize_kernel, dim3(P), dim3(256), 0, s, ws + w.loss_q, ws + w.loss_g, q_idx, g_idx, N, Mg, result);
    REID_CHECK_LAUNCH("reid_cross_triplet_fwd(finalize)");
    return REID_OK;
}

extern "C" int reid_cross_triplet_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const uint8_t* q_valid,
                                      const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg, int32_t D, float margin,
                                      int32_t normalize, float eps, const float* q_d, const int32_t* q_idx, const float* g_d,
                                      const int32_t* g_idx, const float* ws, const float* result, const float* gscale, float* dq,
                                      int32_t lddq, float* dg, int32_t lddg, void* stream) {
    const char* who = "reid_cross_triplet_bwd";
    REID_CHECK_ARG(q && g && q_d && q_idx && g_d && g_idx && ws && result && gscale && dq && dg, "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, Mg, D, ldg, "ldg")) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, lddq, "lddq")) return rc;
    if (int rc = check_ld(who, Mg, D, lddg, "lddg")) return rc;
    if (int rc = check_scalars(who, margin, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(ws) && aligned16(dq) && aligned16(dg),
                   "%s: q, g, ws, dq or dg is not 16-byte aligned", who);
    const Ws w(P, N, Mg, D);
    const int PN = P * N;
    const Sides sd = normalize ? Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D} : Sides{q, ldq, g, ldg};
    hipLaunchKernelGGL(xt_bwd_kernel, dim3((PN + Mg + 3) / 4), dim3(256), 0, (hipStream_t)stream, sd, q_valid, g_valid, P, N, Mg, D, margin,
                       normalize, eps, q_d, q_idx, g_d, g_idx, ws + w.inv, ws + w.norm, result, gscale, dq, lddq, dg, lddg);
    REID_CHECK_LAUNCH("reid_cross_triplet_bwd");
    return REID_OK;
}
