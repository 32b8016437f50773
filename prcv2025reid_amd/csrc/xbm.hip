// Cross-batch memory for the cross-modal triplet loss (Wang et al., "Cross-Batch Memory for Embedding Learning", CVPR 2020) for gfx950,
// all fp32: a ring of the last M rows of every side (side 0 = vis, sides 1 .. P = the non-vis modalities) on the device, and the
// cross-modal batch-hard triplet loss of cross_triplet.hip with that ring as the candidates.  The reference has no such loss;
// include/reid_hip.h (reid_xbm_*) and DESIGN.md section 16 are the definition.
//
// The kernels here decode indices and call the pieces of triplet_mine.h (shared with triplet.hip, cross_triplet.hip and
// hc_triplet.hip); the entry points use its argument checks.
//
// Enqueue, launch 1 (xbm_enqueue_kernel): one wave per (side, row).  Row i of every side goes to slot (cursor[0] + i) mod M as its
//   unit row (triplet::unit_row: the bits of reid_l2norm_rows) or as it is; the vis side's waves write the labels, every wave its
//   validity byte.  The cursor is READ from device memory, so a replayed graph keeps filing rows where the last replay stopped.
// Enqueue, launch 2 (xbm_advance_kernel): one thread moves the cursor -- a launch of its own, behind the rows in stream order, so no
//   row launch can see it half way.
// Forward, launch 1 (xbm_unit_kernel, normalize = 1 only): the unit rows of the batch into ws, as cross_triplet.hip's xt_unit_kernel.
// Forward, launch 2 (xbm_mine_kernel): blockIdx = (pair, direction, tile of 4 anchors).  Direction q->mem: the q rows of pair p
//   against the slots of ring side 0; g->mem: the g rows against the slots of ring side p + 1.  ONE call of triplet::mine_tile with
//   NO_SELF: an anchor never meets its own side.  Indices are slot numbers.
// Forward, launch 3 (xbm_refine_kernel): one wave per anchor copies the two rows it keeps from the ring into ws and re-evaluates the
//   two distances with an fp64 sum (triplet::refine_anchor).
// Forward, launch 4 (xbm_finalize_kernel): one workgroup per pair, the ordered fp64 sums -> result [P, 4] = {L_p, flag_p, n_q, n_g}.
// Backward (xbm_bwd_kernel): one wave per output row.  The ring's rows are constants, so a row has only its own two terms as an
//   anchor (a vis row: for p ascending), taken from the COPIES in ws -- the ring may have been overwritten by later enqueues -- and
//   the projection through the normalisation in the same kernel, as xt_bwd_kernel.
// No atomics anywhere: two runs give the same bits in every output.  Nothing is allocated, synchronised or read back.
#include "triplet_mine.h"

namespace {

using namespace triplet;

// ws (floats): unit rows (P + 1) N D (q rows, then g rows) | kept rows 2 P N x 2 D (anchor slot dir * P N + p N + a: positive | negative)
// | 1 / max(|x|, eps) (P + 1) N | |x| (P + 1) N | row losses: q->mem P N, g->mem P N
struct Ws {
    int64_t unit, kept, inv, norm, loss_q, loss_g, total;
    Ws(int64_t P, int64_t N, int64_t D) {
        const int64_t R = (P + 1) * N;
        unit = 0; kept = R * D; inv = kept + 4 * P * N * D; norm = inv + R; loss_q = norm + R; loss_g = loss_q + P * N; total = loss_g + P * N;
    }
};

// wave w = side * N + i: row i of side `side` (0: g, s > 0: q rows of pair s - 1) into its slot of the ring
__global__ __launch_bounds__(256) void xbm_enqueue_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ g, int ldg,
                                                          const int64_t* __restrict__ labels, const uint8_t* __restrict__ q_valid,
                                                          const uint8_t* __restrict__ g_valid, int P, int N, int M, int D, int normalize,
                                                          float eps, float* __restrict__ rows, int64_t* __restrict__ mem_labels,
                                                          uint8_t* __restrict__ mem_valid, const int* __restrict__ cursor) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= (P + 1) * N) return;
    const int side = w / N, i = w % N;
    const int slot = (int)(((unsigned)cursor[0] + (unsigned)i) % (unsigned)M);       // inside the ring whatever the cursor holds
    const float* src = side ? q + ((size_t)(side - 1) * N + i) * ldq : g + (size_t)i * ldg;
    float* dst = rows + ((size_t)side * M + slot) * D;
    if (normalize) {
        float inv, norm;                                                             // (not kept: the forward has its own)
        unit_row(src, D, eps, dst, &inv, &norm, lane);
    } else {
        f32x4 v[NV];
        load_row(v, src, lane, D);
        store_row(dst, v, lane, D);
    }
    if (lane == 0) {
        const uint8_t* valid = side ? q_valid : g_valid;
        mem_valid[(size_t)side * M + slot] = !valid || valid[side ? (side - 1) * N + i : i] ? 1 : 0;
        if (side == 0) mem_labels[slot] = labels[i];
    }
}

// cursor = (next slot, rows ever written; the count stops at INT_MAX)
__global__ void xbm_advance_kernel(int* __restrict__ cursor, int N, int M) {
    const int c0 = cursor[0], c1 = cursor[1];
    cursor[0] = (int)(((unsigned)c0 + (unsigned)N) % (unsigned)M);
    cursor[1] = c1 > 0x7fffffff - N ? 0x7fffffff : c1 + N;
}

// rows [0, PN) are q rows, rows [PN, PN + N) are g rows; one wave per row (triplet::unit_row).  (The same body as cross_triplet.hip's
// xt_unit_kernel and hc_triplet.hip's hc_unit_kernel.)
__global__ __launch_bounds__(256) void xbm_unit_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ g, int ldg, int PN,
                                                       int N, int D, float eps, float* __restrict__ unit, float* __restrict__ inv_out,
                                                       float* __restrict__ norm_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= PN + N) return;
    unit_row(row < PN ? q + (size_t)row * ldq : g + (size_t)(row - PN) * ldg, D, eps, unit + (size_t)row * D, inv_out + row, norm_out + row,
             threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void xbm_mine_kernel(Sides s, const int64_t* __restrict__ labels, const uint8_t* __restrict__ q_valid,
                                                       const uint8_t* __restrict__ g_valid, const float* __restrict__ rows,
                                                       const int64_t* __restrict__ mem_labels, const uint8_t* __restrict__ mem_valid, int P,
                                                       int N, int M, int D, float margin, float* __restrict__ q_d, int* __restrict__ q_idx,
                                                       float* __restrict__ g_d, int* __restrict__ g_idx, float* __restrict__ loss_q,
                                                       float* __restrict__ loss_g) {
    const int tn = (N + TA - 1) / TA;
    const int p = blockIdx.x / (2 * tn), t = blockIdx.x % (2 * tn);
    const bool qm = t < tn;                                          // uniform over the workgroup; ONE call: one LDS image
    const int side = qm ? 0 : p + 1;                                 // the ring side the anchors do NOT come from
    const Rows a = qm ? Rows{s.q + (size_t)p * N * s.ldq, s.ldq, labels, q_valid ? q_valid + p * N : nullptr, N}
                      : Rows{s.g, s.ldg, labels, g_valid, N};
    const Rows c{rows + (size_t)side * M * D, D, mem_labels, mem_valid + (size_t)side * M, M};
    float* d = (qm ? q_d : g_d) + p * N;                             // [2, P N]: d_ap | d_an
    int* ix = (qm ? q_idx : g_idx) + p * N;
    mine_tile(a, c, (qm ? t : t - tn) * TA, NO_SELF, D, margin, d, d + P * N, ix, ix + P * N, (qm ? loss_q : loss_g) + p * N);
}

// One wave per anchor of either direction (w = dir * P N + p N + a): the two ring rows it keeps are copied into ws, where the backward
// finds them whatever has been enqueued since, and its two distances are re-evaluated from the same rows with an fp64 sum and rounded
// once (triplet::refine_anchor: why), its row loss from them.
__global__ __launch_bounds__(256) void xbm_refine_kernel(Sides s, const float* __restrict__ rows, int P, int N, int M, int D, float margin,
                                                         float* __restrict__ q_d, const int* __restrict__ q_idx, float* __restrict__ g_d,
                                                         const int* __restrict__ g_idx, float* __restrict__ kept,
                                                         float* __restrict__ loss_q, float* __restrict__ loss_g) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int PN = P * N;
    if (w >= 2 * PN) return;
    const bool qm = w < PN;
    const int r = qm ? w : w - PN;                                                   // r = p N + a: the anchor's slot in [P, N]
    const int p = r / N, a = r % N;
    const float* xa = qm ? s.q + (size_t)r * s.ldq : s.g + (size_t)a * s.ldg;
    const float* xc = rows + (size_t)(qm ? 0 : p + 1) * M * D;                       // the candidates' side of the ring
    float* d = qm ? q_d : g_d;
    const int* ix = qm ? q_idx : g_idx;
    const int jp = ix[r], jn = ix[PN + r];
    if (jp < 0 || jp >= M || jn < 0 || jn >= M) return;                              // not active: the zeros stay, nothing is kept
    f32x4 v[NV];
    float* k = kept + (size_t)w * 2 * D;
    load_row(v, xc + (size_t)jp * D, lane, D); store_row(k, v, lane, D);
    load_row(v, xc + (size_t)jn * D, lane, D); store_row(k + D, v, lane, D);
    float dp, dn;                                                                    // (lane 0's)
    refine_anchor(xa, xc, D, jp, jn, D, lane, dp, dn);
    if (lane == 0) {
        d[r] = dp; d[PN + r] = dn;
        (qm ? loss_q : loss_g)[r] = row_loss_of(dp - dn, margin);
    }
}

// one workgroup per pair: thread t adds rows t, t + 256, ... of a direction in fp64, the 256 sums are added in index order (the body
// of cross_triplet.hip's xt_finalize_kernel with both directions N rows long)
__global__ __launch_bounds__(256) void xbm_finalize_kernel(const float* __restrict__ loss_q, const float* __restrict__ loss_g,
                                                           const int* __restrict__ q_idx, const int* __restrict__ g_idx, int N,
                                                           float* __restrict__ result) {
    __shared__ double s_sum[2][256];
    __shared__ int s_cnt[2][256];
    const int tid = threadIdx.x, p = blockIdx.x;
    for (int dir = 0; dir < 2; ++dir) {
        const float* rl = (dir ? loss_g : loss_q) + (size_t)p * N;
        const int* ip = (dir ? g_idx : q_idx) + (size_t)p * N;
        double s = 0.0;
        int c = 0;
        for (int r = tid; r < N; r += 256)
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

// one wave per output row: rows [0, P N) of dq, then rows [0, N) of dg
__global__ __launch_bounds__(256) void xbm_bwd_kernel(Sides s, const uint8_t* __restrict__ q_valid, const uint8_t* __restrict__ g_valid, int P,
                                                      int N, int D, float margin, int normalize, float eps, const float* __restrict__ q_d,
                                                      const int* __restrict__ q_idx, const float* __restrict__ g_d,
                                                      const int* __restrict__ g_idx, const float* __restrict__ kept,
                                                      const float* __restrict__ inv, const float* __restrict__ norm,
                                                      const float* __restrict__ result, const float* __restrict__ gscale,
                                                      float* __restrict__ dq, int lddq, float* __restrict__ dg, int lddg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int PN = P * N;
    if (row >= PN + N) return;
    const bool is_q = row < PN;
    const int me = is_q ? row % N : row - PN;
    const float* xr = is_q ? s.q + (size_t)row * s.ldq : s.g + (size_t)me * s.ldg;
    float* o = is_q ? dq + (size_t)row * lddq : dg + (size_t)me * lddg;
    const bool valid = is_q ? (!q_valid || q_valid[row]) : (!g_valid || g_valid[me]);
    f32x4 xi[NV], acc[NV];
    load_row(xi, xr, lane, D, valid);
    zero_acc(acc);
    if (valid) {                                                     // (an invalid row is no anchor: zeros)
        for (int p = is_q ? row / N : 0; p < (is_q ? row / N + 1 : P); ++p) {
            // The row's two terms as an anchor of pair p, c = gscale[p] * 0.5 * l' / max(1, n) with n the active anchors of its
            // direction.  (triplet::add_own reads the chosen rows by index from the other side; here they are the two copies.)
            const int r = p * N + me;
            const int* ix = is_q ? q_idx : g_idx; const float* d = is_q ? q_d : g_d;
            if (ix[r] >= 0 && ix[PN + r] >= 0) {
                const float dp = d[r], dn = d[PN + r];
                const float c = gscale[p] * 0.5f / fmaxf(result[4 * p + (is_q ? 2 : 3)], 1.f) * row_dloss_of(dp - dn, margin);
                const float* k = kept + ((size_t)(is_q ? 0 : PN) + r) * 2 * D;
                add_term(acc, xi, k, term_scale(c, dp), lane, D);
                add_term(acc, xi, k + D, -term_scale(c, dn), lane, D);
            }
        }
        if (normalize) {
            const int r = is_q ? row : PN + me;
            if (norm[r] >= eps) {                                    // dx = (G - x^ (x^ . G)) / max(|x|, eps); the same block as in
                float dot = 0.f;                                     // cross_triplet.hip's xt_bwd_kernel
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

// the ring's own limits: N <= M <= MAX_ROWS (check_dims has P, N, M and D in their ranges)
int check_ring(const char* who, int32_t P, int32_t N, int32_t M, int32_t D) {
    if (int rc = check_dims(who, P, N, M, D)) return rc;
    REID_CHECK_ARG(N <= M, "%s: N=%d rows do not fit a memory of M=%d slots", who, N, M);
    return REID_OK;
}

}  // namespace

extern "C" int64_t reid_xbm_ws_floats(int32_t P, int32_t N, int32_t M, int32_t D) {
    if (int rc = check_ring("reid_xbm_ws_floats", P, N, M, D)) return rc;
    return Ws(P, N, D).total;
}

extern "C" int reid_xbm_enqueue(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* labels, const uint8_t* q_valid,
                                const uint8_t* g_valid, int32_t P, int32_t N, int32_t M, int32_t D, int32_t normalize, float eps,
                                float* rows, int64_t* mem_labels, uint8_t* mem_valid, int32_t* cursor, void* stream) {
    const char* who = "reid_xbm_enqueue";
    REID_CHECK_ARG(q && g && labels && rows && mem_labels && mem_valid && cursor, "%s: null pointer", who);
    if (int rc = check_ring(who, P, N, M, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, N, D, ldg, "ldg")) return rc;
    if (int rc = check_scalars(who, 0.f, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(rows), "%s: q, g or rows is not 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(xbm_enqueue_kernel, dim3(((P + 1) * N + 3) / 4), dim3(256), 0, s, q, ldq, g, ldg, labels, q_valid, g_valid, P, N, M, D,
                       normalize, eps, rows, mem_labels, mem_valid, cursor);
    REID_CHECK_LAUNCH("reid_xbm_enqueue(rows)");
    hipLaunchKernelGGL(xbm_advance_kernel, dim3(1), dim3(1), 0, s, cursor, N, M);
    REID_CHECK_LAUNCH("reid_xbm_enqueue(cursor)");
    return REID_OK;
}

extern "C" int reid_xbm_triplet_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* labels, const uint8_t* q_valid,
                                    const uint8_t* g_valid, int32_t P, int32_t N, int32_t M, int32_t D, float margin, int32_t normalize,
                                    float eps, const float* rows, const int64_t* mem_labels, const uint8_t* mem_valid, float* q_d,
                                    int32_t* q_idx, float* g_d, int32_t* g_idx, float* ws, float* result, void* stream) {
    const char* who = "reid_xbm_triplet_fwd";
    REID_CHECK_ARG(q && g && labels && rows && mem_labels && mem_valid && q_d && q_idx && g_d && g_idx && ws && result, "%s: null pointer", who);
    if (int rc = check_ring(who, P, N, M, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, N, D, ldg, "ldg")) return rc;
    if (int rc = check_scalars(who, margin, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(rows) && aligned16(ws), "%s: q, g, rows or ws is not 16-byte aligned", who);
    const Ws w(P, N, D);
    hipStream_t s = (hipStream_t)stream;
    const int PN = P * N;
    Sides sd{q, ldq, g, ldg};
    if (normalize) {
        hipLaunchKernelGGL(xbm_unit_kernel, dim3((PN + N + 3) / 4), dim3(256), 0, s, q, ldq, g, ldg, PN, N, D, eps, ws + w.unit, ws + w.inv,
                           ws + w.norm);
        REID_CHECK_LAUNCH("reid_xbm_triplet_fwd(unit rows)");
        sd = Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D};
    }
    hipLaunchKernelGGL(xbm_mine_kernel, dim3(P * 2 * ((N + TA - 1) / TA)), dim3(256), 0, s, sd, labels, q_valid, g_valid, rows, mem_labels,
                       mem_valid, P, N, M, D, margin, q_d, q_idx, g_d, g_idx, ws + w.loss_q, ws + w.loss_g);
    REID_CHECK_LAUNCH("reid_xbm_triplet_fwd(mine)");
    hipLaunchKernelGGL(xbm_refine_kernel, dim3((2 * PN + 3) / 4), dim3(256), 0, s, sd, rows, P, N, M, D, margin, q_d, q_idx, g_d, g_idx,
                       ws + w.kept, ws + w.loss_q, ws + w.loss_g);
    REID_CHECK_LAUNCH("reid_xbm_triplet_fwd(refine)");
    hipLaunchKernelGGL(xbm_finalize_kernel, dim3(P), dim3(256), 0, s, ws + w.loss_q, ws + w.loss_g, q_idx, g_idx, N, result);
    REID_CHECK_LAUNCH("reid_xbm_triplet_fwd(finalize)");
    return REID_OK;
}

extern "C" int reid_xbm_triplet_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const uint8_t* q_valid, const uint8_t* g_valid,
                                    int32_t P, int32_t N, int32_t D, float margin, int32_t normalize, float eps, const float* q_d,
                                    const int32_t* q_idx, const float* g_d, const int32_t* g_idx, const float* ws, const float* result,
                                    const float* gscale, float* dq, int32_t lddq, float* dg, int32_t lddg, void* stream) {
    const char* who = "reid_xbm_triplet_bwd";
    REID_CHECK_ARG(q && g && q_d && q_idx && g_d && g_idx && ws && result && gscale && dq && dg, "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, N, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, N, D, ldg, "ldg")) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, lddq, "lddq")) return rc;
    if (int rc = check_ld(who, N, D, lddg, "lddg")) return rc;
    if (int rc = check_scalars(who, margin, normalize, eps)) return rc;
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(ws) && aligned16(dq) && aligned16(dg),
                   "%s: q, g, ws, dq or dg is not 16-byte aligned", who);
    const Ws w(P, N, D);
    const int PN = P * N;
    const Sides sd = normalize ? Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D} : Sides{q, ldq, g, ldg};
    hipLaunchKernelGGL(xbm_bwd_kernel, dim3((PN + N + 3) / 4), dim3(256), 0, (hipStream_t)stream, sd, q_valid, g_valid, P, N, D, margin,
                       normalize, eps, q_d, q_idx, g_d, g_idx, ws + w.kept, ws + w.inv, ws + w.norm, result, gscale, dq, lddq, dg, lddg);
    REID_CHECK_LAUNCH("reid_xbm_triplet_bwd");
    return REID_OK;
}
