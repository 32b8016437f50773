// Cluster-contrast memory loss (ClusterNCE: the cluster-level memory of SpCL, Ge et al., NeurIPS 2020; Cluster-Contrast, Dai et al.,
// 2021) for gfx950, all fp32: a non-parametric classifier over ONE unit centroid per cluster, kept in a table on the device and moved by
// momentum, never by the optimizer.  The reference has no such loss; include/reid_hip.h (reid_cluster_nce_*) and DESIGN.md section 23 are
// the definition.
//
// x [S*N, D] holds S sides stacked (row s * N + i = instance i of side s), labels [N] are shared by the sides, table [K, D] holds unit rows.
//   l_rc = (x^_r . C_c) / tau,  loss = mean over the used rows of lse_c(l_rc) - l_r,y.  The [R, K] logits are never stored: a TS x TS tile
//   of x^ C^T lives in the accumulators of v_mfma_f32_32x32x2_f32 (exact fp32 products): gemm_core.h's f32_tile, which sdm.hip
//   uses too -- operands staged by LDS-DMA in lds_tile.h's swizzled 128-byte rows, double buffered over the K-steps.
// Forward:
//   1 cnce_unit_kernel     one wave per row: x^ = x / max(|x|, 1e-12), 1 / max(|x|, 1e-12) and the row's "used" flag into ws.
//   2 cnce_stat_kernel     grid (row tiles, splits): a workgroup walks the class tiles of its split; every lane carries a running
//                          (maximum, sum of exp) per accumulator element, merged over the lanes, the two waves of a row and -- in
//                          cnce_finalize_kernel -- the splits in a fixed order; the lane that holds (r, y_r) leaves the target cosine.
//   3 cnce_finalize_kernel ONE workgroup: lse, row loss and target cosine per row, the used rows' losses added in ASCENDING ROW ORDER in
//                          fp64 -> result = {sum / max(1, n_used), n_used}.
//   with gradients only (the table is streamed a second time):
//   4 cnce_grad_kernel     grid (row tiles, splits, 256-column slices of D): the tile again, p = exp(l - lse) parked in LDS (row stride
//                          TS + 1 floats), then sum_c p_rc C_c for the slice's columns on the matrix cores into per-split partials.
//   5 cnce_combine_kernel  one wave per row: the partials added in split order, G = (sum_c p C_c - C_y) / tau projected through the
//                          normalisation, H = (G - x^ (x^ . G)) / max(|x|, 1e-12) into ws: all the backward needs.
// Update (cnce_update_kernel): gather form of center_update_kernel -- the wave of the lowest contributing row of a label walks that
//   label's contributing rows in ascending order and is the only wave that touches that centroid.
// Backward (cnce_bwd_kernel): dx = (dloss / max(1, n_used)) * H from ws alone: the table may have moved since the forward.
// Centroid initialisation (cnce_centroids_kernel): one wave per cluster over the rows the host has grouped by label.
// No atomics anywhere; nothing is allocated, synchronised or read back.
#include "gemm_core.h"
#include "cluster_nce_ws.h"      // the workspace layout and the shape checks, shared with hybrid_nce.hip

// A logit is the ROUNDED product cos * (1 / tau) wherever it is formed (the running maximum, the exponent of p, l_y of the row loss):
// with K = 1 lse equals l_y bit for bit and loss and gradient are exactly 0.  A fused multiply-add would keep the product unrounded in
// some of these places, so there are none in this file (as center.hip, ema.hip, expand.hip); the matrix-core products are not affected.
#pragma clang fp contract(off)

namespace {
using namespace gemmcore;
using triplet::NV;
using triplet::load_row;
using triplet::store_row;
using triplet::zero_acc;
using cnce::MAX_SIDES;
using cnce::EPS;
using cnce::Ws;
using cnce::check_d;
using cnce::check_shape;
using cnce::check_table;

constexpr int TS = 64;                   // row tile = class tile: 4 waves as 2 x 2, one 32 x 32 MFMA tile each
constexpr int TARGET_WGS = 512;          // the class range is split until the grid has about this many workgroups (a constant: the
                                         // rule depends on the shape only, so two devices form the same sums)
constexpr int MAX_SPLITS = 64;
constexpr int SLICE = 256;               // columns of D one grad workgroup accumulates: 2 chunks of 32 per wave
constexpr float M_NONE = -3.0e38f;       // running maximum of "nothing yet": finite, so exp(m - m') never sees inf - inf
constexpr int LDS_BYTES = F32Tile<TS>::LDS_STAGE;      // f32_tile's staging buffers; the p tile (TS x (TS + 1) floats) takes them over after the K loop
constexpr int P_LD = TS + 1;
static_assert(TS * P_LD * 4 <= LDS_BYTES, "the p tile must fit the staging buffers");

struct Plan { int row_tiles, class_tiles, per_split, splits, slices; };
Plan plan_of(int R, int K, int D) {
    Plan p;
    p.row_tiles = (R + TS - 1) / TS;
    p.class_tiles = (K + TS - 1) / TS;
    int want = TARGET_WGS / p.row_tiles;
    want = want < 1 ? 1 : want > MAX_SPLITS ? MAX_SPLITS : want;
    if (want > p.class_tiles) want = p.class_tiles;
    p.per_split = (p.class_tiles + want - 1) / want;
    p.splits = (p.class_tiles + p.per_split - 1) / p.per_split;      // no empty split
    p.slices = (D + SLICE - 1) / SLICE;
    return p;
}

__device__ __forceinline__ bool row_used(const int64_t* __restrict__ labels, const uint8_t* __restrict__ valid, int r, int N, int K) {
    const int64_t y = labels[r % N];
    return (!valid || valid[r]) && y >= 0 && y < (int64_t)K;
}

// (m, s) <- the running (maximum, sum of exp(. - maximum)) of both; M_NONE / 0 is the neutral element
__device__ __forceinline__ void merge_ms(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

__global__ __launch_bounds__(256) void cnce_unit_kernel(const float* __restrict__ x, int ldx, const int64_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ valid, int R, int N, int D, int K,
                                                        float* __restrict__ xhat, float* __restrict__ used, float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    float norm;                                                      // (nobody needs |x| itself)
    triplet::unit_row(x + (size_t)r * ldx, D, EPS, xhat + (size_t)r * D, inv + r, &norm, lane);
    if (lane == 0) used[r] = row_used(labels, valid, r, N, K) ? 1.f : 0.f;
}

struct TileArgs {
    const float* xhat; const float* table; const float* used; const int64_t* labels;
    int R, N, D, K, per_split, class_tiles;
    float inv_tau;
};

__global__ __launch_bounds__(256, 2) void cnce_stat_kernel(const TileArgs p, float* __restrict__ part, float* __restrict__ tgt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int l_y[TS];                            // the row's label, -1 for a row that is not used (or past R)
    __shared__ float l_ms[2][TS][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * TS, split = blockIdx.y;
    if (tid < TS) {
        const int r = m0 + tid;
        l_y[tid] = (r < p.R && p.used[r] != 0.f) ? (int)p.labels[r % p.N] : -1;
    }                                                  // (read after the barriers of the first f32_tile)
    const int j = lane & 31, h = lane >> 5;
    float mx[16], sm[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { mx[r] = M_NONE; sm[r] = 0.f; }
    const int ct1 = min((split + 1) * p.per_split, p.class_tiles);
    for (int ct = split * p.per_split; ct < ct1; ++ct) {
        const int n0 = ct * TS;
        f32x16_t tile[1][1];       // [m][n] on (reg, lane): m = 32 wm + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), n = 32 wn + (lane & 31)
        f32_tile<TS>(p.xhat + (size_t)m0 * p.D, p.R - 1 - m0, p.table + (size_t)n0 * p.D, p.K - 1 - n0, p.D, smem, tile);
        const f32x16_t& acc = tile[0][0];
        const int col = n0 + wn * 32 + j;
        if (col < p.K) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = acc[r] * p.inv_tau;          // (rounded on its own: the finalize kernel forms l_y by the same product)
                const float mn = fmaxf(mx[r], v);      // (a NaN logit: the maximum stays, the sum turns NaN)
                sm[r] = sm[r] * expf(mx[r] - mn) + expf(v - mn);
                mx[r] = mn;
                if (l_y[ml] == col) tgt[m0 + ml] = acc[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) merge_ms(mx[r], sm[r], __shfl_xor(mx[r], o, 64), __shfl_xor(sm[r], o, 64));
        if (j == 0) {
            const int ml = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            l_ms[wn][ml][0] = mx[r]; l_ms[wn][ml][1] = sm[r];
        }
    }
    __syncthreads();
    if (tid < TS && m0 + tid < p.R) {
        float m = l_ms[0][tid][0], s = l_ms[0][tid][1];
        merge_ms(m, s, l_ms[1][tid][0], l_ms[1][tid][1]);
        float* o = part + ((size_t)split * p.R + m0 + tid) * 2;
        o[0] = m; o[1] = s;
    }
}

__global__ __launch_bounds__(256) void cnce_finalize_kernel(const float* __restrict__ part, const float* __restrict__ tgt,
                                                            const float* __restrict__ used, int R, int splits, float inv_tau,
                                                            float* __restrict__ lse_out, float* __restrict__ row_loss,
                                                            float* __restrict__ tcos, float* __restrict__ result) {
    __shared__ float s_loss[256];
    __shared__ float s_used[256];
    const int tid = threadIdx.x;
    double sum = 0.0;                                                // (thread 0's)
    int n = 0;
    for (int r0 = 0; r0 < R; r0 += 256) {
        __syncthreads();                                             // the previous piece has been added
        const int r = r0 + tid;
        if (r < R) {
            const bool u = used[r] != 0.f;
            float m = M_NONE, s = 0.f;
            for (int k = 0; k < splits; ++k) merge_ms(m, s, part[((size_t)k * R + r) * 2], part[((size_t)k * R + r) * 2 + 1]);
            const float lse = m + logf(s);
            const float tc = u ? tgt[r] : 0.f;
            const float l = u ? lse - tc * inv_tau : 0.f;      // (no fused multiply-add: K = 1 gives lse = l_y and a loss of exactly 0)
            lse_out[r] = lse; tcos[r] = tc; row_loss[r] = l;
            s_loss[tid] = l; s_used[tid] = u ? 1.f : 0.f;
        }
        __syncthreads();
        if (tid == 0) {
            const int m = min(256, R - r0);
            for (int u = 0; u < m; ++u)
                if (s_used[u] != 0.f) { sum += (double)s_loss[u]; ++n; }
        }
    }
    if (tid == 0) {
        result[0] = (float)(sum / (double)(n > 0 ? n : 1));
        result[1] = (float)n;
    }
}

__global__ __launch_bounds__(256, 2) void cnce_grad_kernel(const TileArgs p, const float* __restrict__ lse, float* __restrict__ gpart) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float l_lse[TS];                        // +inf for a row that is not used: p = exp(l - inf) = 0
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * TS, split = blockIdx.y, chunk0 = blockIdx.z * (SLICE / 32);
    if (tid < TS) {
        const int r = m0 + tid;
        l_lse[tid] = (r < p.R && p.used[r] != 0.f) ? lse[r] : INFINITY;
    }
    const int i = lane & 31, h = lane >> 5;
    float* ps = (float*)smem;                          // [TS][P_LD], over the (idle) staging buffers
    f32x16_t g[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[q][a][r] = 0.f;
    const int ct1 = min((split + 1) * p.per_split, p.class_tiles);
    for (int ct = split * p.per_split; ct < ct1; ++ct) {
        const int n0 = ct * TS;
        f32x16_t tile[1][1];       // [m][n] on (reg, lane): m = 32 wm + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), n = 32 wn + (lane & 31)
        f32_tile<TS>(p.xhat + (size_t)m0 * p.D, p.R - 1 - m0, p.table + (size_t)n0 * p.D, p.K - 1 - n0, p.D, smem, tile);
        const f32x16_t& acc = tile[0][0];
        const int nl = wn * 32 + i;
        const bool ok = n0 + nl < p.K;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ml = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            ps[ml * P_LD + nl] = ok ? expf(acc[r] * p.inv_tau - l_lse[ml]) : 0.f;       // (the logit the first pass saw)
        }
        __syncthreads();
        const int k_max = p.K - 1 - n0;                // class rows past K: p is 0 and so is the operand (0 * a non-finite C[K - 1] = NaN)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = chunk0 + wave + 4 * q;       // wave-uniform
            if (c < (p.D >> 5)) {
                const float* bcol = p.table + (size_t)n0 * p.D + 32 * c + i;
#pragma unroll 4
                for (int s = 0; s < TS / 2; ++s) {
                    const int k = 2 * s + h;
                    const float bv = k <= k_max ? bcol[(size_t)k * p.D] : 0.f;
#pragma unroll
                    for (int a = 0; a < 2; ++a) g[q][a] = mfma_f32(ps[(32 * a + i) * P_LD + k], bv, g[q][a]);
                }
            }
        }
        __syncthreads();                               // the p tile has been read: the next tile may stage over it
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = chunk0 + wave + 4 * q;
        if (c < (p.D >> 5)) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (row < p.R) gpart[((size_t)split * p.R + row) * p.D + 32 * c + i] = g[q][a][r];
                }
        }
    }
}

__global__ __launch_bounds__(256) void cnce_combine_kernel(const float* __restrict__ gpart, int splits, const float* __restrict__ table,
                                                           const int64_t* __restrict__ labels, const float* __restrict__ used,
                                                           const float* __restrict__ xhat, const float* __restrict__ inv, int R, int N,
                                                           int D, float inv_tau, float* __restrict__ H) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    f32x4 acc[NV];
    zero_acc(acc);
    if (used[r] != 0.f) {
        for (int k = 0; k < splits; ++k) {
            f32x4 gv[NV];
            load_row(gv, gpart + ((size_t)k * R + r) * D, lane, D);
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = acc[v] + gv[v];
        }
        f32x4 cy[NV], xh[NV];
        load_row(cy, table + (size_t)labels[r % N] * D, lane, D);
        load_row(xh, xhat + (size_t)r * D, lane, D);
        float dot = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            acc[v] = (acc[v] - cy[v]) * inv_tau;
            const f32x4 q = xh[v] * acc[v];
            dot += (q[0] + q[1]) + (q[2] + q[3]);
        }
        dot = wave_sum(dot);
        const float rn = inv[r];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = (acc[v] - xh[v] * dot) * rn;
    }
    store_row(H + (size_t)r * D, acc, lane, D);
}

__global__ __launch_bounds__(256) void cnce_update_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ valid, int R,
                                                          int N, int D, const float* __restrict__ row_loss, const float* __restrict__ tcos,
                                                          const float* __restrict__ xhat, float* __restrict__ table, int K, float mom,
                                                          int hard) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    if (!row_used(labels, valid, r, N, K) || !isfinite(row_loss[r])) return;
    const int64_t y = labels[r % N];
    // lane l looks at row b + l: does it contribute to centroid y?
    auto mine = [&](int b) {
        const int o = b + lane;
        return __ballot(o < R && labels[o % N] == y && (!valid || valid[o]) && isfinite(row_loss[o]));
    };
    for (int b = 0; b < r; b += 64)                                  // an earlier contributing row of this label: its wave does the work
        if (mine(b) & (b + 64 <= r ? ~0ull : (1ull << (r - b)) - 1)) return;
    float* c = table + (size_t)y * D;
    f32x4 cv[NV];
    load_row(cv, c, lane, D);
    const float keep = 1.f - mom;
    auto blend = [&](int o) {
        f32x4 xv[NV];
        load_row(xv, xhat + (size_t)o * D, lane, D);
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            cv[v] = cv[v] * mom + xv[v] * keep;
            const f32x4 q = cv[v] * cv[v];
            s += (q[0] + q[1]) + (q[2] + q[3]);
        }
        const float den = fmaxf(sqrtf(wave_sum(s)), EPS);
#pragma unroll
        for (int v = 0; v < NV; ++v) cv[v] = cv[v] / den;
    };
    int best = r;                                                    // 'hard': the contributing row with the smallest target cosine
    float best_cos = tcos[r];
    for (int b = r & ~63; b < R; b += 64) {
        unsigned long long hit = mine(b);
        if (b < r) hit &= ~((1ull << (r - b)) - 1);                  // (nobody in front of r: checked above)
        while (hit) {
            const int o = b + __builtin_ctzll(hit);
            hit &= hit - 1;
            if (!hard) blend(o);
            else if (tcos[o] < best_cos) { best = o; best_cos = tcos[o]; }      // (ascending rows, strict <: ties go to the lowest row)
        }
    }
    if (hard) blend(best);
    store_row(c, cv, lane, D);
}

__global__ __launch_bounds__(256) void cnce_bwd_kernel(int R, int D, const float* __restrict__ H, const float* __restrict__ used,
                                                       const float* __restrict__ result, const float* __restrict__ dloss,
                                                       float* __restrict__ dx, int lddx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    const float coef = dloss[0] / fmaxf(1.0f, result[1]);
    f32x4 hv[NV];
    load_row(hv, H + (size_t)r * D, lane, D, used[r] != 0.f);        // (an unused row: zeros whatever coef is)
    if (used[r] != 0.f) {
#pragma unroll
        for (int v = 0; v < NV; ++v) hv[v] = hv[v] * coef;
    }
    store_row(dx + (size_t)r * lddx, hv, lane, D);
}

// cluster k = rows order[offsets[k]] .. order[offsets[k + 1] - 1] of feats, as the host has grouped them (ascending row index inside a
// cluster): the fp32 sum in that order, divided by the count, normalised.  An empty cluster gets zeros (the callers refuse one).
__global__ __launch_bounds__(256) void cnce_centroids_kernel(const float* __restrict__ feats, int ldf, const int64_t* __restrict__ order,
                                                             const int64_t* __restrict__ offsets, int K, int D, float* __restrict__ table) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (k >= K) return;
    const int64_t b = offsets[k], e = offsets[k + 1];
    f32x4 acc[NV];
    zero_acc(acc);
    for (int64_t t = b; t < e; ++t) {
        f32x4 xv[NV];
        load_row(xv, feats + (size_t)order[t] * ldf, lane, D);
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = acc[v] + xv[v];
    }
    if (e > b) {
        const float cnt = (float)(e - b);
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            acc[v] = acc[v] / cnt;
            const f32x4 q = acc[v] * acc[v];
            s += (q[0] + q[1]) + (q[2] + q[3]);
        }
        const float den = fmaxf(sqrtf(wave_sum(s)), EPS);
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = acc[v] / den;
    }
    store_row(table + (size_t)k * D, acc, lane, D);
}

}  // namespace

extern "C" int64_t reid_cluster_nce_ws_floats(int32_t S, int32_t N, int32_t D, int32_t K) {
    const char* who = "reid_cluster_nce_ws_floats";
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = check_table(who, K, D)) return rc;
    return Ws((int64_t)S * N, D, plan_of(S * N, K, D).splits).total;
}

extern "C" int reid_cluster_nce_plan(int32_t R, int32_t K, int32_t D, int32_t* plan) {
    const char* who = "reid_cluster_nce_plan";
    REID_CHECK_ARG(plan, "%s: null pointer", who);
    REID_CHECK_ARG(R >= 1 && R <= MAX_SIDES * triplet::MAX_ROWS, "%s: R=%d (1..73728)", who, R);
    if (int rc = check_d(who, D)) return rc;
    if (int rc = check_table(who, K, D)) return rc;
    const Plan p = plan_of(R, K, D);
    plan[0] = TS; plan[1] = TS; plan[2] = p.splits; plan[3] = p.per_split;
    return REID_OK;
}

extern "C" int reid_cluster_nce_fwd(const float* x, int32_t ldx, const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N,
                                    int32_t D, const float* table, int32_t K, float tau, int32_t with_grad, float* ws, float* row_loss,
                                    float* target_cos, float* result, void* stream) {
    const char* who = "reid_cluster_nce_fwd";
    REID_CHECK_ARG(x && labels && table && ws && row_loss && target_cos && result, "%s: null pointer", who);
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = check_table(who, K, D)) return rc;
    if (int rc = triplet::check_ld(who, (int64_t)S * N, D, ldx, "ldx")) return rc;
    REID_CHECK_ARG(tau > 0.f && tau - tau == 0.f, "%s: tau=%g (> 0, finite)", who, (double)tau);
    REID_CHECK_ARG(with_grad == 0 || with_grad == 1, "%s: with_grad=%d (0 or 1)", who, with_grad);
    REID_CHECK_ARG(triplet::aligned16(x) && triplet::aligned16(table) && triplet::aligned16(ws), "%s: x, table or ws is not 16-byte aligned", who);
    const int R = S * N;
    const Plan pl = plan_of(R, K, D);
    const Ws w(R, D, pl.splits);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cnce_unit_kernel, dim3((R + 3) / 4), dim3(256), 0, s, x, ldx, labels, valid, R, N, D, K, ws + w.xhat, ws + w.used,
                       ws + w.inv);
    REID_CHECK_LAUNCH("reid_cluster_nce_fwd(unit)");
    TileArgs p{};
    p.xhat = ws + w.xhat; p.table = table; p.used = ws + w.used; p.labels = labels;
    p.R = R; p.N = N; p.D = D; p.K = K; p.per_split = pl.per_split; p.class_tiles = pl.class_tiles;
    p.inv_tau = 1.0f / tau;
    hipLaunchKernelGGL(cnce_stat_kernel, dim3(pl.row_tiles, pl.splits), dim3(256), LDS_BYTES, s, p, ws + w.part, ws + w.tgt);
    REID_CHECK_LAUNCH("reid_cluster_nce_fwd(stat)");
    hipLaunchKernelGGL(cnce_finalize_kernel, dim3(1), dim3(256), 0, s, ws + w.part, ws + w.tgt, ws + w.used, R, pl.splits, p.inv_tau,
                       ws + w.lse, row_loss, target_cos, result);
    REID_CHECK_LAUNCH("reid_cluster_nce_fwd(finalize)");
    if (with_grad) {
        hipLaunchKernelGGL(cnce_grad_kernel, dim3(pl.row_tiles, pl.splits, pl.slices), dim3(256), LDS_BYTES, s, p, ws + w.lse, ws + w.gpart);
        REID_CHECK_LAUNCH("reid_cluster_nce_fwd(grad)");
        hipLaunchKernelGGL(cnce_combine_kernel, dim3((R + 3) / 4), dim3(256), 0, s, ws + w.gpart, pl.splits, table, labels, ws + w.used,
                           ws + w.xhat, ws + w.inv, R, N, D, p.inv_tau, ws + w.h);
        REID_CHECK_LAUNCH("reid_cluster_nce_fwd(combine)");
    }
    return REID_OK;
}

extern "C" int reid_cluster_nce_update(const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* row_loss,
                                       const float* target_cos, const float* ws, float* table, int32_t K, float momentum, int32_t mode,
                                       void* stream) {
    const char* who = "reid_cluster_nce_update";
    REID_CHECK_ARG(labels && row_loss && target_cos && ws && table, "%s: null pointer", who);
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = check_table(who, K, D)) return rc;
    REID_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "%s: momentum=%g (0..1)", who, (double)momentum);
    REID_CHECK_ARG(mode == REID_CLUSTER_NCE_MEAN || mode == REID_CLUSTER_NCE_HARD, "%s: mode=%d (0 = mean, 1 = hard)", who, mode);
    REID_CHECK_ARG(triplet::aligned16(table) && triplet::aligned16(ws), "%s: table or ws is not 16-byte aligned", who);
    const int R = S * N;
    const Ws w(R, D, 1);                                             // (x^ sits in front of everything that depends on the splits)
    hipLaunchKernelGGL(cnce_update_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, labels, valid, R, N, D, row_loss, target_cos,
                       ws + w.xhat, table, K, momentum, mode);
    REID_CHECK_LAUNCH("reid_cluster_nce_update");
    return REID_OK;
}

extern "C" int reid_cluster_nce_bwd(int32_t S, int32_t N, int32_t D, const float* ws, const float* result, const float* dloss, float* dx,
                                    int32_t lddx, void* stream) {
    const char* who = "reid_cluster_nce_bwd";
    REID_CHECK_ARG(ws && result && dloss && dx, "%s: null pointer", who);
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = triplet::check_ld(who, (int64_t)S * N, D, lddx, "lddx")) return rc;
    REID_CHECK_ARG(triplet::aligned16(ws) && triplet::aligned16(dx), "%s: ws or dx is not 16-byte aligned", who);
    const int R = S * N;
    const Ws w(R, D, 1);
    hipLaunchKernelGGL(cnce_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, R, D, ws + w.h, ws + w.used, result, dloss, dx,
                       lddx);
    REID_CHECK_LAUNCH("reid_cluster_nce_bwd");
    return REID_OK;
}

extern "C" int reid_cluster_centroids(const float* feats, int32_t ldf, int64_t rows, const int64_t* order, const int64_t* offsets, int32_t K,
                                      int32_t D, float* table, void* stream) {
    const char* who = "reid_cluster_centroids";
    REID_CHECK_ARG(feats && order && offsets && table, "%s: null pointer", who);
    if (int rc = check_d(who, D)) return rc;
    if (int rc = check_table(who, K, D)) return rc;
    REID_CHECK_ARG(rows >= 1, "%s: rows=%lld (>= 1)", who, (long long)rows);
    if (int rc = triplet::check_ld(who, rows, D, ldf, "ldf")) return rc;
    REID_CHECK_ARG(triplet::aligned16(feats) && triplet::aligned16(table), "%s: feats or table is not 16-byte aligned", who);
    hipLaunchKernelGGL(cnce_centroids_kernel, dim3((K + 3) / 4), dim3(256), 0, (hipStream_t)stream, feats, ldf, order, offsets, K, D, table);
    REID_CHECK_LAUNCH("reid_cluster_centroids");
    return REID_OK;
}
