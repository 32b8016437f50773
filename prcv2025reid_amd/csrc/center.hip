// Center loss (Wen et al., "A Discriminative Feature Learning Approach for Deep Face Recognition", ECCV 2016; next to the triplet loss
// in Luo et al., "Bag of Tricks and A Strong Baseline for Deep Person Re-identification", 2019) for gfx950, all fp32: one centre per
// identity in a table on the device, every used row pulled towards the centre of its label, and Wen's update of the centres the
// forward has just used.  The reference has no such loss; include/reid_hip.h (reid_center_*) and DESIGN.md section 19 are the definition.
//
// x [S*N, D] holds S sides stacked (row s * N + i = instance i of side s), labels [N] are shared by the sides.  One wave64 per row in
// every row kernel, the row as NV 16-byte chunks per lane (triplet_mine.h's load_row / store_row).
// Forward, launch 1 (center_fwd_kernel): diff = x - centers[y] into ws, d2 = sum diff^2 (per-lane partial sums, then wave_sum), the
//   row's "used" flag into ws.  An unused row (invalid, or a label outside [0, C)) never touches the table: zeros.
// Forward, launch 2 (center_finalize_kernel): ONE workgroup; its 256 threads stage 256 rows at a time in LDS, thread 0 adds the used
//   rows' d2 in ASCENDING ROW ORDER in fp64 -> result = {0.5 * sum / max(1, n_used), n_used}.
// Update (center_update_kernel): gather form.  The wave of row r leaves at once unless r is the lowest-index contributing row of its
//   label (contributing = used and d2 finite); the leader adds -diff of the label's contributing rows in ascending row order, divides
//   by 1 + n_j and moves its centre row -- the only wave that reads or writes that row, so no atomics and two runs give the same bits.
// Backward (center_bwd_kernel): dx = (dloss / max(1, n_used)) * diff from ws alone: the table may have moved since the forward.
// Nothing is allocated, synchronised or read back.
#include "triplet_mine.h"

// The definition rounds every difference, sum, quotient and product once so that a float32 loop on the host reproduces the bits of
// diff, of the updated centres and of dx: no fused multiply-adds in this file (as ema.hip, expand.hip).
#pragma clang fp contract(off)

namespace {

using triplet::NV;
using triplet::load_row;
using triplet::store_row;
using triplet::zero_acc;

constexpr int MAX_SIDES = 9;

// ws (floats): diff S N D | used flags (1.f / 0.f) S N
struct Ws {
    int64_t diff, used, total;
    Ws(int64_t S, int64_t N, int64_t D) { diff = 0; used = S * N * D; total = used + S * N; }
};

__device__ __forceinline__ bool row_used(const int64_t* __restrict__ labels, const uint8_t* __restrict__ valid, int r, int N, int C) {
    const int64_t y = labels[r % N];
    return (!valid || valid[r]) && y >= 0 && y < (int64_t)C;
}

__global__ __launch_bounds__(256) void center_fwd_kernel(const float* __restrict__ x, int ldx, const int64_t* __restrict__ labels,
                                                         const uint8_t* __restrict__ valid, int R, int N, int D,
                                                         const float* __restrict__ centers, int C, float* __restrict__ diff,
                                                         float* __restrict__ used_out, float* __restrict__ d2) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    const bool used = row_used(labels, valid, r, N, C);
    f32x4 xv[NV], cv[NV];
    load_row(xv, x + (size_t)r * ldx, lane, D, used);
    load_row(cv, centers + (size_t)(used ? labels[r % N] : 0) * D, lane, D, used);     // (an unused row reads no centre)
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        xv[v] = xv[v] - cv[v];
        const f32x4 q = xv[v] * xv[v];
        s += (q[0] + q[1]) + (q[2] + q[3]);
    }
    store_row(diff + (size_t)r * D, xv, lane, D);
    s = wave_sum(s);
    if (lane == 0) {
        d2[r] = used ? s : 0.f;
        used_out[r] = used ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void center_finalize_kernel(const float* __restrict__ d2, const float* __restrict__ used, int R,
                                                              float* __restrict__ result) {
    __shared__ float s_d2[256];
    __shared__ float s_used[256];
    const int tid = threadIdx.x;
    double sum = 0.0;                                                // (thread 0's)
    int n = 0;
    for (int r0 = 0; r0 < R; r0 += 256) {
        __syncthreads();                                             // the previous piece has been added
        if (r0 + tid < R) { s_d2[tid] = d2[r0 + tid]; s_used[tid] = used[r0 + tid]; }
        __syncthreads();
        if (tid == 0) {
            const int m = min(256, R - r0);
            for (int u = 0; u < m; ++u)
                if (s_used[u] != 0.f) { sum += (double)s_d2[u]; ++n; }
        }
    }
    if (tid == 0) {
        result[0] = (float)(0.5 * sum / (double)(n > 0 ? n : 1));
        result[1] = (float)n;
    }
}

__global__ __launch_bounds__(256) void center_update_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ valid, int R,
                                                            int N, int D, const float* __restrict__ d2, const float* __restrict__ diff,
                                                            float* __restrict__ centers, int C, float alpha) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    if (!row_used(labels, valid, r, N, C) || !isfinite(d2[r])) return;
    const int64_t y = labels[r % N];
    // lane l looks at row b + l: does it contribute to centre y?
    auto mine = [&](int b) {
        const int o = b + lane;
        return __ballot(o < R && labels[o % N] == y && (!valid || valid[o]) && isfinite(d2[o]));
    };
    for (int b = 0; b < r; b += 64)                                  // an earlier contributing row of this label: its wave does the work
        if (mine(b) & (b + 64 <= r ? ~0ull : (1ull << (r - b)) - 1)) return;
    f32x4 acc[NV];
    zero_acc(acc);
    int n = 0;
    for (int b = r & ~63; b < R; b += 64) {
        unsigned long long hit = mine(b);
        if (b < r) hit &= ~((1ull << (r - b)) - 1);                  // (nobody in front of r: checked above)
        while (hit) {
            const int o = b + __builtin_ctzll(hit);
            hit &= hit - 1;
            f32x4 dv[NV];
            load_row(dv, diff + (size_t)o * D, lane, D);
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = acc[v] + (-dv[v]);
            ++n;
        }
    }
    const float den = (float)(1 + n);
    float* c = centers + (size_t)y * D;
    f32x4 cv[NV];
    load_row(cv, c, lane, D);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const f32x4 delta = acc[v] / den;
        const f32x4 step = delta * alpha;
        cv[v] = cv[v] - step;
    }
    store_row(c, cv, lane, D);
}

__global__ __launch_bounds__(256) void center_bwd_kernel(int R, int D, const float* __restrict__ diff, const float* __restrict__ used,
                                                         const float* __restrict__ result, const float* __restrict__ dloss,
                                                         float* __restrict__ dx, int lddx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    const float coef = dloss[0] / fmaxf(1.0f, result[1]);
    f32x4 dv[NV];
    load_row(dv, diff + (size_t)r * D, lane, D, used[r] != 0.f);     // (an unused row: zeros whatever coef is)
    if (used[r] != 0.f) {
#pragma unroll
        for (int v = 0; v < NV; ++v) dv[v] = dv[v] * coef;
    }
    store_row(dx + (size_t)r * lddx, dv, lane, D);
}

int check_shape(const char* who, int32_t S, int32_t N, int32_t D) {
    REID_CHECK_ARG(S >= 1 && S <= MAX_SIDES, "%s: S=%d (1..9)", who, S);
    REID_CHECK_ARG(N >= 1 && N <= triplet::MAX_ROWS, "%s: N=%d (1..8192)", who, N);
    return triplet::check_d(who, D);                                 // (S N D <= 9 * 8192 * 1024 < 2^31: diff [S N, D] fits)
}

int check_table(const char* who, int32_t C, int32_t D) {
    REID_CHECK_ARG(C >= 1, "%s: C=%d (>= 1)", who, C);
    REID_CHECK_ARG((int64_t)C * D < (1ll << 31), "%s: C * D beyond 2^31 elements", who);
    return REID_OK;
}

}  // namespace

extern "C" int64_t reid_center_ws_floats(int32_t S, int32_t N, int32_t D) {
    if (int rc = check_shape("reid_center_ws_floats", S, N, D)) return rc;
    return Ws(S, N, D).total;
}

extern "C" int reid_center_fwd(const float* x, int32_t ldx, const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D,
                               const float* centers, int32_t C, float* ws, float* d2, float* result, void* stream) {
    const char* who = "reid_center_fwd";
    REID_CHECK_ARG(x && labels && centers && ws && d2 && result, "%s: null pointer", who);
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = check_table(who, C, D)) return rc;
    if (int rc = triplet::check_ld(who, (int64_t)S * N, D, ldx, "ldx")) return rc;
    REID_CHECK_ARG(triplet::aligned16(x) && triplet::aligned16(centers) && triplet::aligned16(ws), "%s: x, centers or ws is not 16-byte aligned", who);
    const Ws w(S, N, D);
    const int R = S * N;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(center_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, x, ldx, labels, valid, R, N, D, centers, C, ws + w.diff,
                       ws + w.used, d2);
    REID_CHECK_LAUNCH("reid_center_fwd(rows)");
    hipLaunchKernelGGL(center_finalize_kernel, dim3(1), dim3(256), 0, s, d2, ws + w.used, R, result);
    REID_CHECK_LAUNCH("reid_center_fwd(finalize)");
    return REID_OK;
}

extern "C" int reid_center_update(const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* d2,
                                  const float* ws, float* centers, int32_t C, float alpha, void* stream) {
    const char* who = "reid_center_update";
    REID_CHECK_ARG(labels && d2 && ws && centers, "%s: null pointer", who);
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = check_table(who, C, D)) return rc;
    REID_CHECK_ARG(alpha - alpha == 0.f, "%s: alpha=%g is not finite", who, (double)alpha);
    REID_CHECK_ARG(triplet::aligned16(centers) && triplet::aligned16(ws), "%s: centers or ws is not 16-byte aligned", who);
    const Ws w(S, N, D);
    const int R = S * N;
    hipLaunchKernelGGL(center_update_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, labels, valid, R, N, D, d2, ws + w.diff,
                       centers, C, alpha);
    REID_CHECK_LAUNCH("reid_center_update");
    return REID_OK;
}

extern "C" int reid_center_bwd(int32_t S, int32_t N, int32_t D, const float* ws, const float* result, const float* dloss, float* dx,
                               int32_t lddx, void* stream) {
    const char* who = "reid_center_bwd";
    REID_CHECK_ARG(ws && result && dloss && dx, "%s: null pointer", who);
    if (int rc = check_shape(who, S, N, D)) return rc;
    if (int rc = triplet::check_ld(who, (int64_t)S * N, D, lddx, "lddx")) return rc;
    REID_CHECK_ARG(triplet::aligned16(ws) && triplet::aligned16(dx), "%s: ws or dx is not 16-byte aligned", who);
    const Ws w(S, N, D);
    const int R = S * N;
    hipLaunchKernelGGL(center_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, R, D, ws + w.diff, ws + w.used, result, dloss,
                       dx, lddx);
    REID_CHECK_LAUNCH("reid_center_bwd");
    return REID_OK;
}
