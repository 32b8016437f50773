// Hybrid memory of SpCL (Ge et al., "Self-paced Contrastive Learning with Hybrid Memory", NeurIPS 2020, sections 3.1-3.2) for gfx950,
// all fp32: ONE unit entry per training instance, V [M, D], kept across re-clusterings, and a table T [C, D] of class means that is
// kept EXACT after every update -- a cluster's class vector is the mean of its members' entries, an un-clustered instance is a class
// of its own.  The mean of dot products is the dot product with the mean, so the loss itself is reid_cluster_nce_fwd / _bwd against T
// (cluster_nce.hip: no tile loop here); this file is the memory.  include/reid_hip.h (reid_class_means, reid_hybrid_*) and DESIGN.md
// section 25 are the definition.
//
// The members of class c are order[offsets[c]] .. order[offsets[c + 1] - 1], ascending instance index (the host groups them once per
// re-labelling).  Per column d:  T_c[d] = fl(fl(sum of V_i[d] over the members, added one by one in that order) / float(n_c)): the sum
// starts FROM the first member (not from +0: a singleton class is its entry bit for bit, a -0 included), nothing is fused, the rows
// are not renormalised.
//   hyb_means_kernel      one workgroup per class, one 16-byte column chunk per thread (D / 4 threads, rounded up to whole waves).
//                         The additions of a column are a serial chain by definition; what can overlap is the gather: every thread
//                         keeps FLY member rows in flight and adds them in order when they have arrived.
//   hyb_instances_kernel  cnce_update_kernel's gather scheme keyed by INSTANCE: the wave of the lowest contributing row of an instance
//                         walks that instance's contributing rows in ascending row order (side order; a repeated index in row order),
//                         v <- m v + (1 - m) x^_r, v <- v / max(|v|, 1e-12), and is the only reader and writer of that entry.
//   hyb_refresh_kernel    one workgroup per ROW: the workgroup of the lowest contributing row of a class re-forms that class's mean
//                         from the updated V (hyb_means_kernel's body) and is the only writer of that row of T; every other
//                         workgroup leaves.  Classes without a contributing row keep their bits.
// The two update kernels run in stream order.  No atomics; nothing is allocated, synchronised or read back.
#include "cluster_nce_ws.h"

// T_c is defined with every addition and the division rounded on their own, and the blend with its two products rounded before the
// sum: no fused multiply-add in this file (as cluster_nce.hip).
#pragma clang fp contract(off)

namespace {
using triplet::NV;
using triplet::load_row;
using triplet::store_row;
using cnce::EPS;

constexpr int FLY = 16;                  // member rows a thread has in flight: 16 x 16 bytes = 64 VGPRs

// Row t of the class's member list, this thread's column chunk.
__device__ __forceinline__ f32x4 member(const float* __restrict__ col, int ldv, const int64_t* __restrict__ order, int64_t t) {
    return *(const f32x4*)(col + (size_t)order[t] * ldv);
}

// The mean of the members order[b .. e) of V for the 4 columns at `col` (V + the chunk's first column); e > b.
__device__ __forceinline__ f32x4 mean_chunk(const float* __restrict__ col, int ldv, const int64_t* __restrict__ order, int64_t b, int64_t e) {
    f32x4 acc = member(col, ldv, order, b);
    int64_t t = b + 1;
    for (; t + FLY <= e; t += FLY) {
        f32x4 xv[FLY];
#pragma unroll
        for (int u = 0; u < FLY; ++u) xv[u] = member(col, ldv, order, t + u);
#pragma unroll
        for (int u = 0; u < FLY; ++u) acc = acc + xv[u];             // (ascending: the order is part of the definition)
    }
    for (; t < e; ++t) acc = acc + member(col, ldv, order, t);
    return acc / (float)(e - b);
}

// The whole workgroup: row c of T from the members of class c.  An empty class gets zeros (the callers refuse one).
__device__ __forceinline__ void class_mean(const float* __restrict__ V, int ldv, const int64_t* __restrict__ order,
                                           const int64_t* __restrict__ offsets, int64_t c, int D, float* __restrict__ T) {
    const int col = 4 * threadIdx.x;
    if (col >= D) return;
    const int64_t b = offsets[c], e = offsets[c + 1];
    *(f32x4*)(T + (size_t)c * D + col) = e > b ? mean_chunk(V + col, ldv, order, b, e) : f32x4{0.f, 0.f, 0.f, 0.f};
}

__global__ __launch_bounds__(256) void hyb_means_kernel(const float* __restrict__ V, int ldv, const int64_t* __restrict__ order,
                                                        const int64_t* __restrict__ offsets, int D, float* __restrict__ T) {
    class_mean(V, ldv, order, offsets, blockIdx.x, D, T);
}

__global__ __launch_bounds__(256) void hyb_instances_kernel(const int64_t* __restrict__ index, const uint8_t* __restrict__ valid, int R, int N,
                                                            int D, const float* __restrict__ row_loss, const float* __restrict__ xhat,
                                                            float* __restrict__ V, int ldv, int64_t M, float mom) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t me = index[r % N];
    if (!((!valid || valid[r]) && me >= 0 && me < M && isfinite(row_loss[r]))) return;
    // lane l looks at row b + l: does it contribute to entry `me`?
    auto mine = [&](int b) {
        const int o = b + lane;
        return __ballot(o < R && index[o % N] == me && (!valid || valid[o]) && isfinite(row_loss[o]));
    };
    for (int b = 0; b < r; b += 64)                                  // an earlier contributing row of this instance: its wave does the work
        if (mine(b) & (b + 64 <= r ? ~0ull : (1ull << (r - b)) - 1)) return;
    float* v = V + (size_t)me * ldv;
    f32x4 cv[NV];
    load_row(cv, v, lane, D);
    const float keep = 1.f - mom;
    for (int b = r & ~63; b < R; b += 64) {
        unsigned long long hit = mine(b);
        if (b < r) hit &= ~((1ull << (r - b)) - 1);                  // (nobody in front of r: checked above)
        while (hit) {
            const int o = b + __builtin_ctzll(hit);
            hit &= hit - 1;
            f32x4 xv[NV];
            load_row(xv, xhat + (size_t)o * D, lane, D);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                cv[k] = cv[k] * mom + xv[k] * keep;
                const f32x4 q = cv[k] * cv[k];
                s += (q[0] + q[1]) + (q[2] + q[3]);
            }
            const float den = fmaxf(sqrtf(wave_sum(s)), EPS);
#pragma unroll
            for (int k = 0; k < NV; ++k) cv[k] = cv[k] / den;
        }
    }
    store_row(v, cv, lane, D);
}

__global__ __launch_bounds__(256) void hyb_refresh_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ valid, int R, int N,
                                                          int D, const float* __restrict__ row_loss, const float* __restrict__ V, int ldv,
                                                          const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                          float* __restrict__ T, int C) {
    const int r = blockIdx.x;                                        // (uniform: the whole workgroup stays or leaves)
    const int64_t y = labels[r % N];
    if (!((!valid || valid[r]) && y >= 0 && y < (int64_t)C && isfinite(row_loss[r]))) return;
    for (int b = 0; b < r; b += blockDim.x) {                        // an earlier contributing row of this class: its workgroup does the work
        const int o = b + threadIdx.x;
        if (__syncthreads_or(o < r && labels[o % N] == y && (!valid || valid[o]) && isfinite(row_loss[o]))) return;
    }
    class_mean(V, ldv, order, offsets, y, D, T);
}

int threads_of(int D) { return ((D / 4) + 63) & ~63; }              // one 16-byte chunk per thread, whole waves: 64 .. 256

int check_entries(const char* who, const float* V, int32_t ldv, int64_t M, int32_t D) {
    REID_CHECK_ARG(M >= 1, "%s: M=%lld (>= 1)", who, (long long)M);
    REID_CHECK_ARG(ldv >= D && ldv % 4 == 0, "%s: ldv=%d (a multiple of 4, >= D=%d)", who, ldv, D);
    REID_CHECK_ARG(triplet::aligned16(V), "%s: V is not 16-byte aligned", who);
    return REID_OK;
}

}  // namespace

extern "C" int reid_class_means(const float* V, int32_t ldv, int64_t M, const int64_t* order, const int64_t* offsets, int32_t C, int32_t D,
                                float* T, void* stream) {
    const char* who = "reid_class_means";
    REID_CHECK_ARG(V && order && offsets && T, "%s: null pointer", who);
    if (int rc = cnce::check_d(who, D)) return rc;
    if (int rc = cnce::check_table(who, C, D)) return rc;
    if (int rc = check_entries(who, V, ldv, M, D)) return rc;
    REID_CHECK_ARG(triplet::aligned16(T), "%s: T is not 16-byte aligned", who);
    hipLaunchKernelGGL(hyb_means_kernel, dim3(C), dim3(threads_of(D)), 0, (hipStream_t)stream, V, ldv, order, offsets, D, T);
    REID_CHECK_LAUNCH("reid_class_means");
    return REID_OK;
}

extern "C" int reid_hybrid_update_instances(const int64_t* index, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* row_loss,
                                            const float* ws, float* V, int32_t ldv, int64_t M, float momentum, void* stream) {
    const char* who = "reid_hybrid_update_instances";
    REID_CHECK_ARG(index && row_loss && ws && V, "%s: null pointer", who);
    if (int rc = cnce::check_shape(who, S, N, D)) return rc;
    if (int rc = check_entries(who, V, ldv, M, D)) return rc;
    REID_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "%s: momentum=%g (0..1)", who, (double)momentum);
    REID_CHECK_ARG(triplet::aligned16(ws), "%s: ws is not 16-byte aligned", who);
    const int R = S * N;
    const cnce::Ws w(R, D, 1);                                       // (x^ sits in front of everything that depends on the splits)
    hipLaunchKernelGGL(hyb_instances_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, index, valid, R, N, D, row_loss,
                       ws + w.xhat, V, ldv, M, momentum);
    REID_CHECK_LAUNCH("reid_hybrid_update_instances");
    return REID_OK;
}

extern "C" int reid_hybrid_refresh_classes(const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* row_loss,
                                           const float* V, int32_t ldv, int64_t M, const int64_t* order, const int64_t* offsets, float* T,
                                           int32_t C, void* stream) {
    const char* who = "reid_hybrid_refresh_classes";
    REID_CHECK_ARG(labels && row_loss && V && order && offsets && T, "%s: null pointer", who);
    if (int rc = cnce::check_shape(who, S, N, D)) return rc;
    if (int rc = cnce::check_table(who, C, D)) return rc;
    if (int rc = check_entries(who, V, ldv, M, D)) return rc;
    REID_CHECK_ARG(triplet::aligned16(T), "%s: T is not 16-byte aligned", who);
    hipLaunchKernelGGL(hyb_refresh_kernel, dim3(S * N), dim3(threads_of(D)), 0, (hipStream_t)stream, labels, valid, S * N, N, D, row_loss, V,
                       ldv, order, offsets, T, C);
    REID_CHECK_LAUNCH("reid_hybrid_refresh_classes");
    return REID_OK;
}
