// Batch-hard triplet loss (Hermans et al. 2017) on the fused pre-BN feature for gfx950, all fp32.  The reference has no such loss.
//
//   d2(i,j) = sum_c (x_ic - x_jc)^2   -- the DIFFERENCE form on the vector ALU.  The fused feature is mostly batch mean (|mean| / std per
//   column reaches 25-65), so the Gram form |x|^2 + |y|^2 - 2 x.y loses 4e-4 .. 4.5e-3 of d2 in fp32 -- more than the gap between the
//   hardest and the second-hardest candidate -- while the difference form stays at D * 2^-24 whatever the mean.
//   The whole problem is 3 B^2 D flop (1.6 GFLOP at B = 1024): the matrix cores are not needed.
//
// Forward, launch 1 (triplet_fwd_kernel): a workgroup owns TA = 4 anchors and mines them against all rows with triplet::mine_tile
//   (triplet_mine.h: one candidate per lane, 256-row pieces staged through padded LDS rows).
// Forward, launch 2 (triplet_finalize_kernel): ONE workgroup adds row_loss in a fixed order in fp64 -> result = {loss, n_active}.
// Backward (triplet_bwd_kernel): gather form, one wave per output row i: its own two terms, then every anchor a in ascending order whose
//   idx_p[a] or idx_n[a] is i.  No atomics anywhere: two runs give the same bits in every output.
// triplet_mine.h is shared with cross_triplet.hip and hc_triplet.hip; from it come the mining loop, the row helpers and the two halves
// of the gather form (add_own, add_chosen_by) of the kernels here, and the D / leading-dimension checks of the entry points.
#include "triplet_mine.h"

namespace {

using namespace triplet;

__global__ __launch_bounds__(256) void triplet_fwd_kernel(const float* __restrict__ x, int ldx, const int64_t* __restrict__ labels,
                                                          const uint8_t* __restrict__ valid, int rows, int D, float margin,
                                                          float* __restrict__ d_ap, float* __restrict__ d_an, int* __restrict__ idx_p,
                                                          int* __restrict__ idx_n, float* __restrict__ row_loss) {
    const Rows all{x, ldx, labels, valid, rows};
    const int a0 = blockIdx.x * TA;
    mine_tile(all, all, a0, a0, D, margin, d_ap, d_an, idx_p, idx_n, row_loss);      // a row is no positive of itself
}

// one workgroup: thread t adds rows t, t + 256, ... in fp64, the 256 sums are added in index order (the same tail, with more sums
// and counts, ends xt_finalize_kernel and hc_finalize_kernel)
__global__ __launch_bounds__(256) void triplet_finalize_kernel(const float* __restrict__ row_loss, const int* __restrict__ idx_p, int rows,
                                                               float* __restrict__ result) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    int n = 0;
    for (int r = tid; r < rows; r += 256)
        if (idx_p[r] >= 0) { s += (double)row_loss[r]; ++n; }
    s_sum[tid] = s; s_cnt[tid] = n;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        int c = 0;
        for (int u = 0; u < 256; ++u) { t += s_sum[u]; c += s_cnt[u]; }
        result[0] = (float)(t / (double)(c > 0 ? c : 1));
        result[1] = (float)c;
    }
}

// one wave per output row
__global__ __launch_bounds__(256) void triplet_bwd_kernel(const float* __restrict__ x, int ldx, int rows, int D, float margin,
                                                          const float* __restrict__ d_ap, const float* __restrict__ d_an,
                                                          const int* __restrict__ idx_p, const int* __restrict__ idx_n,
                                                          const float* __restrict__ result, const float* __restrict__ dloss,
                                                          float* __restrict__ dx, int lddx) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= rows) return;
    const float g = dloss[0] / fmaxf(result[1], 1.f);
    const float* xr = x + (size_t)i * ldx;
    f32x4 xi[NV], acc[NV];
    load_row(xi, xr, lane, D);
    zero_acc(acc);
    add_own(acc, xi, i, x, ldx, rows, idx_p, idx_n, d_ap, d_an, g, margin, lane, D);            // i as an active anchor: its own two terms
    add_chosen_by(acc, xi, i, x, ldx, rows, idx_p, idx_n, d_ap, d_an, g, margin, lane, D);      // anchors that chose i, in ascending order
    store_row(dx + (size_t)i * lddx, acc, lane, D);
}

int triplet_check_shape(const char* who, int32_t rows, int32_t D, int32_t ld, const char* ld_name) {
    if (int rc = check_d(who, D)) return rc;
    REID_CHECK_ARG(rows >= 1 && rows <= MAX_ROWS, "%s: rows=%d (1..8192)", who, rows);      // (its own: the message says "rows")
    return check_ld(who, rows, D, ld, ld_name);
}

}  // namespace

extern "C" int reid_triplet_hard_fwd(const float* x, int32_t ldx, const int64_t* labels, const uint8_t* valid, int32_t rows, int32_t D,
                                     float margin, float* d_ap, float* d_an, int32_t* idx_p, int32_t* idx_n, float* row_loss,
                                     float* result, void* stream) {
    REID_CHECK_ARG(x && labels && d_ap && d_an && idx_p && idx_n && row_loss && result, "reid_triplet_hard_fwd: null pointer");
    if (int rc = triplet_check_shape("reid_triplet_hard_fwd", rows, D, ldx, "ldx")) return rc;
    REID_CHECK_ARG(aligned16(x), "reid_triplet_hard_fwd: x is not 16-byte aligned");
    REID_CHECK_ARG(margin == margin, "reid_triplet_hard_fwd: margin is NaN");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(triplet_fwd_kernel, dim3((rows + TA - 1) / TA), dim3(256), 0, s, x, ldx, labels, valid, rows, D, margin, d_ap, d_an,
                       idx_p, idx_n, row_loss);
    REID_CHECK_LAUNCH("reid_triplet_hard_fwd(mine)");
    hipLaunchKernelGGL(triplet_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, idx_p, rows, result);
    REID_CHECK_LAUNCH("reid_triplet_hard_fwd(finalize)");
    return REID_OK;
}

extern "C" int reid_triplet_hard_bwd(const float* x, int32_t ldx, int32_t rows, int32_t D, float margin, const float* d_ap,
                                     const float* d_an, const int32_t* idx_p, const int32_t* idx_n, const float* result,
                                     const float* dloss, float* dx, int32_t lddx, void* stream) {
    REID_CHECK_ARG(x && d_ap && d_an && idx_p && idx_n && result && dloss && dx, "reid_triplet_hard_bwd: null pointer");
    if (int rc = triplet_check_shape("reid_triplet_hard_bwd", rows, D, ldx, "ldx")) return rc;
    if (int rc = triplet_check_shape("reid_triplet_hard_bwd", rows, D, lddx, "lddx")) return rc;
    REID_CHECK_ARG(aligned16(x) && aligned16(dx), "reid_triplet_hard_bwd: x or dx is not 16-byte aligned");
    REID_CHECK_ARG(margin == margin, "reid_triplet_hard_bwd: margin is NaN");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((rows + 3) / 4), block(256);
    hipLaunchKernelGGL(triplet_bwd_kernel, grid, block, 0, s, x, ldx, rows, D, margin, d_ap, d_an, idx_p, idx_n, result, dloss, dx, lddx);
    REID_CHECK_LAUNCH("reid_triplet_hard_bwd");
    return REID_OK;
}
