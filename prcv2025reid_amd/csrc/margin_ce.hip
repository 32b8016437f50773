// Cosine-margin identity heads (NormFace / CosFace / ArcFace / Circle) with a fused label-smoothed CE for gfx950: fp32 in and out,
// the products and sums of the logits and their gradients in fp64.  The reference has none: its identity branch is a plain Linear followed by label-smoothed CE.
//
//   rx_b = 1 / max(|x_b|, eps), rw_c = 1 / max(|W_c|, eps), cos_bc = (x_b . W_c) rx_b rw_c, l_bc = s cos_bc   (the logits)
//   z'   = the margin logits of include/reid_hip.h (cosine: l; cosface: l_y - s m; arcface: s phi(clamp(cos_y)); circle: s alpha (cos - delta))
//   row loss = (1 - e)(lse(z') - z'_y) + e (lse(z') - mean_c z'_c), the loss the mean over the used rows (valid != 0 and 0 <= y < C)
//
// Cosine logits, forward (reid_cos_logits_fwd): cos_norms_kernel (one wave per row of x and of W, inverse norms in fp64),
//   cos_logits_kernel (32 x 32 tiles, fp64 products and sums, l = s (x_b . W_c) rx_b rw_c rounded once).
// Cosine logits, backward: cos_bwd_prep_kernel (ONE launch: G = g (rw . W) [B, D] and H = g^T (rx . x) [C, D] in fp64),
//   cos_bwd_fix_kernel (ONE launch: dx_b = s rx_b (G_b - xh_b (xh_b . G_b)), dW_c = s rw_c (H_c - wh_c (wh_c . H_c)); a row below eps
//   has no projection term).  The projections are what dz W - x rx^2 tb is, with tb_b = sum_c g l = s xh_b . G_b taken from G itself.
// Margin CE, forward (reid_margin_ce_fwd): margin_ce_fwd_kernel, one wave per row: the margin transform is recomputed from the logit in
//   every pass, so z' lives in registers only; margin_ce_reduce_kernel, ONE workgroup: the row losses added in a fixed order in fp64.
// Margin CE, backward (reid_margin_ce_bwd): one wave per row, dl = gs (p - e / C - (1 - e)[c == y]) dz'/dl, the target's p_y - 1 taken as
//   -sum_{c != y} p_c; unused rows get zeros.
// No atomics anywhere in this file: two runs give the same bits in every output.  Every row is walked one column per lane (stride
// 64), with 64-bit offsets: no alignment or leading-dimension multiple is asked for, padding columns are neither read nor written.
#include <math.h>
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------- cosine logits
// rows 0 .. B-1: x, rows B .. B+C-1: W -- the same instruction sequence for both, so bit-equal rows get bit-equal inverse norms
__global__ __launch_bounds__(256) void cos_norms_kernel(const float* __restrict__ x, int ldx, int B, const float* __restrict__ W, int ldw,
                                                        int C, int D, float eps, double* __restrict__ rx, double* __restrict__ rw) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= B + C) return;
    const float* row = r < B ? x + (size_t)r * ldx : W + (size_t)(r - B) * ldw;
    double s = 0.0;
    for (int c = lane; c < D; c += 64) { const double v = (double)row[c]; s = fma(v, v, s); }
    s = wave_sum_f64(s);
    if (lane == 0) {
        const double inv = 1.0 / fmax(sqrt(s), (double)eps);
        if (r < B) rx[r] = inv; else rw[r - B] = inv;
    }
}

// One 32 x 32 tile of  acc(m, n) = sum_k A(m, k) ks(k) B(k, n)  with fp64 products and sums (k ascending: a fixed order), by a
// workgroup of 256 threads, each owning 2 x 2 outputs; A and B are fp32 with element strides, ks an optional fp64 factor per k.  The
// dot products of this head cancel (a class centre against an unrelated row; a gradient that is orthogonal to its own row), so an
// fp32 sum loses what the result is made of; the shapes are latency bound, the fp64 rate is not what they wait for.  K steps of 16
// through LDS, the next step's operands travel global -> registers while this one is multiplied.
constexpr int GT = 32, GK = 16, GP = GT + 2;             // tile edge, K step, padded LDS row (doubles)
__device__ __forceinline__ void tile_gemm_f64(const float* __restrict__ A, long sam, long sak, const float* __restrict__ Bm, long sbk, long sbn,
                                              const double* __restrict__ ks, int M, int N, int K, int m0, int n0, double (&acc)[2][2]) {
    __shared__ __attribute__((aligned(16))) double As[GK * GP];
    __shared__ __attribute__((aligned(16))) double Bs[GK * GP];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const bool a_kfast = sak == 1, b_kfast = sbk == 1;
    // element e = tid + 256 i of a 32 x 16 operand tile: the fast thread index follows the contiguous stride
    auto coords = [&](bool kfast, int i, int& xx, int& kk) {
        const int e = tid + 256 * i;
        if (kfast) { kk = e & 15; xx = e >> 4; } else { xx = e & 31; kk = e >> 5; }
    };
    double ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int xx, kk;
            coords(a_kfast, i, xx, kk);
            const int m = m0 + xx, ka = k0 + kk;
            ra[i] = (m < M && ka < K) ? (double)A[(long)m * sam + (long)ka * sak] * (ks ? ks[ka] : 1.0) : 0.0;
            coords(b_kfast, i, xx, kk);
            const int n = n0 + xx, kb = k0 + kk;
            rb[i] = (n < N && kb < K) ? (double)Bm[(long)kb * sbk + (long)n * sbn] : 0.0;
        }
    };
    acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = 0.0;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();                                 // the previous step has been read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int xx, kk;
            coords(a_kfast, i, xx, kk);
            As[kk * GP + xx] = ra[i];
            coords(b_kfast, i, xx, kk);
            Bs[kk * GP + xx] = rb[i];
        }
        __syncthreads();
        if (k0 + GK < K) fetch(k0 + GK);
#pragma unroll
        for (int kk = 0; kk < GK; ++kk) {
            const double a0 = As[kk * GP + 2 * ty], a1 = As[kk * GP + 2 * ty + 1];
            const double b0 = Bs[kk * GP + 2 * tx], b1 = Bs[kk * GP + 2 * tx + 1];
            acc[0][0] = fma(a0, b0, acc[0][0]); acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]); acc[1][1] = fma(a1, b1, acc[1][1]);
        }
    }
}

// l_bc = s (x_b . W_c) rx_b rw_c, everything in fp64 up to the one rounding of the result
__global__ __launch_bounds__(256) void cos_logits_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ W, int ldw, int B, int C,
                                                         int D, float s, const double* __restrict__ rx, const double* __restrict__ rw,
                                                         float* __restrict__ l, int ldl) {
    const int ntn = (C + GT - 1) / GT;
    const int m0 = (blockIdx.x / ntn) * GT, n0 = (blockIdx.x % ntn) * GT;
    double acc[2][2];
    tile_gemm_f64(x, ldx, 1, W, 1, ldw, nullptr, B, C, D, m0, n0, acc);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int b = m0 + 2 * ty + i, c = n0 + 2 * tx + j;
            if (b < B && c < C) l[(size_t)b * ldl + c] = (float)((double)s * acc[i][j] * rx[b] * rw[c]);
        }
}

// workgroups [0, ng): tiles of G [B, D] = g (rw . W), G_b = sum_c g_bc rw_c W_c; workgroups [ng, ..): tiles of H [C, D] = g^T (rx . x),
// H_c = sum_b g_bc rx_b x_b; both kept in fp64 for cos_bwd_fix_kernel
__global__ __launch_bounds__(256) void cos_bwd_prep_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ x, int ldx,
                                                           const float* __restrict__ W, int ldw, const double* __restrict__ rx,
                                                           const double* __restrict__ rw, int B, int C, int D, double* __restrict__ G,
                                                           double* __restrict__ H, int ng) {
    const int ntn = (D + GT - 1) / GT;
    const bool isg = (int)blockIdx.x < ng;
    const int t = isg ? blockIdx.x : blockIdx.x - ng;
    const int m0 = (t / ntn) * GT, n0 = (t % ntn) * GT;
    double acc[2][2];
    if (isg) tile_gemm_f64(g, ldg, 1, W, ldw, 1, rw, B, D, C, m0, n0, acc);
    else tile_gemm_f64(g, 1, ldg, x, ldx, 1, rx, C, D, B, m0, n0, acc);
    double* out = isg ? G : H;
    const int M = isg ? B : C;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + 2 * ty + i, n = n0 + 2 * tx + j;
            if (m < M && n < D) out[(size_t)m * D + n] = acc[i][j];
        }
}

// rows 0 .. B-1 (when dx): dx_b = s rx_b (G_b - xh_b (xh_b . G_b)), xh_b = x_b rx_b; rows B .. B+C-1 (when dW): dW_c = s rw_c (H_c -
// wh_c (wh_c . H_c)).  sum_c g_bc cos_bc = xh_b . G_b, so the projection needs no logits; fp64 up to the one rounding of the result.
// A row whose norm is not above eps (inv = 1 / eps) was divided by the constant eps: no projection term.
__global__ __launch_bounds__(256) void cos_bwd_fix_kernel(const float* __restrict__ x, int ldx, const double* __restrict__ rx,
                                                          const double* __restrict__ G, float* __restrict__ dx, int lddx,
                                                          const float* __restrict__ W, int ldw, const double* __restrict__ rw,
                                                          const double* __restrict__ H, float* __restrict__ dW, int lddw, int B, int C, int D,
                                                          float s, float eps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= B + C) return;
    const bool isx = r < B;
    if (isx ? !dx : !dW) return;
    const int i = isx ? r : r - B;
    const float* src = isx ? x + (size_t)i * ldx : W + (size_t)i * ldw;
    const double* acc = (isx ? G : H) + (size_t)i * D;
    float* dst = isx ? dx + (size_t)i * lddx : dW + (size_t)i * lddw;
    const double inv = isx ? rx[i] : rw[i];
    double dot = 0.0;
    if (inv < 1.0 / (double)eps) {
        for (int c = lane; c < D; c += 64) dot = fma((double)src[c] * inv, acc[c], dot);
        dot = wave_sum_f64(dot);
    }
    const double k = (double)s * inv;
    for (int c = lane; c < D; c += 64) dst[c] = (float)(k * (acc[c] - ((double)src[c] * inv) * dot));
}

// ---------------------------------------------------------------------------------------------- margin CE
struct Margin {
    int kind;
    float s, m;
    float cos_m, sin_m, thr, mm;         // arcface: cos(m), sin(m), cos(pi - m), m sin(pi - m), rounded once from fp64
};

constexpr float ARC_LO = -1.f + 1.1920928955078125e-07f, ARC_HI = 1.f - 1.1920928955078125e-07f;      // +-(1 - 2^-23)

// z' of one class from its logit l, and dz'/dl
template <bool WITH_D>
__device__ __forceinline__ float margin_z(const Margin& M, float l, bool target, float& dz) {
    dz = 1.f;
    if (M.kind == REID_MARGIN_COSINE) return l;
    if (M.kind == REID_MARGIN_COSFACE) return target ? l - M.s * M.m : l;
    const float cs = l / M.s;
    if (M.kind == REID_MARGIN_ARCFACE) {
        if (!target) return l;
        const float t = fminf(fmaxf(cs, ARC_LO), ARC_HI);
        float phi;
        if (t > M.thr) {
            const float sq = sqrtf(1.f - t * t);
            phi = t * M.cos_m - sq * M.sin_m;
            if (WITH_D) dz = M.cos_m + t * M.sin_m / sq;
        } else {
            phi = t - M.mm;
        }
        if (WITH_D && !(cs >= ARC_LO && cs <= ARC_HI)) dz = 0.f;                                       // the clamp acted (torch.clamp)
        return M.s * phi;
    }
    // circle: alpha_p = max(1 + m - cos_y, 0), alpha_n = max(cos_c + m, 0) are constants of the gradient
    const float a = target ? fmaxf(1.f + M.m - cs, 0.f) : fmaxf(cs + M.m, 0.f);
    dz = a;
    return M.s * a * (cs - (target ? 1.f - M.m : M.m));
}

// max, sum of exponentials, sum and target value of z' of one row, by one wave.  The exponentials are summed without the target's
// (se_o) and its own is kept beside them (ey), se = se_o + ey: the backward takes p_y - 1 = -se_o / se from them, which keeps its
// relative accuracy where p_y rounds to 1 (a target far ahead of the other classes is what a margin head trains towards).
__device__ __forceinline__ void margin_row_stats(const Margin& M, const float* __restrict__ l, int C, int y, int lane, float& mx, float& se_o,
                                                 float& ey, float& sz, float& zy) {
    mx = -INFINITY; sz = 0.f; zy = 0.f;
    float d;
    for (int c = lane; c < C; c += 64) {
        const float z = margin_z<false>(M, l[c], c == y, d);
        mx = fmaxf(mx, z); sz += z;
        if (c == y) zy = z;
    }
    mx = wave_max(mx); sz = wave_sum(sz); zy = wave_sum(zy);         // (zy: one lane holds it, the others 0)
    se_o = 0.f;
    for (int c = lane; c < C; c += 64)
        if (c != y) se_o += expf(margin_z<false>(M, l[c], false, d) - mx);
    se_o = wave_sum(se_o);
    ey = expf(zy - mx);
}

__device__ __forceinline__ bool row_used(const int64_t* __restrict__ labels, const uint8_t* __restrict__ valid, int row, int C) {
    const int64_t y = labels[row];
    return (!valid || valid[row]) && y >= 0 && y < C;
}

__global__ __launch_bounds__(256) void margin_ce_fwd_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ labels,
                                                            const uint8_t* __restrict__ valid, int rows, int C, Margin M, float e,
                                                            float* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= rows) return;
    float loss = 0.f;
    if (row_used(labels, valid, row, C)) {
        float mx, se_o, ey, sz, zy;
        margin_row_stats(M, logits + (size_t)row * ld, C, (int)labels[row], lane, mx, se_o, ey, sz, zy);
        const float lse = mx + logf(se_o + ey);
        loss = (1.f - e) * (lse - zy) + e * (lse - sz / (float)C);
    }
    if (lane == 0) row_loss[row] = loss;
}

// one workgroup: thread t adds rows t, t + 256, ... in fp64, the 256 sums are added in index order (triplet_finalize_kernel's tail)
__global__ __launch_bounds__(256) void margin_ce_reduce_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ labels,
                                                               const uint8_t* __restrict__ valid, int rows, int C, float* __restrict__ result) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    int n = 0;
    for (int r = tid; r < rows; r += 256)
        if (row_used(labels, valid, r, C)) { s += (double)row_loss[r]; ++n; }
    s_sum[tid] = s; s_cnt[tid] = n;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        int c = 0;
        for (int u = 0; u < 256; ++u) { t += s_sum[u]; c += s_cnt[u]; }
        result[0] = (float)t;
        result[1] = (float)c;
        result[2] = (float)(t / (double)(c > 0 ? c : 1));
    }
}

__global__ __launch_bounds__(256) void margin_ce_bwd_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ labels,
                                                            const uint8_t* __restrict__ valid, int rows, int C, Margin M, float e,
                                                            const float* __restrict__ result, const float* __restrict__ dloss,
                                                            float* __restrict__ dl, int lddl) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= rows) return;
    float* d = dl + (size_t)row * lddl;
    if (!row_used(labels, valid, row, C)) {
        for (int c = lane; c < C; c += 64) d[c] = 0.f;
        return;
    }
    const float* l = logits + (size_t)row * ld;
    const int y = (int)labels[row];
    float mx, se_o, ey, sz, zy;
    margin_row_stats(M, l, C, y, lane, mx, se_o, ey, sz, zy);
    const float gs = dloss[0] / fmaxf(result[1], 1.f), inv = 1.f / (se_o + ey), sm = e / (float)C;
    for (int c = lane; c < C; c += 64) {
        float dz;
        const float z = margin_z<true>(M, l[c], c == y, dz);
        // p_c - e / C off the target; on it p_y - e / C - (1 - e) = (e - e / C) - sum_{c != y} p_c
        const float t = c == y ? (e - sm) - se_o * inv : expf(z - mx) * inv - sm;
        d[c] = gs * t * dz;
    }
}

int margin_of(const char* who, int32_t kind, float scale, float margin, float smoothing, Margin& M) {
    REID_CHECK_ARG(kind >= REID_MARGIN_COSINE && kind <= REID_MARGIN_CIRCLE, "%s: kind=%d (0 cosine, 1 cosface, 2 arcface, 3 circle)", who, kind);
    REID_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, "%s: scale=%g (> 0, finite)", who, (double)scale);
    REID_CHECK_ARG(smoothing >= 0.f && smoothing <= 1.f, "%s: smoothing=%g (0..1)", who, (double)smoothing);
    if (kind == REID_MARGIN_COSINE) margin = 0.f;                  // ignored
    const double lim = kind == REID_MARGIN_ARCFACE ? 1.5707963267948966 : 1.0;
    REID_CHECK_ARG(margin >= 0.f && (double)margin < lim, "%s: margin=%g (0 <= margin < %s)", who, (double)margin,
                   kind == REID_MARGIN_ARCFACE ? "pi/2 for arcface" : "1 for cosface and circle");
    const double m = (double)margin, pi = 3.14159265358979323846;
    M.kind = kind; M.s = scale; M.m = margin;
    M.cos_m = (float)cos(m); M.sin_m = (float)sin(m); M.thr = (float)cos(pi - m); M.mm = (float)(m * sin(pi - m));
    return REID_OK;
}

int check_matrix(const char* who, const char* name, int64_t rows, int32_t cols, int32_t ld) {
    REID_CHECK_ARG(ld >= cols, "%s: %s=%d (>= %d columns)", who, name, ld, cols);
    REID_CHECK_ARG(rows * (int64_t)ld < (1ll << 40), "%s: rows * %s beyond 2^40 elements", who, name);
    return REID_OK;
}

constexpr int MAX_DIM = 1 << 24;         // rows, classes, columns: the grids and the int arithmetic of the kernels stay far inside int32

}  // namespace

extern "C" int reid_cos_logits_fwd(const float* x, int32_t ldx, const float* W, int32_t ldw, int32_t B, int32_t C, int32_t D, float scale,
                                   float eps, double* rx, double* rw, float* logits, int32_t ldl, void* stream) {
    const char* who = "reid_cos_logits_fwd";
    REID_CHECK_ARG(x && W && rx && rw && logits, "%s: null pointer", who);
    REID_CHECK_ARG(B >= 1 && C >= 1 && D >= 1 && B <= MAX_DIM && C <= MAX_DIM && D <= MAX_DIM, "%s: B=%d C=%d D=%d (1..2^24)", who, B, C, D);
    if (int rc = check_matrix(who, "ldx", B, D, ldx)) return rc;
    if (int rc = check_matrix(who, "ldw", C, D, ldw)) return rc;
    if (int rc = check_matrix(who, "ldl", B, C, ldl)) return rc;
    REID_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, "%s: scale=%g (> 0, finite)", who, (double)scale);
    REID_CHECK_ARG(eps >= 0.f, "%s: eps=%g (>= 0)", who, (double)eps);
    const int64_t tiles = (int64_t)((B + GT - 1) / GT) * ((C + GT - 1) / GT);
    REID_CHECK_ARG(tiles < (1ll << 31), "%s: B=%d x C=%d beyond 2^31 tiles", who, B, C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cos_norms_kernel, dim3((B + C + 3) / 4), dim3(256), 0, s, x, ldx, B, W, ldw, C, D, eps, rx, rw);
    REID_CHECK_LAUNCH("reid_cos_logits_fwd(norms)");
    hipLaunchKernelGGL(cos_logits_kernel, dim3((unsigned)tiles), dim3(256), 0, s, x, ldx, W, ldw, B, C, D, scale, rx, rw, logits, ldl);
    REID_CHECK_LAUNCH("reid_cos_logits_fwd(logits)");
    return REID_OK;
}

extern "C" int reid_cos_logits_bwd_prep(const float* g, int32_t ldg, const float* x, int32_t ldx, const float* W, int32_t ldw,
                                        const double* rx, const double* rw, int32_t B, int32_t C, int32_t D, double* G, double* H,
                                        void* stream) {
    const char* who = "reid_cos_logits_bwd_prep";
    REID_CHECK_ARG(g && (G || H), "%s: null pointer", who);
    REID_CHECK_ARG(!G || (W && rw), "%s: G needs W and rw", who);
    REID_CHECK_ARG(!H || (x && rx), "%s: H needs x and rx", who);
    REID_CHECK_ARG(B >= 1 && C >= 1 && D >= 1 && B <= MAX_DIM && C <= MAX_DIM && D <= MAX_DIM, "%s: B=%d C=%d D=%d (1..2^24)", who, B, C, D);
    if (int rc = check_matrix(who, "ldg", B, C, ldg)) return rc;
    if (G) { if (int rc = check_matrix(who, "ldw", C, D, ldw)) return rc; }
    if (H) { if (int rc = check_matrix(who, "ldx", B, D, ldx)) return rc; }
    const int64_t ntn = (D + GT - 1) / GT;
    const int64_t ng = G ? ((B + GT - 1) / GT) * ntn : 0, nh = H ? ((C + GT - 1) / GT) * ntn : 0;
    REID_CHECK_ARG(ng + nh < (1ll << 31), "%s: (B=%d + C=%d) x D=%d beyond 2^31 tiles", who, B, C, D);
    hipLaunchKernelGGL(cos_bwd_prep_kernel, dim3((unsigned)(ng + nh)), dim3(256), 0, (hipStream_t)stream, g, ldg, x, ldx, W, ldw, rx, rw, B, C,
                       D, G, H, (int)ng);
    REID_CHECK_LAUNCH(who);
    return REID_OK;
}

extern "C" int reid_cos_logits_bwd_fix(const float* x, int32_t ldx, const double* rx, const double* G, float* dx, int32_t lddx,
                                       const float* W, int32_t ldw, const double* rw, const double* H, float* dW, int32_t lddw, int32_t B,
                                       int32_t C, int32_t D, float scale, float eps, void* stream) {
    const char* who = "reid_cos_logits_bwd_fix";
    REID_CHECK_ARG(dx || dW, "%s: neither dx nor dW", who);
    REID_CHECK_ARG(!dx || (x && rx && G), "%s: dx needs x, rx and G", who);
    REID_CHECK_ARG(!dW || (W && rw && H), "%s: dW needs W, rw and H", who);
    REID_CHECK_ARG(B >= 1 && C >= 1 && D >= 1 && B <= MAX_DIM && C <= MAX_DIM && D <= MAX_DIM, "%s: B=%d C=%d D=%d (1..2^24)", who, B, C, D);
    if (dx) {
        if (int rc = check_matrix(who, "ldx", B, D, ldx)) return rc;
        if (int rc = check_matrix(who, "lddx", B, D, lddx)) return rc;
    }
    if (dW) {
        if (int rc = check_matrix(who, "ldw", C, D, ldw)) return rc;
        if (int rc = check_matrix(who, "lddw", C, D, lddw)) return rc;
    }
    REID_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, "%s: scale=%g (> 0, finite)", who, (double)scale);
    REID_CHECK_ARG(eps >= 0.f, "%s: eps=%g (>= 0)", who, (double)eps);
    hipLaunchKernelGGL(cos_bwd_fix_kernel, dim3((B + C + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, rx, G, dx, lddx, W, ldw, rw, H,
                       dW, lddw, B, C, D, scale, eps);
    REID_CHECK_LAUNCH(who);
    return REID_OK;
}

extern "C" int reid_margin_ce_fwd(const float* logits, int32_t ld, const int64_t* labels, const uint8_t* valid, int32_t rows, int32_t C,
                                  int32_t kind, float scale, float margin, float smoothing, float* row_loss, float* result, void* stream) {
    const char* who = "reid_margin_ce_fwd";
    REID_CHECK_ARG(logits && labels && row_loss && result, "%s: null pointer", who);
    REID_CHECK_ARG(rows >= 1 && C >= 1 && rows <= MAX_DIM && C <= MAX_DIM, "%s: rows=%d C=%d (1..2^24)", who, rows, C);
    if (int rc = check_matrix(who, "ld", rows, C, ld)) return rc;
    Margin M;
    if (int rc = margin_of(who, kind, scale, margin, smoothing, M)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(margin_ce_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, ld, labels, valid, rows, C, M, smoothing, row_loss);
    REID_CHECK_LAUNCH("reid_margin_ce_fwd(rows)");
    hipLaunchKernelGGL(margin_ce_reduce_kernel, dim3(1), dim3(256), 0, s, row_loss, labels, valid, rows, C, result);
    REID_CHECK_LAUNCH("reid_margin_ce_fwd(reduce)");
    return REID_OK;
}

extern "C" int reid_margin_ce_bwd(const float* logits, int32_t ld, const int64_t* labels, const uint8_t* valid, int32_t rows, int32_t C,
                                  int32_t kind, float scale, float margin, float smoothing, const float* result, const float* dloss,
                                  float* dlogits, int32_t lddl, void* stream) {
    const char* who = "reid_margin_ce_bwd";
    REID_CHECK_ARG(logits && labels && result && dloss && dlogits, "%s: null pointer", who);
    REID_CHECK_ARG(rows >= 1 && C >= 1 && rows <= MAX_DIM && C <= MAX_DIM, "%s: rows=%d C=%d (1..2^24)", who, rows, C);
    if (int rc = check_matrix(who, "ld", rows, C, ld)) return rc;
    if (int rc = check_matrix(who, "lddl", rows, C, lddl)) return rc;
    Margin M;
    if (int rc = margin_of(who, kind, scale, margin, smoothing, M)) return rc;
    hipLaunchKernelGGL(margin_ce_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, labels, valid, rows, C, M,
                       smoothing, result, dloss, dlogits, lddl);
    REID_CHECK_LAUNCH(who);
    return REID_OK;
}
