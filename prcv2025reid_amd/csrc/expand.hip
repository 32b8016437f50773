// Query expansion / database-side augmentation for gfx950: out[i] = normalise(x[i] + sum_t w_t table[nbr[i, t]]) over the first k
// eligible entries of row i's ranked list (definition: include/reid_hip.h, reid_expand_rows).  One 64-lane wavefront owns one output
// row; the list is evaluated by its first kl lanes, the rows it names are gathered 16 bytes per lane, UNROLL rows in flight, and
// added in list order.  The kernel is bound by those gathers (k + 2 rows of D floats move per output row against 2 k D flops).
#include "common.h"

// The definition adds w * table[nbr] as a product and a separate sum so that a float32 loop on the host reproduces the bits: no
// fused multiply-adds in this file.
#pragma clang fp contract(off)

namespace {

constexpr int MAXV = 4;     // float4 vectors per lane: D <= 64*4*4 = 1024 (reid_l2norm_rows' limit)
constexpr int UNROLL = 4;   // neighbour rows whose loads are issued before the first dependent add

__device__ __forceinline__ int lane_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float lane_bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// VN: float4 vectors per lane that this instantiation touches (1: D <= 256, 2: D <= 512, 4: D <= 1024)
template <int VN>
__global__ __launch_bounds__(256) void expand_rows_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ table, int64_t ldt,
                                                          int M, const int32_t* __restrict__ nbr, const float* __restrict__ score, int ldn,
                                                          int kl, int k, int alpha, int64_t self_base, int normalize, float eps,
                                                          float* __restrict__ out, int64_t ldo, int rows, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nv = D >> 2;

    // lane t < kl: entry t of the list -- eligibility and weight
    int nb = -1;
    float w = 0.f;
    bool elig = false;
    if (lane < kl) {
        nb = nbr[(size_t)row * ldn + lane];
        const float s = score[(size_t)row * ldn + lane];
        elig = nb >= 0 && nb < M && s == s && !(self_base >= 0 && (int64_t)nb == self_base + row);
        if (alpha == 0) {
            w = 1.f;
        } else {
            const float p = fmaxf(s, 0.f);
            w = p;
            for (int a = 1; a < alpha; ++a) w = w * p;
        }
    }
    // the first k eligible entries are used (their rank among the eligible ones: ballot + prefix count); of those, the ones with a
    // non-zero weight are added.  The mask keeps list order: its set bits are walked from the lowest.
    const uint64_t em = __ballot(elig);
    const int before = __popcll(em & ((1ull << lane) - 1ull));
    uint64_t m = __ballot(elig && before < k && w != 0.f);

    f32x4 acc[VN];
    const float* xr = x + (size_t)row * ldx;
#pragma unroll
    for (int i = 0; i < VN; ++i) {
        const int c = lane + i * 64;
        acc[i] = c < nv ? *(const f32x4*)(xr + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }

    while (__popcll(m) >= UNROLL) {
        f32x4 r[UNROLL][VN];
        float wu[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int t = __builtin_ctzll(m);
            m &= m - 1;
            const float* tr = table + (size_t)lane_bcast(nb, t) * ldt;       // wave-uniform row, 64-bit offset
            wu[u] = lane_bcast(w, t);
#pragma unroll
            for (int i = 0; i < VN; ++i) {
                const int c = lane + i * 64;
                r[u][i] = c < nv ? *(const f32x4*)(tr + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int i = 0; i < VN; ++i) acc[i] = acc[i] + wu[u] * r[u][i];
    }
    while (m) {
        const int t = __builtin_ctzll(m);
        m &= m - 1;
        const float* tr = table + (size_t)lane_bcast(nb, t) * ldt;
        const float wt = lane_bcast(w, t);
        f32x4 r[VN];
#pragma unroll
        for (int i = 0; i < VN; ++i) {
            const int c = lane + i * 64;
            r[i] = c < nv ? *(const f32x4*)(tr + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < VN; ++i) acc[i] = acc[i] + wt * r[i];
    }

    float inv = 1.f;
    if (normalize) {          // l2norm_kernel's shape: per-lane partial sums, wave_sum, sqrtf, one division, one product
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VN; ++i) s += acc[i][0] * acc[i][0] + acc[i][1] * acc[i][1] + acc[i][2] * acc[i][2] + acc[i][3] * acc[i][3];
        inv = 1.f / fmaxf(sqrtf(wave_sum(s)), eps);
    }
    float* orow = out + (size_t)row * ldo;
#pragma unroll
    for (int i = 0; i < VN; ++i) {
        const int c = lane + i * 64;
        if (c < nv) *(f32x4*)(orow + c * 4) = normalize ? acc[i] * inv : acc[i];
    }
}

}  // namespace

extern "C" int reid_expand_rows(const float* x, int64_t ldx, const float* table, int64_t ldt, int32_t M, const int32_t* nbr,
                                const float* score, int32_t ldn, int32_t kl, int32_t k, int32_t alpha, int64_t self_base,
                                int32_t normalize, float eps, float* out, int64_t ldo, int32_t rows, int32_t D, void* stream) {
    REID_CHECK_ARG(x && table && nbr && score && out, "reid_expand_rows: null pointer");
    REID_CHECK_ARG(rows >= 1 && M >= 1, "reid_expand_rows: rows=%d M=%d (both >= 1)", rows, M);
    REID_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 64 * 4 * MAXV, "reid_expand_rows: D=%d unsupported (a multiple of 4, <= %d)", D, 64 * 4 * MAXV);
    REID_CHECK_ARG(kl >= 1 && kl <= REID_EXPAND_MAX_LIST, "reid_expand_rows: kl=%d outside 1..%d", kl, REID_EXPAND_MAX_LIST);
    REID_CHECK_ARG(k >= 1 && k <= kl, "reid_expand_rows: k=%d outside 1..kl=%d", k, kl);
    REID_CHECK_ARG(ldn >= kl, "reid_expand_rows: ldn=%d < kl=%d", ldn, kl);
    REID_CHECK_ARG(alpha >= 0 && alpha <= REID_EXPAND_MAX_ALPHA, "reid_expand_rows: alpha=%d outside 0..%d", alpha, REID_EXPAND_MAX_ALPHA);
    REID_CHECK_ARG(self_base >= -1, "reid_expand_rows: self_base=%lld (-1 = none)", (long long)self_base);
    REID_CHECK_ARG(normalize == 0 || normalize == 1, "reid_expand_rows: normalize=%d (0 or 1)", normalize);
    REID_CHECK_ARG(eps >= 0.f, "reid_expand_rows: eps=%g (>= 0)", (double)eps);
    REID_CHECK_ARG(ldx % 4 == 0 && ldt % 4 == 0 && ldo % 4 == 0 && ldx >= D && ldt >= D && ldo >= D,
                   "reid_expand_rows: ldx=%lld ldt=%lld ldo=%lld (multiples of 4, >= D=%d)", (long long)ldx, (long long)ldt, (long long)ldo, D);
    REID_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0,
                   "reid_expand_rows: x, table and out must be 16-byte aligned");
    REID_CHECK_ARG(out != table && out != x, "reid_expand_rows: out must not be table or x (rows are read while others are written)");
    const dim3 g((rows + 3) / 4), b(256);
    hipStream_t s = (hipStream_t)stream;
#define REID_EXPAND(VN)                                                                                                          \
    hipLaunchKernelGGL(expand_rows_kernel<VN>, g, b, 0, s, x, ldx, table, ldt, M, nbr, score, ldn, kl, k, alpha, self_base, normalize, \
                       eps, out, ldo, rows, D)
    if (D <= 256) REID_EXPAND(1);
    else if (D <= 512) REID_EXPAND(2);
    else REID_EXPAND(4);
#undef REID_EXPAND
    REID_CHECK_LAUNCH("reid_expand_rows");
    return REID_OK;
}
