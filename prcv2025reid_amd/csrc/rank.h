// Ranking primitives shared by the top-k and metric kernels (retrieval.hip, select.hip, metrics.hip, rerank.hip).  The ONE definition
// of the tie rule of the evaluation side -- score descending, index ascending: the order of a stable descending sort -- and of the
// small pieces built around it; the kernel files only use them.
#pragma once
#include "common.h"

namespace ranking {

// (a, ia) ranks before (b, ib); K = float (a score) or uint32_t (an order-preserving key, below)
template <typename K>
__device__ __forceinline__ bool ranks_before(K a, int ia, K b, int ib) {
    static_assert(sizeof(K) == 4, "float scores or u32 keys");
    return a > b || (a == b && ia < ib);
}

// Order-preserving u32 key of a float's bits (a larger float has a larger key) and its inverse; no float maps to 0, so 0 stands for
// "nothing yet" / "no candidate" and reads back as -inf.
__device__ __forceinline__ uint32_t key_of_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t key_of(float f) { return key_of_bits(__float_as_uint(f)); }
__device__ __forceinline__ float key_value(uint32_t key) {
    return key == 0 ? -INFINITY : __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// The key of x + 0.0f with every NaN first and equal to each other: -0 == +0, the smallest (-inf) is 0x007fffff.
__device__ __forceinline__ uint32_t order_key(uint32_t b) {
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;      // NaN
    if ((b << 1) == 0) b = 0;                                      // -0 -> +0
    return key_of_bits(b);
}

// The four image ids a query ignores (row `row` of q_excl [nq, 4]; -1 = none): gallery row j is excluded when its image id g_img[j]
// is one of them.  Masking only when both arrays are given.
struct Excluded4 {
    const int32_t* g_img;
    int id[4];
    bool any;                                                       // any id other than -1
    template <typename Row>
    __device__ __forceinline__ Excluded4(const int32_t* q_excl, const int32_t* g_img_, Row row) : g_img(g_img_), id{-1, -1, -1, -1} {
        if (q_excl && g_img) {
#pragma unroll
            for (int u = 0; u < 4; ++u) id[u] = q_excl[row * 4 + u];
        }
        any = (id[0] & id[1] & id[2] & id[3]) != -1;
    }
    template <typename Col>
    __device__ __forceinline__ bool operator()(Col j) const {
        if (!any) return false;
        const int g = g_img[j];
        return g >= 0 && (g == id[0] || g == id[1] || g == id[2] || g == id[3]);
    }
};

// Bitonic sort of n2 (key, index) pairs in LDS, best rank first, by a workgroup of 256 threads; n2 a power of two, the pairs visible to
// all threads on entry (a barrier behind the last write) and on return.
template <typename K>
__device__ __forceinline__ void lds_rank_sort(K* key, int* idx, int n2, int tid) {
    for (int kb = 2; kb <= n2; kb <<= 1)
        for (int j = kb >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n2; t += 256) {
                const int u = t ^ j;
                if (u > t) {
                    const bool up = (t & kb) == 0;                  // ascending position = earlier rank
                    const K ka = key[t], kc = key[u];
                    const int ia = idx[t], ic = idx[u];
                    const bool swap = up ? ranks_before(kc, ic, ka, ia) : ranks_before(ka, ia, kc, ic);
                    if (swap) { key[t] = kc; key[u] = ka; idx[t] = ic; idx[u] = ia; }
                }
            }
            __syncthreads();
        }
}

// Exclusive prefix of v over a workgroup of 256 threads in thread order (ws: one int per wave, free to be rewritten only after the next
// barrier); total: the sum over all threads.
__device__ __forceinline__ int block_excl_scan(int v, int* ws, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < w) base += ws[u];
        total += ws[u];
    }
    return base + inc - v;
}

// The wave's best (score, index) by the rank rule, in every lane.  With pos: a lane whose pos is negative holds no entry.
__device__ __forceinline__ void wave_best(float& s, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64); const int oi = __shfl_xor(i, o, 64);
        if (ranks_before(os, oi, s, i)) { s = os; i = oi; }
    }
}
__device__ __forceinline__ void wave_best(float& s, int& i, int& pos) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64); const int oi = __shfl_xor(i, o, 64); const int op = __shfl_xor(pos, o, 64);
        if (op >= 0 && (pos < 0 || ranks_before(os, oi, s, i))) { s = os; i = oi; pos = op; }
    }
}

// A wave's candidates of one query live in REGISTERS, one entry per lane: appending is two v_cndmask (no LDS, no shuffles).
// When all 64 lanes are taken, the entries are ranked against each other (64 readlane broadcasts), moved to the lane of their
// rank with one ds_permute -- i.e. sorted -- and everything behind rank k is dropped; the k-th entry becomes the bar a row has
// to clear from then on.  Rows that clear the bar get rarer as the scan proceeds (~k ln(rows/k) in total).
struct LaneList { float s; int i; };
constexpr int INVALID_IDX0 = 0x7fffffc0;     // 64 distinct "after everything" keys for unused lanes

// sort the wave's entries best-first across the lanes; entries of lanes >= cnt or with a negative index are void and end up
// last.  Returns the number of real entries.
__device__ __forceinline__ int lanelist_sort(LaneList& e, int cnt, int lane) {
    const bool real = lane < cnt && e.i >= 0;
    const float ms = real ? e.s : -INFINITY;
    const int mi = real ? e.i : INVALID_IDX0 + lane;
    int rank = 0;
#pragma unroll
    for (int m = 0; m < 64; ++m) {
        const float os = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ms), m));
        const int oi = __builtin_amdgcn_readlane(mi, m);
        rank += ranks_before(os, oi, ms, mi) ? 1 : 0;
    }
    e.s = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(rank * 4, __builtin_bit_cast(int, ms)));
    e.i = __builtin_amdgcn_ds_permute(rank * 4, mi);
    return __builtin_popcountll(__ballot(real));
}

// the k best of n entries in LDS (void entries: index < 0), sorted into lanes [0, k) of the calling wave; k <= 32:
// a window of 64 lanes = the best k so far + up to 64 - k new entries per sort
__device__ __forceinline__ int wave_select_lds(const float* sc, const int32_t* ix, int n, int k, int lane, LaneList& e) {
    int have = n < 64 ? n : 64;
    e = lane < have ? LaneList{sc[lane], ix[lane]} : LaneList{-INFINITY, -1};
    int next = have;
    int real = lanelist_sort(e, have, lane);
    while (next < n) {
        const int keep = real < k ? real : k;
        const int take = (n - next) < (64 - keep) ? (n - next) : (64 - keep);
        if (lane >= keep && lane < keep + take) e = LaneList{sc[next + lane - keep], ix[next + lane - keep]};
        next += take;
        real = lanelist_sort(e, keep + take, lane);
    }
    return real < k ? real : k;
}

}  // namespace ranking
