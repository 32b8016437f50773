// Exact top-k lists of fp32 score rows on the device (contract: include/reid_hip.h, reid_rows_topk): position r of row q is the
// r-th entry of a stable descending sort of the row's eligible columns, without sorting the row.
//
// Every value maps to an order-preserving u32 key (-0 == +0, every NaN first and equal to each other); an entry ranks before another
// when its key is larger, or equal with the smaller column.  One workgroup owns one row:
//   1. radix select of the k-th key, most significant digit first (12 + 12 + 8 bits): an LDS histogram of the digit over the entries
//      that share the digits found so far, a suffix sum from the top bin down, the bin in which the count crosses k.  `above` counts
//      the entries that beat every key of that bin.  The refinement stops as soon as `above` plus the bin fit the candidate buffer;
//   2. one collecting pass: everything from the bin upward goes into the LDS buffer through an integer slot counter.  Only when all 32
//      key bits are fixed and the entries EQUAL to that key still overflow the buffer (lambda = 0 re-ranking: tens of thousands of
//      exact zeros across the cut) the equal ones are taken by ascending column instead: the row is walked in column order, 1024
//      columns per step, a workgroup prefix sum ranks the step's equal entries, and the first k - above of them are kept;
//   3. a bitonic sort of the buffer (at most 2048 (key, column) pairs) by (key descending, column ascending), then the k outputs.
// The row is read two to four times (16-byte loads); after the first pass it comes from L2 / the Infinity Cache.  Integer LDS atomics
// only: the slot a candidate lands in varies from run to run, the sorted output does not.
#include "rank.h"

namespace {

using namespace ranking;

constexpr int SEL_BINS = 4096;      // histogram bins of one digit (12 bits; the last digit has 8)
constexpr int SEL_CAP = 2048;       // candidate buffer, >= REID_ROWS_TOPK_MAX_K
constexpr int SEL_MAX_K = 1024;

struct SelectParams {
    const float* S; long long ld;               // scores [nq, ld]
    const int32_t* g_img; const int32_t* q_excl;  // [n], [nq, 4]; masking only when both are given
    int32_t* out_idx; uint32_t* out_score;      // [nq, k]
    int n, k;
};

__global__ __launch_bounds__(256) void rows_topk_kernel(const SelectParams p) {
    __shared__ int hist[SEL_BINS];
    __shared__ uint32_t ckey[SEL_CAP];
    __shared__ int cidx[SEL_CAP];
    __shared__ int wsum[2][4];
    __shared__ int sel[3];          // the crossing bin, the entries above it, the entries in it
    __shared__ int ccount;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = p.k;
    const uint32_t n = (uint32_t)p.n, nvec = (n + 3u) >> 2;         // the last 16 bytes may reach into the padding: ld % 4 == 0
    const uint32_t* row = (const uint32_t*)(p.S + (long long)q * p.ld);
    const Excluded4 excluded(p.q_excl, p.g_img, (long long)q);
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
    auto keys4 = [&](uint32_t t, uint32_t kk[4]) {                  // keys of columns 4t .. 4t + 3; 0 = past n or excluded
        const u32x4 v = *(const u32x4*)(row + 4 * (size_t)t);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t j = 4 * t + u;
            kk[u] = (j < n && !excluded(j)) ? order_key(v[u]) : 0u;
        }
    };

    // ---- 1. the k-th key, digit by digit -----------------------------------------------------------------------------------------
    uint32_t prefix = 0, mask = 0;      // the digits fixed so far: candidates of the cut have (key & mask) == prefix
    int above = 0;                      // entries with (key & mask) > prefix: all of them are in the list
    bool ranked = false;                // all 32 bits fixed and the equal entries overflow the buffer
    for (int level = 0; level < 3; ++level) {
        const int shift = level == 0 ? 20 : (level == 1 ? 8 : 0);
        const int nb = level == 2 ? 256 : SEL_BINS;
        for (int b = tid; b < nb; b += 256) hist[b] = 0;
        __syncthreads();
        if (tid == 0) sel[0] = -1;
        for (uint32_t t = tid; t < nvec; t += 256) {
            uint32_t kk[4];
            keys4(t, kk);
            int bin[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                in[u] = kk[u] != 0u && (kk[u] & mask) == prefix;
                bin[u] = (int)((kk[u] >> shift) & (uint32_t)(nb - 1));
            }
            // a wave whose active lanes' entries all fall into one bin (a block of equal values) adds once, not once per entry, to one address
            const int b0 = __builtin_amdgcn_readfirstlane(bin[0]);
            const bool same = in[0] && in[1] && in[2] && in[3] && bin[0] == b0 && bin[1] == b0 && bin[2] == b0 && bin[3] == b0;
            if (__all(same)) {
                const unsigned long long act = __ballot(1);
                if (lane == __ffsll((long long)act) - 1) atomicAdd(&hist[b0], 4 * __popcll(act));
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (in[u]) atomicAdd(&hist[bin[u]], 1);
            }
        }
        __syncthreads();
        // suffix sums from the top bin down: thread t owns bins [t * per, (t + 1) * per)
        const int per = nb >> 8;
        int s = 0;
        for (int u = 0; u < per; ++u) s += hist[tid * per + u];
        int incl = s;                                               // this thread's bins and those of the higher lanes of the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_down(incl, o, 64);
            if (lane + o < 64) incl += v;
        }
        if (lane == 0) wsum[0][wave] = incl;
        __syncthreads();
        int hi = above + incl - s;                                  // entries that beat every key of this thread's bins
        for (int w = wave + 1; w < 4; ++w) hi += wsum[0][w];
        if (hi < k && k <= hi + s) {                                // the count crosses k inside this thread's bins
            int run = hi;
            for (int u = per - 1; u >= 0; --u) {
                const int c = hist[tid * per + u];
                if (k <= run + c) { sel[0] = tid * per + u; sel[1] = run; sel[2] = c; break; }
                run += c;
            }
        }
        __syncthreads();
        const int sb = sel[0];
        if (sb < 0) break;              // fewer than k eligible columns (level 0 only): mask = 0 takes all of them
        above = sel[1];
        prefix |= (uint32_t)sb << shift;
        mask |= (uint32_t)(nb - 1) << shift;
        if (above + sel[2] <= SEL_CAP) break;
        ranked = level == 2;
    }

    // ---- 2. collect ------------------------------------------------------------------------------------------------------------------
    if (tid == 0) ccount = 0;
    __syncthreads();                    // (also: every thread has read sel[] before anything below runs)
    auto take = [&](uint32_t key, uint32_t j) {
        const int o = atomicAdd(&ccount, 1);
        if (o < SEL_CAP) { ckey[o] = key; cidx[o] = (int)j; }
    };
    if (!ranked) {
        for (uint32_t t = tid; t < nvec; t += 256) {
            uint32_t kk[4];
            keys4(t, kk);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (kk[u] != 0u && (kk[u] & mask) >= prefix) take(kk[u], 4 * t + u);
        }
    } else {
        // prefix is the k-th key itself: keys above it are taken as they come, the equal ones by ascending column until `need` are found
        const int need = k - above;
        int found = 0;                  // equal entries in the columns walked so far (the same in every thread)
        uint32_t c0 = 0;
        for (int it = 0; c0 < nvec && found < need; c0 += 256, ++it) {
            const uint32_t t = c0 + tid;
            uint32_t kk[4] = {0u, 0u, 0u, 0u};
            if (t < nvec) keys4(t, kk);
            int mine = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (kk[u] > prefix) take(kk[u], 4 * t + u);
                mine += kk[u] == prefix;
            }
            int total;                  // one barrier per step: the next step writes the other half of wsum
            int rank = found + block_excl_scan(mine, wsum[it & 1], total);   // this step's equal entries of the lower threads
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (kk[u] == prefix) {
                    if (rank < need) take(kk[u], 4 * t + u);
                    ++rank;
                }
            found += total;
        }
        for (uint32_t t = c0 + tid; t < nvec; t += 256) {           // behind the last equal entry that is kept: larger keys only
            uint32_t kk[4];
            keys4(t, kk);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (kk[u] > prefix) take(kk[u], 4 * t + u);
        }
    }
    __syncthreads();

    // ---- 3. order the candidates, write the list -----------------------------------------------------------------------------------------
    const int total = min(ccount, SEL_CAP);
    int n2 = 1;
    while (n2 < total) n2 <<= 1;
    for (int t = total + tid; t < n2; t += 256) { ckey[t] = 0u; cidx[t] = 0x7fffffff; }
    __syncthreads();
    lds_rank_sort(ckey, cidx, n2, tid);
    int32_t* oi = p.out_idx + (long long)q * k;
    uint32_t* os = p.out_score + (long long)q * k;
    for (int r = tid; r < k; r += 256) {
        if (r < total) {
            const int j = cidx[r];
            oi[r] = j;
            os[r] = row[j];                                         // the score's own bits
        } else {
            oi[r] = -1;
            os[r] = 0xff800000u;                                    // -inf
        }
    }
}

}  // namespace

extern "C" int reid_rows_topk(const float* scores, int64_t ld, int32_t nq, int32_t n, int32_t k, const int32_t* g_img,
                              const int32_t* q_excl, int32_t* out_idx, float* out_score, void* stream) {
    REID_CHECK_ARG(scores && out_idx && out_score, "reid_rows_topk: null pointer");
    REID_CHECK_ARG(nq >= 1 && n >= 1 && ld >= n && ld % 4 == 0, "reid_rows_topk: nq=%d n=%d ld=%lld (ld >= n, ld %% 4 == 0)", nq, n,
                   (long long)ld);
    REID_CHECK_ARG(k >= 1 && k <= SEL_MAX_K, "reid_rows_topk: k=%d outside 1..%d", k, SEL_MAX_K);
    REID_CHECK_ARG(((uintptr_t)scores & 15) == 0, "reid_rows_topk: scores must be 16-byte aligned");
    static_assert(SEL_CAP >= SEL_MAX_K && SEL_MAX_K == REID_ROWS_TOPK_MAX_K, "candidate buffer");
    const SelectParams p{scores, (long long)ld, g_img, q_excl, out_idx, (uint32_t*)out_score, n, k};
    hipLaunchKernelGGL(rows_topk_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_rows_topk");
    return REID_OK;
}
