// Cutoff metrics of RANKED LISTS on the device (contract: include/reid_hip.h, reid_list_metrics): the per-query quantities of mAP@K /
// CMC@K (reference: compute_map / compute_cmc, train.py:101-138) from the first k gallery rows of a ranking -- what
// ProtocolEvaluator.ranked_lists, GalleryIndex.topk or a submission file hold -- instead of from score rows (metrics.hip).
//
// One wave per query, four queries per workgroup, no LDS and no barrier:
//   1. npos: the query's CSR row is counted under the same-image exclusion (step 1 of rank_metrics_kernel without the sort);
//   2. the list is walked in chunks of 64 positions, one per lane.  A ballot of the live lanes (a gallery row that is not excluded)
//      gives every lane its position among the live entries by a popcount below its own bit, a ballot of the hits (live and of the
//      query's pid) gives the hit's ordinal the same way; two carries (live entries, hits so far) run across the chunks;
//   3. per cutoff, the hit terms ordinal / position of the chunk are summed by xor shuffles in one fixed order and the chunk sums are
//      added in chunk order, all in fp64: two runs give the same bits.
// A malformed list (see the header) zeroes the query's outputs and sets its status word; indices are range-checked before g_pid / g_img
// are read.
#include "rank.h"

namespace {

using namespace ranking;

constexpr int MAX_CUT = REID_METRICS_MAX_CUTOFFS;
constexpr int WAVES = 4;           // queries per workgroup

struct ListParams {
    const int32_t* idx;                          // [nq, k]
    const int32_t* g_pid; const int32_t* g_img;  // [Ng]; g_img may be null
    const int32_t* q_pid; const int32_t* q_slot; // [nq]
    const int32_t* q_excl;                       // [nq, 4]; may be null
    const int32_t* csr_off; const int32_t* csr_idx;
    int32_t* npos; int32_t* rank1; int32_t* hits; double* sum_at; int32_t* status;
    int nq, k, Ng, n_cut;
    int cut[MAX_CUT];
};

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64 * WAVES) void list_metrics_kernel(const ListParams p) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= p.nq) return;                                      // whole waves leave; nothing below synchronises across waves
    const Excluded4 excluded(p.q_excl, p.g_img, q);
    const int slot = p.q_slot[q];
    int np = 0;
    if (slot >= 0) {
        const int b = p.csr_off[slot], e = p.csr_off[slot + 1];
        for (int t = b + lane; t < e; t += 64) np += excluded(p.csr_idx[t]) ? 0 : 1;
    }
    np = wave_sum_i32(np);
    const int pid = p.q_pid[q];
    const int32_t* row = p.idx + (long long)q * p.k;
    const unsigned long long below = (1ull << lane) - 1ull;     // the lanes before this one
    int live_before = 0, hits_before = 0, rank1 = 0, err = 0;
    bool ended = false;                                         // a -1 has been seen: only -1 may follow
    int hit_at[MAX_CUT] = {};
    double sum_at[MAX_CUT] = {};
    for (int base = 0; base < p.k; base += 64) {
        const int pos = base + lane;
        const bool in_list = pos < p.k;
        const int j = in_list ? row[pos] : -1;
        const bool entry = j >= 0 && j < p.Ng;                  // only these index g_pid / g_img
        const unsigned long long end_m = __ballot(in_list && j == -1);
        const unsigned long long entry_m = __ballot(entry);
        if (__ballot(in_list && j < -1)) err |= REID_LIST_BAD_NEGATIVE;
        if (__ballot(in_list && j >= p.Ng)) err |= REID_LIST_BAD_RANGE;
        // an entry behind a -1 of an earlier chunk, or behind the first -1 of this one
        if (entry_m && (ended || (end_m && (entry_m >> __builtin_ctzll(end_m))))) err |= REID_LIST_BAD_ORDER;
        ended = ended || end_m != 0;
        const bool live = entry && !excluded(j);
        const bool hit = live && p.g_pid[j] == pid;
        const unsigned long long live_m = __ballot(live), hit_m = __ballot(hit);
        const int position = live_before + __builtin_popcountll(live_m & below) + 1;       // rank among the entries that count
        const int ordinal = hits_before + __builtin_popcountll(hit_m & below) + 1;
        const double term = hit ? (double)ordinal / (double)position : 0.0;
        if (rank1 == 0 && hit_m) rank1 = live_before + __builtin_popcountll(live_m & ((1ull << __builtin_ctzll(hit_m)) - 1ull)) + 1;
#pragma unroll
        for (int c = 0; c < MAX_CUT; ++c) {
            if (c < p.n_cut) {
                const bool inside = hit && position <= p.cut[c];
                double s = inside ? term : 0.0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                sum_at[c] += s;
                hit_at[c] += __builtin_popcountll(__ballot(inside));
            }
        }
        live_before += __builtin_popcountll(live_m);
        hits_before += __builtin_popcountll(hit_m);
    }
    if (lane == 0) { p.npos[q] = err ? 0 : np; p.rank1[q] = err ? 0 : rank1; p.status[q] = err; }
#pragma unroll
    for (int c = 0; c < MAX_CUT; ++c)
        if (c < p.n_cut && lane == c) {
            p.hits[(long long)q * p.n_cut + c] = err ? 0 : hit_at[c];
            p.sum_at[(long long)q * p.n_cut + c] = err ? 0.0 : sum_at[c];
        }
}

}  // namespace

extern "C" int reid_list_metrics(const int32_t* idx, int32_t nq, int32_t k, const int32_t* g_pid, const int32_t* g_img,
                                 const int32_t* q_pid, const int32_t* q_slot, const int32_t* q_excl, const int32_t* csr_off,
                                 const int32_t* csr_idx, int32_t Ng, const int32_t* cutoffs, int32_t n_cut, int32_t* npos,
                                 int32_t* rank1, int32_t* hits, double* sum_at, int32_t* status, void* stream) {
    REID_CHECK_ARG(idx && g_pid && q_pid && q_slot && csr_off && csr_idx && cutoffs && npos && rank1 && hits && sum_at && status,
                   "reid_list_metrics: null pointer");
    REID_CHECK_ARG(nq >= 1 && Ng >= 1, "reid_list_metrics: nq=%d Ng=%d", nq, Ng);
    REID_CHECK_ARG(k >= 1 && k <= REID_ROWS_TOPK_MAX_K, "reid_list_metrics: k=%d outside 1..%d", k, REID_ROWS_TOPK_MAX_K);
    REID_CHECK_ARG(n_cut >= 1 && n_cut <= MAX_CUT, "reid_list_metrics: n_cut=%d outside 1..%d", n_cut, MAX_CUT);
    ListParams p{idx, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx, npos, rank1, hits, sum_at, status, nq, k, Ng, n_cut, {}};
    for (int c = 0; c < n_cut; ++c) {
        REID_CHECK_ARG(cutoffs[c] >= 1 && (c == 0 || cutoffs[c] > cutoffs[c - 1]),
                       "reid_list_metrics: cutoffs must be >= 1 and strictly ascending (cutoffs[%d]=%d)", c, cutoffs[c]);
        REID_CHECK_ARG(cutoffs[c] <= k, "reid_list_metrics: cutoff %d beyond the list length k=%d", cutoffs[c], k);
        p.cut[c] = cutoffs[c];
    }
    hipLaunchKernelGGL(list_metrics_kernel, dim3((nq + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_list_metrics");
    return REID_OK;
}
