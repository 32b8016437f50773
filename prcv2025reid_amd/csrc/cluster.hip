// DBSCAN over similarity rows on the device (contract: include/reid_hip.h, "DBSCAN"; definition: DESIGN.md §22).  The rows arrive chunk
// by chunk (the s* rows of a pooled re-ranker, or any fp32 similarity rows) and are never kept: each chunk is turned into its slice of
// the eps-neighbour CSR, and everything after that works on the CSR alone.
//
//   reid_dbscan_count     one workgroup per row: |N(i)| by 16-byte loads and a workgroup sum; the core flag beside it.
//   reid_dbscan_fill      one workgroup per row, 1024 columns per step: a workgroup prefix sum of the step's neighbours ranks them, so the
//                         columns land ascending whatever the order the waves run in (a compaction, not an append).
//   reid_dbscan_hook      16 lanes per core row (neighbour lists are tens of entries long; longer ones are walked 16 at a time): for each
//                         directed edge to another core, atomicMin(parent[max(ru, rv)], min(ru, rv)) on the two ends' parents, and one
//                         add to `changed` per wave that saw two different parents.
//   reid_dbscan_compress  one thread per row: chases its own pointer to the root and stores the root.
//   reid_dbscan_border    16 lanes per core row: atomicMin(label[j], root(i)) for every non-core j in N(i).
//
// The components scheme and why it ends.  INVARIANT: parent[x] <= x at all times, and a parent only ever decreases (the hook stores
// min(ru, rv) < max(ru, rv) with atomicMin, the compress pass stores an ancestor, which is <= the old parent).  A chase x -> parent[x] -> ..
// therefore strictly decreases until it meets a fixed point and ends in at most x steps, whatever other threads store meanwhile; a
// load that returns an older value of a parent returns an older ancestor, which is still an ancestor.  Every link joins two rows that
// an edge chain connects, so a tree never leaves its component; the host stops at the first round in which no edge saw two
// different parents: then every component is one tree, and its root is its smallest row since parent[x] <= x.  No kernel waits for
// another workgroup, polls memory or loops on a condition another workgroup must satisfy: the rounds are separate launches and the
// host reads `changed` between them.
//
// Only integer atomicMin / atomicAdd: the values they leave do not depend on the order of arrival, so counts, flags, the CSR and the
// labels are the same bits in every run (the number of rounds may differ by the interleaving inside a hook pass).
#include "rank.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float row4;

struct RowsParams {
    const float* S; long long ld;           // similarity rows [nr, ld]
    long long row0;                         // global index of row 0 of the chunk: its own column always counts
    float thr;
    int n, min_samples;
    int32_t* count; uint8_t* core;          // [nr] (count pass)
    const int64_t* rowptr; int32_t* cols;   // [nr + 1] chunk-local offsets, [cap] (fill pass)
    long long cap;
};

// columns 4t .. 4t + 3 of the row: bit u is set when column 4t + u is a neighbour.  NaN >= thr is false, +inf >= thr is true.
__device__ __forceinline__ int neighbours4(const float* row, uint32_t t, uint32_t n, uint32_t self, float thr) {
    const row4 v = *(const row4*)(row + 4 * (size_t)t);       // the last 16 bytes may reach into the padding: ld % 4 == 0
    int m = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t j = 4 * t + u;
        m |= (j < n && (j == self || v[u] >= thr)) ? 1 << u : 0;
    }
    return m;
}

__global__ __launch_bounds__(256) void dbscan_count_kernel(const RowsParams p) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = blockIdx.x;
    const uint32_t n = (uint32_t)p.n, nvec = (n + 3u) >> 2, self = (uint32_t)(p.row0 + r);
    const float* row = p.S + r * p.ld;
    int c = 0;
    for (uint32_t t = tid; t < nvec; t += 256) c += __popc(neighbours4(row, t, n, self, p.thr));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (tid == 0) {
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        p.count[r] = total;
        p.core[r] = total >= p.min_samples ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void dbscan_fill_kernel(const RowsParams p) {
    __shared__ int wsum[2][4];
    const int tid = threadIdx.x;
    const long long r = blockIdx.x;
    const uint32_t n = (uint32_t)p.n, nvec = (n + 3u) >> 2, self = (uint32_t)(p.row0 + r);
    const float* row = p.S + r * p.ld;
    const long long base = p.rowptr[r];
    const long long end = min((long long)p.rowptr[r + 1], p.cap);     // never at or past the next row, never past the array
    long long found = 0;                                               // neighbours in the columns walked so far (the same in every thread)
    int it = 0;
    for (uint32_t c0 = 0; c0 < nvec; c0 += 256, ++it) {
        const uint32_t t = c0 + tid;
        const int m = t < nvec ? neighbours4(row, t, n, self, p.thr) : 0;
        int total;                          // one barrier per step: the next step writes the other half of wsum
        long long pos = base + found + ranking::block_excl_scan(__popc(m), wsum[it & 1], total);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (m >> u & 1) {
                if (pos >= 0 && pos < end) p.cols[pos] = (int32_t)(4 * t + u);
                ++pos;
            }
        found += total;
    }
}

struct GraphParams {
    const int64_t* rowptr; const int32_t* cols; long long nnz;      // the eps-neighbour CSR of all N rows
    const uint8_t* core;
    int32_t* parent; int32_t* label; int32_t* changed;
    int N;
};

constexpr int ROW_LANES = 16;                   // lanes that share one row of the CSR
constexpr int ROWS_PER_BLOCK = 256 / ROW_LANES;

// the lane group's row and its slice of cols, clipped to the array; false for a row past N or a non-core row
__device__ __forceinline__ bool core_row(const GraphParams& p, long long& i, long long& b, long long& e) {
    i = (long long)blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / ROW_LANES;
    if (i >= p.N || !p.core[i]) return false;
    b = max((long long)p.rowptr[i], 0LL);
    e = min((long long)p.rowptr[i + 1], p.nnz);
    return true;
}

__global__ __launch_bounds__(256) void dbscan_hook_kernel(const GraphParams p) {
    long long i, b, e;
    bool differ = false;
    if (core_row(p, i, b, e)) {
        const uint32_t N = (uint32_t)p.N;
        const int ru = p.parent[i];
        for (long long t = b + threadIdx.x % ROW_LANES; t < e; t += ROW_LANES) {
            const int j = p.cols[t];
            if ((uint32_t)j >= N || !p.core[j]) continue;           // an index outside its range is skipped
            const int rv = p.parent[j];
            if (rv == ru || (uint32_t)ru >= N || (uint32_t)rv >= N) continue;
            atomicMin(&p.parent[max(ru, rv)], min(ru, rv));         // parent[x] <= x stays true: min < max
            differ = true;
        }
    }
    const unsigned long long saw = __ballot(differ);                // every lane of the wave is here again
    if (saw != 0ull && (threadIdx.x & 63) == __ffsll((long long)saw) - 1) atomicAdd(p.changed, 1);
}

__global__ __launch_bounds__(256) void dbscan_compress_kernel(int32_t* parent, int N) {
    const long long x = blockIdx.x * 256LL + threadIdx.x;
    if (x >= N) return;
    int r = parent[x];
    // strictly decreasing until the fixed point: at most x steps.  A value that breaks parent[r] <= r (not ours) ends the chase.
    for (long long step = 0; step <= x; ++step) {
        if ((uint32_t)r >= (uint32_t)N) return;
        const int q = parent[r];
        if (q >= r) break;
        r = q;
    }
    parent[x] = r;
}

__global__ __launch_bounds__(256) void dbscan_border_kernel(const GraphParams p) {
    long long i, b, e;
    if (!core_row(p, i, b, e)) return;
    const uint32_t N = (uint32_t)p.N;
    const int root = p.parent[i];
    for (long long t = b + threadIdx.x % ROW_LANES; t < e; t += ROW_LANES) {
        const int j = p.cols[t];
        if ((uint32_t)j < N && !p.core[j]) atomicMin(&p.label[j], root);
    }
}

}  // namespace

#define DBSCAN_CHECK_ROWS(name)                                                                                                     \
    REID_CHECK_ARG(nr >= 1 && n >= 1 && ld >= n && ld % 4 == 0, name ": nr=%d n=%d ld=%lld (ld >= n, ld %% 4 == 0)", nr, n, (long long)ld); \
    REID_CHECK_ARG(row0 >= 0 && row0 + nr <= n, name ": row0=%lld nr=%d n=%d (rows row0 .. row0 + nr - 1 must be columns of the matrix)",   \
                   (long long)row0, nr, n);                                                                                         \
    REID_CHECK_ARG(thr == thr, name ": thr is NaN");                                                                                \
    REID_CHECK_ARG(((uintptr_t)scores & 15) == 0, name ": scores must be 16-byte aligned")

extern "C" int reid_dbscan_count(const float* scores, int64_t ld, int32_t nr, int32_t n, int64_t row0, float thr, int32_t min_samples,
                                 int32_t* count, uint8_t* core, void* stream) {
    REID_CHECK_ARG(scores && count && core, "reid_dbscan_count: null pointer");
    DBSCAN_CHECK_ROWS("reid_dbscan_count");
    REID_CHECK_ARG(min_samples >= 1, "reid_dbscan_count: min_samples=%d (>= 1: a row counts itself)", min_samples);
    const RowsParams p{scores, (long long)ld, (long long)row0, thr, n, min_samples, count, core, nullptr, nullptr, 0};
    hipLaunchKernelGGL(dbscan_count_kernel, dim3(nr), dim3(256), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_dbscan_count");
    return REID_OK;
}

extern "C" int reid_dbscan_fill(const float* scores, int64_t ld, int32_t nr, int32_t n, int64_t row0, float thr, const int64_t* rowptr,
                                int32_t* cols, int64_t cap, void* stream) {
    REID_CHECK_ARG(scores && rowptr, "reid_dbscan_fill: null pointer");
    REID_CHECK_ARG(cap >= 0 && (cols || cap == 0), "reid_dbscan_fill: cap=%lld (null array of columns)", (long long)cap);
    DBSCAN_CHECK_ROWS("reid_dbscan_fill");
    if (cap == 0) return REID_OK;
    const RowsParams p{scores, (long long)ld, (long long)row0, thr, n, 1, nullptr, nullptr, rowptr, cols, (long long)cap};
    hipLaunchKernelGGL(dbscan_fill_kernel, dim3(nr), dim3(256), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_dbscan_fill");
    return REID_OK;
}

#define DBSCAN_CHECK_GRAPH(name)                                                                                   \
    REID_CHECK_ARG(N >= 1, name ": N=%d", N);                                                                      \
    REID_CHECK_ARG(nnz >= 0 && (cols || nnz == 0), name ": nnz=%lld (null array of columns)", (long long)nnz)

extern "C" int reid_dbscan_hook(const int64_t* rowptr, const int32_t* cols, int64_t nnz, const uint8_t* core, int32_t* parent, int32_t N,
                                int32_t* changed, void* stream) {
    REID_CHECK_ARG(rowptr && core && parent && changed, "reid_dbscan_hook: null pointer");
    DBSCAN_CHECK_GRAPH("reid_dbscan_hook");
    const GraphParams p{rowptr, cols, (long long)nnz, core, parent, nullptr, changed, N};
    hipLaunchKernelGGL(dbscan_hook_kernel, dim3((unsigned)((N + (long long)ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_dbscan_hook");
    return REID_OK;
}

extern "C" int reid_dbscan_compress(int32_t* parent, int32_t N, void* stream) {
    REID_CHECK_ARG(parent, "reid_dbscan_compress: null pointer");
    REID_CHECK_ARG(N >= 1, "reid_dbscan_compress: N=%d", N);
    hipLaunchKernelGGL(dbscan_compress_kernel, dim3((unsigned)((N + 255LL) / 256)), dim3(256), 0, (hipStream_t)stream, parent, N);
    REID_CHECK_LAUNCH("reid_dbscan_compress");
    return REID_OK;
}

extern "C" int reid_dbscan_border(const int64_t* rowptr, const int32_t* cols, int64_t nnz, const uint8_t* core, const int32_t* parent,
                                  int32_t* label, int32_t N, void* stream) {
    REID_CHECK_ARG(rowptr && core && parent && label, "reid_dbscan_border: null pointer");
    DBSCAN_CHECK_GRAPH("reid_dbscan_border");
    const GraphParams p{rowptr, cols, (long long)nnz, core, const_cast<int32_t*>(parent), label, nullptr, N};
    hipLaunchKernelGGL(dbscan_border_kernel, dim3((unsigned)((N + (long long)ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_dbscan_border");
    return REID_OK;
}
