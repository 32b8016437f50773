// k-reciprocal re-ranking (Zhong et al., CVPR 2017) on dense pooled rows, N = Nq + Ng <= 65 536 (definition: DESIGN.md
// "k-reciprocal re-ranking"; the reference has no re-ranking, so there is no reference line to cite).
//
//   reid_rerank_weights   one wave per pooled row i: the reciprocal set R(i, k1) from the kNN lists, its expansion R*(i) by the
//                         (2/3)-overlap rule on R(j, kh), then V[i, c] = exp(-(1 - x_i.x_c)) / sum over R*(i) -- integer work on
//                         lists of at most k1 + 1 <= 65 entries in LDS, fp32 dots across the wave, a fixed-order sum, no atomics.
//   reid_rerank_expand    V2[i, :] = mean of V[nbr[i, t], :], t < k2: a row gather, 16-byte accesses, HBM-bound.
//   reid_rerank_jaccard   s*[q, g] = (1 - lambda) m / (2 - m) + lambda cos[q, g], m = sum_j min(A[q, j], B[g, j]): the hot path, a
//                         TN-GEMM-shaped VALU kernel (128 x 128 tile, 8 x 8 accumulators per lane, operands through LDS as [k][row] so
//                         every lane reads its 8 + 8 values with four ds_read_b128) whose inner operation is v_min_f32 + v_add_f32.
//                         A k-step in which the A tile or the B tile holds no non-zero adds exactly +0 to every accumulator (the
//                         rows are non-negative) and is skipped: V2 is > 99 % zeros at protocol scale.
//
// The sparse form (any N that int32 row indices hold; layout: include/reid_hip.h) stores only the non-zeros:
//   reid_rerank_weights_sparse   the same kernel; its last loop writes the R*(i) list and its weights as one padded row of
//                                (column, value) plus vcnt[i], in place of the scatter into a zero-filled dense row.
//   reid_rerank_expand_count /   one workgroup per pooled row: the <= k2 W entries of the padded rows nbr[i, t], t < k2, as
//   reid_rerank_expand_sparse    (column << 8 | t) keys in LDS, one bitonic sort, then every run of one column is summed in ascending
//                                t and divided by k2 -- the dense kernel's value bit for bit.  The count pass writes the number of
//                                runs; the fill pass writes them, columns ascending, at rowptr[i].
//   reid_rerank_jaccard_sparse   the hot path: one workgroup owns one out row.  It zero-fills the row, walks the query's CSR columns
//                                in ascending order and for each the column's CSC list across the threads (gallery rows of one
//                                column are distinct: no two threads touch one element), a barrier between columns, so m[q, g]
//                                accumulates in the out row in ascending column order; one finishing pass blends in the cosine row.
#include "rank.h"

namespace {

using ranking::block_excl_scan;

constexpr int K1_MAX = 64;
constexpr int LIST_MAX = K1_MAX + 1;                       // entries of a kNN list that are read: k1 + 1
constexpr int KH_MAX = K1_MAX / 2;                         // kh = round-half-even(k1 / 2) <= 32, so a list of kh + 1 fits one wave
// |R*(i)| <= |R(i, k1)| + sum over j of |R(j, kh)| <= (k1 + 1) + (k1 + 1)(kh + 1) = (k1 + 1)(kh + 2): the size of the LDS list

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// ---------------------------------------------------------------------------------------------------------------------
// One wave (64 threads) per pooled row.  An index outside [0, N) in nbr (never produced for k1 + 1 <= N) is treated as absent.
// SPARSE: V is vvals and vcols its columns, both [N, ldv]; row i gets R*(i) in list order at positions < vcnt[i] = |R*(i)|.
template <bool SPARSE>
__global__ __launch_bounds__(64) void rerank_weights_kernel(const int32_t* __restrict__ nbr, int ldn, const float* __restrict__ X,
                                                            int ldx, float* __restrict__ V, long long ldv, int32_t* __restrict__ vcols,
                                                            int32_t* __restrict__ vcnt, int N, int D, int k1, int kh) {
    __shared__ int Li[LIST_MAX];        // nbr[i, :k1+1]
    __shared__ int Ri[LIST_MAX];        // R(i, k1) in list order
    extern __shared__ int dyn[];        // 2 x (k1 + 1)(kh + 2) words
    int* Rs = dyn;                      // R*(i): R(i, k1), then the accepted R(j, kh) in order of j, without repeats
    float* Es = (float*)(dyn + (k1 + 1) * (kh + 2));
    const int i = blockIdx.x, lane = threadIdx.x;
    const int n1 = k1 + 1, nh = kh + 1;
    for (int t = lane; t < n1; t += 64) Li[t] = nbr[(long long)i * ldn + t];
    __syncthreads();
    // R(i, k1): entries j of the list whose own list holds i
    int nR = 0;
    for (int t0 = 0; t0 < n1; t0 += 64) {
        const int t = t0 + lane;
        bool in = false;
        if (t < n1) {
            const int j = Li[t];
            if (j >= 0 && j < N) {
                const int32_t* lj = nbr + (long long)j * ldn;
                for (int u = 0; u < n1; ++u) in |= lj[u] == i;
            }
        }
        const unsigned long long m = __ballot(in);
        if (in) Ri[nR + lanes_below(m)] = Li[t];
        nR += __popcll(m);
    }
    __syncthreads();
    for (int t = lane; t < nR; t += 64) Rs[t] = Ri[t];
    int nS = nR;
    __syncthreads();
    // expansion: lane t holds candidate c = nbr[j, t] of R(j, kh); the test uses the ORIGINAL R(i, k1)
    for (int r = 0; r < nR; ++r) {
        const int j = Ri[r];
        int c = -1;
        bool in = false;
        if (lane < nh) {
            c = nbr[(long long)j * ldn + lane];
            if (c >= 0 && c < N) {
                const int32_t* lc = nbr + (long long)c * ldn;
                for (int u = 0; u < nh; ++u) in |= lc[u] == j;
            }
        }
        bool both = false;
        if (in)
            for (int u = 0; u < nR; ++u) both |= Ri[u] == c;
        const int cnt = __popcll(__ballot(in)), inter = __popcll(__ballot(both));
        if (3 * inter > 2 * cnt) {                                 // wave-uniform
            bool fresh = in;
            if (in)
                for (int u = 0; u < nS; ++u) fresh &= Rs[u] != c;   // every lane reads the same address: an LDS broadcast
            const unsigned long long m = __ballot(fresh);
            if (fresh) Rs[nS + lanes_below(m)] = c;
            nS += __popcll(m);
            __syncthreads();
        }
    }
    // weights: one fp32 dot per member, the wave across D
    const float* xi = X + (long long)i * ldx;
    for (int s = 0; s < nS; ++s) {
        const float* xc = X + (long long)Rs[s] * ldx;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) acc = fmaf(xi[d], xc[d], acc);
        acc = wave_sum(acc);
        if (lane == 0) Es[s] = expf(acc - 1.0f);                    // exp(-d), d = 1 - cos
    }
    __syncthreads();
    float sum = 0.f;
    for (int s = lane; s < nS; s += 64) sum += Es[s];               // fixed order: strided partials, then the butterfly
    sum = wave_sum(sum);
    if constexpr (SPARSE) {
        for (int s = lane; s < nS; s += 64) {
            vcols[(long long)i * ldv + s] = Rs[s];
            V[(long long)i * ldv + s] = Es[s] / sum;
        }
        if (lane == 0) vcnt[i] = nS;
    } else {
        for (int s = lane; s < nS; s += 64) V[(long long)i * ldv + Rs[s]] = Es[s] / sum;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rerank_expand_kernel(const float* __restrict__ V, long long ldv, const int32_t* __restrict__ nbr,
                                                            int ldn, float* __restrict__ V2, long long ldo, int N, int k2) {
    const int i = blockIdx.x;                                        // rows on x, the grid dimension whose limit is far above N
    const int c = 4 * (blockIdx.y * 256 + threadIdx.x);
    if (c >= N) return;
    const int32_t* li = nbr + (long long)i * ldn;
    float* out = V2 + (long long)i * ldo + c;
    if (c + 4 <= N) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < k2; ++t) {
            const int j = li[t];
            if (j < 0 || j >= N) continue;
            const f32x4 v = *(const f32x4*)(V + (long long)j * ldv + c);
            acc = t == 0 ? v : acc + v;
        }
        *(f32x4*)out = acc / (float)k2;
    } else {
        for (int e = 0; c + e < N; ++e) {
            float acc = 0.f;
            for (int t = 0; t < k2; ++t) {
                const int j = li[t];
                if (j < 0 || j >= N) continue;
                const float v = V[(long long)j * ldv + c + e];
                acc = t == 0 ? v : acc + v;
            }
            out[e] = acc / (float)k2;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int JT = 128;            // tile: JT query rows x JT gallery rows per workgroup of 256 threads
constexpr int JK = 16;             // pooled columns per k-step
constexpr int JLD = JT + 4;        // LDS row of one k: 132 floats (16-byte multiple; spreads the transposing writes over the banks)

struct JaccardParams {
    const float* A; const float* B; const float* cosr; float* out;
    long long lda, ldb, ldc, ldo;
    int nq, Ng, N;
    float lambda;
};

// 2 x float4 of one operand's tile for this thread: row (tid >> 2) and (tid >> 2) + 64, columns k0 + 4 (tid & 3) .. + 3; zeros past the edges
__device__ __forceinline__ void jaccard_fetch(const float* __restrict__ M, long long ld, int rows, int row0, int k0, int N, int tid,
                                              f32x4 (&v)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = row0 + (tid >> 2) + 64 * h, k = k0 + 4 * (tid & 3);
        v[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < rows) {
            const float* p = M + (long long)r * ld + k;
            if (k + 4 <= N) v[h] = *(const f32x4*)p;
            else
#pragma unroll
                for (int e = 0; e < 4; ++e) if (k + e < N) v[h][e] = p[e];
        }
    }
}

__global__ __launch_bounds__(256, 2) void rerank_jaccard_kernel(const JaccardParams p) {
    __shared__ __attribute__((aligned(16))) float As[JK][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JK][JLD];
    __shared__ int any_nz[2][2];                                   // [parity of the k-step][A, B]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int q0 = blockIdx.y * JT, g0 = blockIdx.x * JT;
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
    if (tid < 4) (&any_nz[0][0])[tid] = 0;
    f32x4 ra[2], rb[2];
    jaccard_fetch(p.A, p.lda, p.nq, q0, 0, p.N, tid, ra);
    jaccard_fetch(p.B, p.ldb, p.Ng, g0, 0, p.N, tid, rb);
    __syncthreads();
    int par = 0;
    for (int k0 = 0; k0 < p.N; k0 += JK, par ^= 1) {
        // stage the fetched k-step, transposed to [k][row]; note whether either tile holds a non-zero (plain stores of the same value)
        bool nza = false, nzb = false;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = (tid >> 2) + 64 * h, k = 4 * (tid & 3);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                As[k + e][r] = ra[h][e]; Bs[k + e][r] = rb[h][e];
                nza |= ra[h][e] != 0.f; nzb |= rb[h][e] != 0.f;
            }
        }
        if (nza) any_nz[par][0] = 1;
        if (nzb) any_nz[par][1] = 1;
        __syncthreads();
        if (k0 + JK < p.N) {                                        // next k-step: in flight under the arithmetic below
            jaccard_fetch(p.A, p.lda, p.nq, q0, k0 + JK, p.N, tid, ra);
            jaccard_fetch(p.B, p.ldb, p.Ng, g0, k0 + JK, p.N, tid, rb);
        }
        if (any_nz[par][0] & any_nz[par][1]) {                      // workgroup-uniform; a skipped step would have added +0 everywhere
#pragma unroll 2
            for (int k = 0; k < JK; ++k) {
                const f32x4 a0 = *(const f32x4*)&As[k][4 * ty], a1 = *(const f32x4*)&As[k][64 + 4 * ty];
                const f32x4 b0 = *(const f32x4*)&Bs[k][4 * tx], b1 = *(const f32x4*)&Bs[k][64 + 4 * tx];
                const float a[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                const float b[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int w = 0; w < 8; ++w) acc[u][w] += fminf(a[u], b[w]);
            }
        }
        __syncthreads();
        if (tid < 2) any_nz[par][tid] = 0;                          // read again two k-steps on, past the next barrier
    }
    const float lam = p.lambda, one_m = 1.0f - p.lambda;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = q0 + 4 * ty + (u & 3) + 64 * (u >> 2);
        if (q >= p.nq) continue;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int g = g0 + 4 * tx + (w & 3) + 64 * (w >> 2);
            if (g >= p.Ng) continue;
            const float m = acc[u][w];
            p.out[(long long)q * p.ldo + g] = one_m * (m / (2.0f - m)) + lam * p.cosr[(long long)q * p.ldc + g];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int SPARSE_MERGE_MAX = REID_RERANK_MERGE_MAX;   // entries one row's merge holds in LDS: 12 bytes each, 96 KB of the CU's 160 KB at the most.
// A call takes what its own bound needs: cap = k2 W rounded up to a power of two (the defaults: 2048 entries, 24 KB, six workgroups per CU).
constexpr int XT = 256;                  // threads of the merge workgroup (block_excl_scan's workgroup size)

// One workgroup per pooled row i.  FILL = false: cnt[i] = number of distinct columns in the union of the padded rows nbr[i, t], t < k2.
// FILL = true: those columns ascending and their values at rowptr[i] (never past rowptr[i + 1]).  A list entry outside [0, N) is
// skipped, as in the dense kernel; a vcnt outside [0, W] is clamped, so the merge never exceeds k2 * W <= cap entries.
template <bool FILL>
__global__ __launch_bounds__(XT) void rerank_expand_sparse_kernel(const int32_t* __restrict__ vcols, const float* __restrict__ vvals,
                                                                  const int32_t* __restrict__ vcnt, long long ldw,
                                                                  const int32_t* __restrict__ nbr, int ldn, int32_t* __restrict__ cnt,
                                                                  const long long* __restrict__ rowptr, int32_t* __restrict__ cols,
                                                                  float* __restrict__ vals, int N, int k2, int W, int cap) {
    extern __shared__ unsigned long long merge_lds[];              // cap keys, then cap values
    unsigned long long* key = merge_lds;                           // column << 8 | t: one sort orders the columns and, inside one, t
    float* val = (float*)(merge_lds + cap);
    __shared__ int src[LIST_MAX], off[LIST_MAX + 1], ws[XT / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (tid < k2) {
        const int j = nbr[(long long)i * ldn + tid];
        const bool ok = j >= 0 && j < N;
        src[tid] = ok ? j : -1;
        off[tid + 1] = ok ? min(max(vcnt[j], 0), W) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        off[0] = 0;
        for (int t = 0; t < k2; ++t) off[t + 1] += off[t];
    }
    __syncthreads();
    const int n = off[k2];
    int P = 1;
    while (P < n) P <<= 1;
    for (int t = tid >> 6; t < k2; t += XT / 64) {                  // a wave per source row
        const int j = src[t], o = off[t], c = off[t + 1] - o;
        for (int s = tid & 63; s < c; s += 64) {
            key[o + s] = ((unsigned long long)(uint32_t)vcols[(long long)j * ldw + s] << 8) | (unsigned)t;
            val[o + s] = vvals[(long long)j * ldw + s];
        }
    }
    for (int e = n + tid; e < P; e += XT) key[e] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = tid; e < P / 2; e += XT) {
                const int a = ((e & ~(j - 1)) << 1) | (e & (j - 1)), b = a | j;
                const unsigned long long ka = key[a], kb = key[b];
                if ((ka > kb) == ((a & k) == 0)) {
                    key[a] = kb; key[b] = ka;
                    const float v = val[a]; val[a] = val[b]; val[b] = v;
                }
            }
            __syncthreads();
        }
    // thread tid owns entries [e0, e1): the heads of the column runs among them
    const int per = (n + XT - 1) / XT, e0 = min(n, tid * per), e1 = min(n, e0 + per);
    int heads = 0;
    for (int e = e0; e < e1; ++e) heads += e == 0 || (key[e] >> 8) != (key[e - 1] >> 8);
    int total;
    int rank = block_excl_scan(heads, ws, total);
    if constexpr (!FILL) {
        if (tid == 0) cnt[i] = total;
    } else {
        const long long base = rowptr[i], room = rowptr[i + 1] - base;
        const float k2f = (float)k2;
        for (int e = e0; e < e1; ++e) {
            const unsigned long long c = key[e] >> 8;
            if (e != 0 && c == (key[e - 1] >> 8)) continue;
            float acc = val[e];                                     // ascending t; the absent terms are the dense kernel's exact + 0
            for (int u = e + 1; u < n && (key[u] >> 8) == c; ++u) acc += val[u];
            if (rank < room) {
                cols[base + rank] = (int32_t)c;
                vals[base + rank] = acc / k2f;
            }
            ++rank;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int SJ = 128;            // threads per out row: the CSC lists are a few hundred entries, and more rows are in flight per CU

struct JaccardSparseParams {
    const long long* rowptr; const int32_t* cols; const float* vals;        // CSR of the query rows (absolute offsets)
    const long long* colptr; const int32_t* rows; const float* cvals;       // CSC of the gallery rows
    const float* cosr; float* out;
    long long ldc, ldo, nnz, nnzc;
    int nq, Ng, N;
    float lambda;
};

__global__ __launch_bounds__(SJ) void rerank_jaccard_sparse_kernel(const JaccardSparseParams p) {
    __shared__ long long cb[SJ], ce[SJ];                            // a batch of the query's columns: CSC list bounds and the query's value
    __shared__ float ca[SJ];
    const int q = blockIdx.x, tid = threadIdx.x;
    float* out = p.out + (long long)q * p.ldo;                      // read and written by every thread, between barriers
    const float* __restrict__ cosr = p.cosr + (long long)q * p.ldc;
    for (int g = tid; g < p.Ng; g += SJ) out[g] = 0.f;
    const long long r0 = min(max(p.rowptr[q], 0ll), p.nnz), r1 = min(max(p.rowptr[q + 1], r0), p.nnz);
    for (long long b0 = r0; b0 < r1; b0 += SJ) {
        const int nb = (int)min((long long)SJ, r1 - b0);
        __syncthreads();                                            // the zero fill, or the last column of the batch before
        if (tid < nb) {
            const int j = p.cols[b0 + tid];
            long long lo = 0, hi = 0;
            if (j >= 0 && j < p.N) {
                lo = min(max(p.colptr[j], 0ll), p.nnzc);
                hi = min(max(p.colptr[j + 1], lo), p.nnzc);
            }
            cb[tid] = lo; ce[tid] = hi; ca[tid] = p.vals[b0 + tid];
        }
        __syncthreads();
        for (int c = 0; c < nb; ++c) {
            const long long lo = cb[c], hi = ce[c];
            if (lo == hi) continue;                                 // workgroup-uniform
            const float a = ca[c];
            for (long long e = lo + tid; e < hi; e += SJ) {
                const int g = p.rows[e];
                if (g >= 0 && g < p.Ng) out[g] += fminf(a, p.cvals[e]);
            }
            __syncthreads();                                        // the next column may touch the same gallery rows
        }
    }
    __syncthreads();
    const float lam = p.lambda, one_m = 1.0f - p.lambda;
    for (int g = tid; g < p.Ng; g += SJ) {
        const float m = out[g];
        out[g] = one_m * (m / (2.0f - m)) + lam * cosr[g];
    }
}

}  // namespace

static int rerank_kh(int k1) {           // round-half-to-even(k1 / 2)
    const int h = k1 / 2;
    return (k1 & 1) ? h + (h & 1) : h;
}

extern "C" int reid_rerank_weights(const int32_t* nbr, int32_t ldn, const float* X, int32_t ldx, float* V, int64_t ldv, int32_t N,
                                   int32_t D, int32_t k1, void* stream) {
    REID_CHECK_ARG(nbr && X && V, "reid_rerank_weights: null pointer");
    REID_CHECK_ARG(k1 >= 1 && k1 <= K1_MAX, "reid_rerank_weights: k1=%d outside 1..%d", k1, K1_MAX);
    REID_CHECK_ARG(N >= 1 && N <= 65536 && k1 + 1 <= N, "reid_rerank_weights: N=%d (k1 + 1 = %d <= N <= 65536)", N, k1 + 1);
    REID_CHECK_ARG(D >= 1 && ldx >= D && ldn >= k1 + 1 && ldv >= N, "reid_rerank_weights: D=%d ldx=%d ldn=%d ldv=%lld", D, ldx, ldn,
                   (long long)ldv);
    REID_CHECK_HIP(hipMemset2DAsync(V, (size_t)ldv * 4, 0, (size_t)N * 4, (size_t)N, (hipStream_t)stream), "reid_rerank_weights: zero fill");
    const int kh = rerank_kh(k1);
    hipLaunchKernelGGL(rerank_weights_kernel<false>, dim3(N), dim3(64), 8 * (k1 + 1) * (kh + 2), (hipStream_t)stream, nbr, ldn, X, ldx, V,
                       (long long)ldv, (int32_t*)nullptr, (int32_t*)nullptr, N, D, k1, kh);
    REID_CHECK_LAUNCH("reid_rerank_weights");
    return REID_OK;
}

extern "C" int reid_rerank_expand(const float* V, int64_t ldv, const int32_t* nbr, int32_t ldn, float* V2, int64_t ldo, int32_t N,
                                  int32_t k1, int32_t k2, void* stream) {
    REID_CHECK_ARG(V && nbr && V2, "reid_rerank_expand: null pointer");
    REID_CHECK_ARG(k1 >= 1 && k1 <= K1_MAX && k2 >= 1 && k2 <= k1 + 1, "reid_rerank_expand: k1=%d k2=%d (1 <= k1 <= %d, 1 <= k2 <= k1 + 1)",
                   k1, k2, K1_MAX);
    REID_CHECK_ARG(N >= 1 && N <= 65536 && ldn >= k2, "reid_rerank_expand: N=%d ldn=%d", N, ldn);
    REID_CHECK_ARG(ldv >= N && ldo >= N && ldv % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)V | (uintptr_t)V2) & 15) == 0,
                   "reid_rerank_expand: ldv=%lld ldo=%lld (>= N, multiples of 4, 16-byte aligned rows)", (long long)ldv, (long long)ldo);
    hipLaunchKernelGGL(rerank_expand_kernel, dim3(N, (N + 1023) / 1024), dim3(256), 0, (hipStream_t)stream, V, (long long)ldv, nbr, ldn, V2,
                       (long long)ldo, N, k2);
    REID_CHECK_LAUNCH("reid_rerank_expand");
    return REID_OK;
}

extern "C" int reid_rerank_jaccard(const float* A, int64_t lda, const float* B, int64_t ldb, const float* cosr, int64_t ldc, float* out,
                                   int64_t ldo, int32_t nq, int32_t Ng, int32_t N, float lambda, void* stream) {
    REID_CHECK_ARG(A && B && cosr && out, "reid_rerank_jaccard: null pointer");
    REID_CHECK_ARG(nq >= 1 && Ng >= 1 && N >= 1 && N <= 65536 && nq <= 65536 && Ng <= 65536, "reid_rerank_jaccard: nq=%d Ng=%d N=%d", nq, Ng, N);
    REID_CHECK_ARG(lda >= N && ldb >= N && lda % 4 == 0 && ldb % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) & 15) == 0,
                   "reid_rerank_jaccard: lda=%lld ldb=%lld (>= N, multiples of 4, 16-byte aligned rows)", (long long)lda, (long long)ldb);
    REID_CHECK_ARG(ldc >= Ng && ldo >= Ng && ldo % 4 == 0, "reid_rerank_jaccard: ldc=%lld ldo=%lld (>= Ng, ldo %% 4 == 0)", (long long)ldc,
                   (long long)ldo);
    JaccardParams p{A, B, cosr, out, (long long)lda, (long long)ldb, (long long)ldc, (long long)ldo, nq, Ng, N, lambda};
    hipLaunchKernelGGL(rerank_jaccard_kernel, dim3((Ng + JT - 1) / JT, (nq + JT - 1) / JT), dim3(256), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_rerank_jaccard");
    return REID_OK;
}

extern "C" int reid_rerank_weights_sparse(const int32_t* nbr, int32_t ldn, const float* X, int32_t ldx, int32_t* vcols, float* vvals,
                                          int32_t* vcnt, int64_t ldw, int32_t N, int32_t D, int32_t k1, void* stream) {
    REID_CHECK_ARG(nbr && X && vcols && vvals && vcnt, "reid_rerank_weights_sparse: null pointer");
    REID_CHECK_ARG(k1 >= 1 && k1 <= K1_MAX, "reid_rerank_weights_sparse: k1=%d outside 1..%d", k1, K1_MAX);
    REID_CHECK_ARG(N >= 1 && k1 + 1 <= N, "reid_rerank_weights_sparse: N=%d (k1 + 1 = %d <= N)", N, k1 + 1);
    const int kh = rerank_kh(k1), W = (k1 + 1) * (kh + 2);
    REID_CHECK_ARG(D >= 1 && ldx >= D && ldn >= k1 + 1 && ldw >= W, "reid_rerank_weights_sparse: D=%d ldx=%d ldn=%d ldw=%lld (ldw >= W = %d)", D,
                   ldx, ldn, (long long)ldw, W);
    hipLaunchKernelGGL(rerank_weights_kernel<true>, dim3(N), dim3(64), 8 * W, (hipStream_t)stream, nbr, ldn, X, ldx, vvals, (long long)ldw,
                       vcols, vcnt, N, D, k1, kh);
    REID_CHECK_LAUNCH("reid_rerank_weights_sparse");
    return REID_OK;
}

static int rerank_expand_sparse_args(const char* name, const void* vcols, const void* vvals, const void* vcnt, int64_t ldw, const void* nbr,
                                     int32_t ldn, int32_t N, int32_t k1, int32_t k2, int* W, int* cap) {
    REID_CHECK_ARG(vcols && vvals && vcnt && nbr, "%s: null pointer", name);
    REID_CHECK_ARG(k1 >= 1 && k1 <= K1_MAX && k2 >= 1 && k2 <= k1 + 1, "%s: k1=%d k2=%d (1 <= k1 <= %d, 1 <= k2 <= k1 + 1)", name, k1, k2,
                   K1_MAX);
    *W = (k1 + 1) * (rerank_kh(k1) + 2);
    REID_CHECK_ARG(k2 * *W <= SPARSE_MERGE_MAX, "%s: k1=%d k2=%d merge k2 (k1 + 1)(kh + 2) = %d entries per row, at most %d", name, k1, k2,
                   k2 * *W, SPARSE_MERGE_MAX);
    REID_CHECK_ARG(N >= 1 && ldn >= k2 && ldw >= *W, "%s: N=%d ldn=%d ldw=%lld (ldw >= W = %d)", name, N, ldn, (long long)ldw, *W);
    *cap = 64;
    while (*cap < k2 * *W) *cap <<= 1;
    return REID_OK;
}

extern "C" int reid_rerank_expand_count(const int32_t* vcols, const float* vvals, const int32_t* vcnt, int64_t ldw, const int32_t* nbr,
                                        int32_t ldn, int32_t* cnt, int32_t N, int32_t k1, int32_t k2, void* stream) {
    int W, cap;
    if (int rc = rerank_expand_sparse_args("reid_rerank_expand_count", vcols, vvals, vcnt, ldw, nbr, ldn, N, k1, k2, &W, &cap)) return rc;
    REID_CHECK_ARG(cnt, "reid_rerank_expand_count: null pointer");
    REID_MAX_LDS(rerank_expand_sparse_kernel<false>, 12 * SPARSE_MERGE_MAX);
    hipLaunchKernelGGL(rerank_expand_sparse_kernel<false>, dim3(N), dim3(XT), 12 * cap, (hipStream_t)stream, vcols, vvals, vcnt, (long long)ldw, nbr,
                       ldn, cnt, (const long long*)nullptr, (int32_t*)nullptr, (float*)nullptr, N, k2, W, cap);
    REID_CHECK_LAUNCH("reid_rerank_expand_count");
    return REID_OK;
}

extern "C" int reid_rerank_expand_sparse(const int32_t* vcols, const float* vvals, const int32_t* vcnt, int64_t ldw, const int32_t* nbr,
                                         int32_t ldn, const int64_t* rowptr, int32_t* cols, float* vals, int32_t N, int32_t k1, int32_t k2,
                                         void* stream) {
    int W, cap;
    if (int rc = rerank_expand_sparse_args("reid_rerank_expand_sparse", vcols, vvals, vcnt, ldw, nbr, ldn, N, k1, k2, &W, &cap)) return rc;
    REID_CHECK_ARG(rowptr && cols && vals, "reid_rerank_expand_sparse: null pointer");
    REID_MAX_LDS(rerank_expand_sparse_kernel<true>, 12 * SPARSE_MERGE_MAX);
    hipLaunchKernelGGL(rerank_expand_sparse_kernel<true>, dim3(N), dim3(XT), 12 * cap, (hipStream_t)stream, vcols, vvals, vcnt, (long long)ldw, nbr,
                       ldn, (int32_t*)nullptr, (const long long*)rowptr, cols, vals, N, k2, W, cap);
    REID_CHECK_LAUNCH("reid_rerank_expand_sparse");
    return REID_OK;
}

extern "C" int reid_rerank_jaccard_sparse(const int64_t* rowptr, const int32_t* cols, const float* vals, int64_t nnz, const int64_t* colptr,
                                          const int32_t* rows, const float* cvals, int64_t nnzc, const float* cosr, int64_t ldc, float* out,
                                          int64_t ldo, int32_t nq, int32_t Ng, int32_t N, float lambda, void* stream) {
    REID_CHECK_ARG(rowptr && colptr && cosr && out, "reid_rerank_jaccard_sparse: null pointer");
    REID_CHECK_ARG(nnz >= 0 && nnzc >= 0 && (nnz == 0 || (cols && vals)) && (nnzc == 0 || (rows && cvals)),
                   "reid_rerank_jaccard_sparse: nnz=%lld nnzc=%lld (null array of non-zeros)", (long long)nnz, (long long)nnzc);
    REID_CHECK_ARG(nq >= 1 && Ng >= 1 && N >= 1, "reid_rerank_jaccard_sparse: nq=%d Ng=%d N=%d", nq, Ng, N);
    REID_CHECK_ARG(ldc >= Ng && ldo >= Ng && ldo % 4 == 0, "reid_rerank_jaccard_sparse: ldc=%lld ldo=%lld (>= Ng, ldo %% 4 == 0)", (long long)ldc,
                   (long long)ldo);
    JaccardSparseParams p{(const long long*)rowptr, cols, vals, (const long long*)colptr, rows, cvals, cosr, out, (long long)ldc, (long long)ldo,
                          (long long)nnz, (long long)nnzc, nq, Ng, N, lambda};
    hipLaunchKernelGGL(rerank_jaccard_sparse_kernel, dim3(nq), dim3(SJ), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_rerank_jaccard_sparse");
    return REID_OK;
}
