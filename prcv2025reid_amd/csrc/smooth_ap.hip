// Cross-modal Smooth-AP ranking loss (Brown et al., "Smooth-AP: Smoothing the Path Towards Large-Scale Image Retrieval", ECCV 2020) for
// gfx950, fp32 in and out: P stacked query sides q [P*N, D] (one per non-vis modality) against the vis side g [Mg, D], ranked in both
// directions, either inside the batch or against the slots of a cross-batch memory (losses.CrossBatchMemory, filed by reid_xbm_enqueue).
// The reference has no such loss; include/reid_hip.h (reid_smooth_ap_*) and DESIGN.md section 24 are the definition.
//
// A direction of a pair is one set of ranking problems: anchors (rows of one side) against a gallery (rows, labels, validity bytes,
// count).  q->g: the q rows of pair p against gallery A (in the batch form g itself, in the ring form ring side 0); g->q: the g rows
// against gallery B of pair p (the q rows of pair p, or ring side p + 1).  The kernels see a direction as a `Dir`.
//
// Forward, launch 1 (sap_unit_kernel, normalize = 1 only): one wave per batch row: its fp32 unit row (triplet::unit_row) with
//   1 / max(|x|, eps) and |x| beside it -- what the gathers and the projection use -- and 1 / max(|x|, eps) in fp64 from an fp64 sum
//   of squares, what the scores use.
// Forward, launch 2 (sap_score_kernel): the score rows S [anchors, G] of both directions.  A workgroup owns 8 anchors x 256 gallery rows,
//   ONE GALLERY ROW PER LANE; [256][32]-float pieces of the gallery are staged in LDS (rows padded by 16 bytes: the per-lane ds_read_b128
//   of "my row" is conflict free) beside the anchors' columns (LDS broadcasts).  The dot product of the fp32 INPUT rows is an fp64 fma
//   chain, times the two fp64 reciprocal norms, rounded to fp32 ONCE (margin_ce.hip's rule: a score error moves a soft rank by up to
//   (G - 1) / (2 tau) times itself).  An invalid gallery row gets -inf: sigma and its derivative are exactly 0 there.
// Forward, launch 3 (sap_rank_kernel): one workgroup per anchor, its score row and a byte per gallery row (invalid / negative /
//   positive) in LDS.  Wave 0 lists the positives in ascending gallery index.  Pass 1: the waves take positives in ascending order, lanes
//   stride over j: R_i, R+_i and, with gradients, B_i = sum_j t_ij and A_i = sum_{j in P} t_ij, t = sigma (1 - sigma), each a per-lane
//   sum in ascending j and the butterfly of wave_sum.  Thread 0 adds R+_i / R_i in ascending i in fp64 -> AP_a.  Pass 2 (gradients): every
//   thread owns gallery rows j and walks the positives in ascending i: ds_j = -(1 / (tau |P|)) sum_{i != j} t_ij ([j in P] / R_i - R+_i /
//   R_i^2); a positive i then adds its own (1 / (tau |P|)) (A_i / R_i - B_i R+_i / R_i^2), which equals sum_j w_ij without a second
//   reduction.  sigma in the overflow-free form e = exp(-|d|): d >= 0 ? 1 / (1 + e) : e / (1 + e); t = e / (1 + e)^2 for either sign.
// Forward, launch 4 (sap_finalize_kernel): one workgroup per pair, the ordered fp64 sums of 1 - AP_a over the active anchors of either
//   direction -> result [P, 4] = {L_p, flag_p, n_qg, n_gq}.
// Forward, launch 5 (sap_gather_kernel, gradients only): a workgroup owns 4 output rows of one side of one pair.  The unit-space gradient
//   of a row is at most two sums: as an anchor, sum_j ds_aj * (gallery row j); in the batch form also as a gallery row of the other
//   direction, sum_a ds_aj * (unit row of anchor a).  Each wave takes a contiguous quarter of the summation index in ascending order (the
//   weights are uniform loads, the rows shared by the 4 outputs), the quarters are added in wave order through LDS, and the projection
//   through the normalisation follows in the same kernel (the block of cross_triplet.hip's xt_bwd_kernel).  The result, unscaled by the
//   cotangent, stays in ws: Hq [P*N, D] and Hg [P, Mg, D].  Ring rows are read HERE and never again: a later enqueue cannot change a
//   pending backward.
// Backward (sap_bwd_kernel): one wave per output row: dq = gscale[p] * Hq, dg = sum over p ascending of gscale[p] * Hg[p]; zeros for
//   invalid rows.
// No atomics anywhere: two runs give the same bits in every output.  Nothing is allocated, synchronised or read back.
#include "triplet_mine.h"

namespace {

using namespace triplet;

constexpr int SA = 8;                    // anchors per workgroup of the score kernel
constexpr int GO = 4;                    // output rows per workgroup of the gather kernel

// One direction.  Anchor (p, a) is row p * apair + a of its side (apair = na: the stacked q rows; 0: the shared g rows); gallery row (p, j)
// is row p * cpair + j of the gallery (cpair = nc: one gallery per pair; 0: shared).  Validity bytes are indexed like the rows.
struct Dir {
    const float* a; int lda; int na; int apair;                      // anchors: the fp32 INPUT rows
    const float* c; int ldc; int nc; int cpair;                      // gallery: the fp32 INPUT rows (ring: the slots)
    const double* ainv; const double* cinv;                          // fp64 1 / max(|x|, eps) per row, NULL: 1
    const int64_t* alab; const uint8_t* aval;                        // labels [na], validity [P or 1, na] or NULL
    const int64_t* clab; const uint8_t* cval;                        // labels [nc], validity [P or 1, nc] or NULL
    float* S; float* DS;                                             // [P, na, nc]: scores, d(1 - AP_a) / ds (DS: gradients only)
    float* ap; int* npos;                                            // [P, na]: AP_a (-1: inactive), |P_a|
};

// ws (floats; every piece a multiple of 4): Hq P N D | Hg P Mg D | unit rows R D | 1 / max(|x|, eps) R | |x| R | the same in fp64 2 R |
// S q->g P N Ga | S g->q P Mg Gb | DS q->g | DS g->q        (R = P N + Mg; H and DS only with gradients)
struct Ws {
    int64_t hq, hg, unit, inv, norm, inv64, s0, s1, ds0, ds1, total;
    static int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }
    Ws(int64_t P, int64_t N, int64_t Mg, int64_t D, int64_t Ga, int64_t Gb, int with_grad) {
        const int64_t R = P * N + Mg, g = with_grad ? 1 : 0;
        hq = 0; hg = hq + g * P * N * D; unit = hg + g * P * Mg * D; inv = unit + R * D; norm = inv + r4(R); inv64 = norm + r4(R);
        s0 = inv64 + r4(2 * R); s1 = s0 + r4(P * N * Ga); ds0 = s1 + r4(P * Mg * Gb); ds1 = ds0 + g * r4(P * N * Ga);
        total = ds1 + g * r4(P * Mg * Gb);
    }
};

// rows [0, PN) are q rows, rows [PN, PN + Mg) are g rows; one wave per row
__global__ __launch_bounds__(256) void sap_unit_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ g, int ldg, int PN, int Mg,
                                                       int D, float eps, float* __restrict__ unit, float* __restrict__ inv_out,
                                                       float* __restrict__ norm_out, double* __restrict__ inv64) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= PN + Mg) return;
    const float* x = row < PN ? q + (size_t)row * ldq : g + (size_t)(row - PN) * ldg;
    unit_row(x, D, eps, unit + (size_t)row * D, inv_out + row, norm_out + row, lane);
    double ss = 0.0;
    for (int c = 4 * lane; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(x + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fma((double)v[e], (double)v[e], ss);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) inv64[row] = 1.0 / fmax(sqrt(ss), (double)eps);
}

// blockIdx = (tile of 256 gallery rows, tile of SA anchors, pair * 2 + direction); a tile outside its direction's extent returns
__global__ __launch_bounds__(256) void sap_score_kernel(Dir d0, Dir d1, int D) {
    __shared__ __attribute__((aligned(16))) float cand[CB * PITCH];
    __shared__ __attribute__((aligned(16))) float anch[SA * DK];
    const Dir d = (blockIdx.z & 1) ? d1 : d0;
    const int p = blockIdx.z >> 1, tid = threadIdx.x;
    const int c0 = blockIdx.x * CB, a0 = blockIdx.y * SA;
    if (c0 >= d.nc || a0 >= d.na) return;                            // uniform over the workgroup
    const float* ar = d.a + (size_t)p * d.apair * d.lda;
    const float* cr = d.c + (size_t)p * d.cpair * d.ldc;
    double acc[SA];
#pragma unroll
    for (int a = 0; a < SA; ++a) acc[a] = 0.0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += DK) {
        const int nc4 = min(DK / 4, (D - k0) >> 2);                  // 16-byte chunks of this piece; the rest is staged as zeros
        __syncthreads();                                             // the previous piece has been read
#pragma unroll
        for (int u = 0; u < CB * (DK / 4) / 256; ++u) {              // rows past the end: clamped, dropped at the store
            const int e = tid + 256 * u, r = e >> 3, c4 = e & 7;
            *(f32x4*)(cand + r * PITCH + 4 * c4) = c4 < nc4 ? *(const f32x4*)(cr + (size_t)min(c0 + r, d.nc - 1) * d.ldc + k0 + 4 * c4) : zero4;
        }
        if (tid < SA * (DK / 4))
            *(f32x4*)(anch + 4 * tid) = (tid & 7) < nc4 ? *(const f32x4*)(ar + (size_t)min(a0 + (tid >> 3), d.na - 1) * d.lda + k0 + 4 * (tid & 7)) : zero4;
        __syncthreads();
#pragma unroll
        for (int c4 = 0; c4 < DK / 4; ++c4) {
            const f32x4 y = *(const f32x4*)(cand + tid * PITCH + 4 * c4);
#pragma unroll
            for (int a = 0; a < SA; ++a) {
                const f32x4 xa = *(const f32x4*)(anch + a * DK + 4 * c4);          // one address per wave: an LDS broadcast
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[a] = fma((double)xa[e], (double)y[e], acc[a]);
            }
        }
    }
    const int j = c0 + tid;
    if (j >= d.nc) return;
    const bool on = !d.cval || d.cval[(size_t)p * d.cpair + j];
    const double cj = d.cinv ? d.cinv[(size_t)p * d.cpair + j] : 1.0;
#pragma unroll
    for (int a = 0; a < SA; ++a)
        if (a0 + a < d.na) {
            const double ai = d.ainv ? d.ainv[(size_t)p * d.apair + a0 + a] : 1.0;
            d.S[((size_t)p * d.na + a0 + a) * d.nc + j] = on ? (float)(acc[a] * (ai * cj)) : -INFINITY;
        }
}

// e = exp(-|d|), r = 1 / (1 + e): sigma(d) = d >= 0 ? r : e r, sigma (1 - sigma) = e r r
__device__ __forceinline__ void sigmoid_parts(float d, float& sg, float& t) {
    const float e = expf(-fabsf(d));
    const float r = 1.f / (1.f + e);
    const float er = e * r;
    sg = d >= 0.f ? r : er;
    t = er * r;
}

// The dynamic LDS of the rank kernel for a gallery of G rows (G4 = G rounded up to 4): s [G4] | ratio [G4] (| v [G4] | u [G4]) floats,
// then the positives' indices as uint16 [G4], then a byte per row [G4]
__host__ __device__ inline int rank_lds_bytes(int G, int with_grad) {
    const int G4 = (G + 3) & ~3;
    return G4 * (4 * (with_grad ? 4 : 2) + 2 + 1);
}

// blockIdx: the anchors (p, a) of direction 0, then those of direction 1
template <bool GRAD>
__global__ __launch_bounds__(256) void sap_rank_kernel(Dir d0, Dir d1, int P, float inv_tau) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool first = (int)blockIdx.x < P * d0.na;
    const Dir d = first ? d0 : d1;
    const int r = first ? blockIdx.x : blockIdx.x - P * d0.na;       // r = p na + a: the anchor's slot in [P, na]
    const int p = r / d.na, a = r % d.na, G = d.nc, G4 = (G + 3) & ~3;
    float* s = smem;
    float* ratio = s + G4;
    float* v = ratio + G4;                                           // (GRAD only)
    float* u = v + G4;
    uint16_t* plist = (uint16_t*)(smem + (GRAD ? 4 : 2) * G4);
    uint8_t* kind = (uint8_t*)(plist + G4);
    const bool a_on = !d.aval || d.aval[(size_t)p * d.apair + a];
    const int64_t y = d.alab[a];
    const float* srow = d.S + (size_t)r * G;
    const uint8_t* cv = d.cval ? d.cval + (size_t)p * d.cpair : nullptr;
    for (int j = tid; j < G; j += 256) {
        s[j] = srow[j];
        kind[j] = cv && !cv[j] ? 0 : d.clab[j] == y ? 2 : 1;
    }
    __syncthreads();
    if (wave == 0) {                                                 // the positives in ascending gallery index, and the two counts
        int np = 0, nv = 0;
        for (int j0 = 0; j0 < G; j0 += 64) {
            const int j = j0 + lane;
            const int k = j < G ? kind[j] : 0;
            const unsigned long long mp = __ballot(k == 2), mv = __ballot(k != 0);
            if (k == 2) plist[np + __popcll(mp & ((1ull << lane) - 1ull))] = (uint16_t)j;
            np += __popcll(mp); nv += __popcll(mv);
        }
        if (lane == 0) { s_cnt[0] = np; s_cnt[1] = nv; }
    }
    __syncthreads();
    const int np = s_cnt[0], nv = s_cnt[1];
    if (!a_on || np == 0 || nv == np) {                              // inactive (uniform): AP is undefined or identically 1
        if (tid == 0) { d.ap[r] = -1.f; d.npos[r] = a_on ? np : 0; }
        return;
    }
    const float ka = inv_tau / (float)np;                            // 1 / (tau |P|)
    float* dsrow = GRAD ? d.DS + (size_t)r * G : nullptr;
    for (int k = wave; k < np; k += 4) {                             // pass 1: positive i = plist[k] against every gallery row
        const int i = plist[k];
        const float si = s[i];
        float sr = 0.f, srp = 0.f, sb = 0.f, sa = 0.f;
        for (int j = lane; j < G; j += 64) {
            float sg, t;
            sigmoid_parts((s[j] - si) * inv_tau, sg, t);
            if (j == i) { sg = 0.f; t = 0.f; }
            const bool pos = kind[j] == 2;
            sr += sg; srp += pos ? sg : 0.f;
            if (GRAD) { sb += t; sa += pos ? t : 0.f; }
        }
        const float R = 1.f + wave_sum(sr), Rp = 1.f + wave_sum(srp);
        if (GRAD) { sb = wave_sum(sb); sa = wave_sum(sa); }
        if (lane == 0) {
            const float rt = Rp / R;
            ratio[k] = rt;
            if (GRAD) {
                const float vi = 1.f / R, ui = rt * vi;              // 1 / R_i and R+_i / R_i^2
                v[k] = vi; u[k] = ui;
                dsrow[i] = ka * (vi * sa - ui * sb);                 // the positive's own term; pass 2 adds the rest
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < np; ++k) t += (double)ratio[k];
        d.ap[r] = (float)(t / (double)np);
        d.npos[r] = np;
    }
    if (GRAD) {
        for (int j = tid; j < G; j += 256) {                         // pass 2: gallery row j against every positive, ascending
            const int kj = kind[j];
            float acc = 0.f;
            if (kj) {
                const float sj = s[j];
                for (int k = 0; k < np; ++k) {
                    const int i = plist[k];
                    float sg, t;
                    sigmoid_parts((sj - s[i]) * inv_tau, sg, t);
                    const float coef = kj == 2 ? v[k] - u[k] : -u[k];
                    if (i != j) acc = fmaf(t, coef, acc);
                }
            }
            dsrow[j] = kj == 2 ? dsrow[j] - ka * acc : -ka * acc;    // (dsrow[j] of a positive: written in pass 1, before the barrier)
        }
    }
}

// one workgroup per pair: thread t adds anchors t, t + 256, ... of a direction in fp64, the 256 sums are added in index order (the tail
// of cross_triplet.hip's xt_finalize_kernel on 1 - AP_a)
__global__ __launch_bounds__(256) void sap_finalize_kernel(const float* __restrict__ q_ap, const float* __restrict__ g_ap, int N, int Mg,
                                                           float* __restrict__ result) {
    __shared__ double s_sum[2][256];
    __shared__ int s_cnt[2][256];
    const int tid = threadIdx.x, p = blockIdx.x;
    for (int dir = 0; dir < 2; ++dir) {
        const int n = dir ? Mg : N;
        const float* ap = dir ? g_ap + (size_t)p * Mg : q_ap + (size_t)p * N;
        double s = 0.0;
        int c = 0;
        for (int r = tid; r < n; r += 256)
            if (ap[r] >= 0.f) { s += 1.0 - (double)ap[r]; ++c; }
        s_sum[dir][tid] = s; s_cnt[dir][tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double t[2] = {0.0, 0.0};
        int c[2] = {0, 0};
        for (int dir = 0; dir < 2; ++dir)
            for (int u = 0; u < 256; ++u) { t[dir] += s_sum[dir][u]; c[dir] += s_cnt[dir][u]; }
        const double L = 0.5 * (t[0] / (double)(c[0] > 0 ? c[0] : 1) + t[1] / (double)(c[1] > 0 ? c[1] : 1));
        const bool any = c[0] + c[1] > 0;
        result[4 * p + 0] = any ? (float)L : 0.f;
        result[4 * p + 1] = any ? 1.f : 0.f;
        result[4 * p + 2] = (float)c[0];
        result[4 * p + 3] = (float)c[1];
    }
}

// One sum of the gather: out[r] += c * sum over x in [0, n) of W[r * wrow + x * wcol] * (row x of X), for the output rows r with on[r]
struct Term {
    const float* W; int64_t wrow, wcol;  // the weights of output row 0; strides to the next output row and the next x
    int n;
    const float* X; int ldx;
    const uint8_t* xvalid;               // [n] or NULL: rows that take part
    const float* xap;                    // [n] or NULL: x is an anchor, skipped when its AP is < 0 (its DS row was never written)
    const float* oap;                    // [GO-tile] or NULL: the outputs are anchors, a row with AP < 0 has no weights
    float c;
};

__device__ __forceinline__ void gather_term(f32x4 (&acc)[GO][NV], const Term& t, int rows, int wave, int lane, int D) {
    if (!t.W) return;
    bool on[GO];
#pragma unroll
    for (int r = 0; r < GO; ++r) on[r] = r < rows && (!t.oap || t.oap[r] >= 0.f);
    const int chunk = (t.n + 3) / 4, x1 = min(t.n, (wave + 1) * chunk);
    for (int x = wave * chunk; x < x1; ++x) {                        // this wave's quarter, ascending
        if ((t.xvalid && !t.xvalid[x]) || (t.xap && !(t.xap[x] >= 0.f))) continue;        // uniform
        f32x4 xr[NV];
        load_row(xr, t.X + (size_t)x * t.ldx, lane, D);
#pragma unroll
        for (int r = 0; r < GO; ++r) {
            const float w = on[r] ? t.c * t.W[r * t.wrow + x * t.wcol] : 0.f;
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r][v][e] = fmaf(w, xr[v][e], acc[r][v][e]);
        }
    }
}

// blockIdx = (pair, tile of GO q rows | tile of GO g rows).  U: the batch's unit rows (normalize = 1) or its rows, q rows then g rows.
__global__ __launch_bounds__(256) void sap_gather_kernel(Dir d0, Dir d1, Sides U, const float* __restrict__ G0, int ldg0, const float* __restrict__ G1,
                                                         int ldg1, int gallery_grad, int P, int N, int Mg, int D, int normalize, float eps,
                                                         const float* __restrict__ inv, const float* __restrict__ norm,
                                                         const float* __restrict__ result, float* __restrict__ Hq, float* __restrict__ Hg) {
    extern __shared__ __attribute__((aligned(16))) float part[];     // [4 waves][GO rows][D]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tq = (N + GO - 1) / GO, tg = (Mg + GO - 1) / GO;
    const int p = blockIdx.x / (tq + tg), t = blockIdx.x % (tq + tg);
    const bool is_q = t < tq;
    const int o0 = (is_q ? t : t - tq) * GO, rows = min(GO, (is_q ? N : Mg) - o0);
    const float c0 = 0.5f / fmaxf(result[4 * p + 2], 1.f), c1 = 0.5f / fmaxf(result[4 * p + 3], 1.f);
    const float* uq = U.q + (size_t)p * N * U.ldq;                   // pair p's q rows in unit space
    // (1) the rows as anchors of their direction, against its gallery; (2) batch form: as gallery rows of the other direction
    Term t1, t2;
    if (is_q) {
        t1 = Term{d0.DS + ((size_t)p * N + o0) * d0.nc, d0.nc, 1, d0.nc, G0, ldg0, d0.cval, nullptr, d0.ap + (size_t)p * N + o0, c0};
        t2 = Term{gallery_grad ? d1.DS + (size_t)p * Mg * d1.nc + o0 : nullptr, 1, d1.nc, Mg, U.g, U.ldg, nullptr, d1.ap + (size_t)p * Mg, nullptr, c1};
    } else {
        t1 = Term{d1.DS + ((size_t)p * Mg + o0) * d1.nc, d1.nc, 1, d1.nc, G1 + (size_t)p * d1.cpair * ldg1, ldg1,
                  d1.cval ? d1.cval + (size_t)p * d1.cpair : nullptr, nullptr, d1.ap + (size_t)p * Mg + o0, c1};
        t2 = Term{gallery_grad ? d0.DS + (size_t)p * N * d0.nc + o0 : nullptr, 1, d0.nc, N, uq, U.ldq, nullptr, d0.ap + (size_t)p * N, nullptr, c0};
    }
    f32x4 acc[GO][NV];
#pragma unroll
    for (int r = 0; r < GO; ++r) zero_acc(acc[r]);
    gather_term(acc, t1, rows, wave, lane, D);
    gather_term(acc, t2, rows, wave, lane, D);
#pragma unroll
    for (int r = 0; r < GO; ++r) store_row(part + ((size_t)wave * GO + r) * D, acc[r], lane, D);
    __syncthreads();
    if (wave >= rows) return;                                        // wave w finishes output row o0 + w
    const int me = o0 + wave;
    const int ur = is_q ? p * N + me : P * N + me;                   // its row among the batch's P N + Mg rows
    const bool valid = is_q ? (!d0.aval || d0.aval[(size_t)p * N + me]) : (!d1.aval || d1.aval[me]);
    f32x4 g[NV], xi[NV], w[NV];
    zero_acc(g);
    load_row(xi, is_q ? uq + (size_t)me * U.ldq : U.g + (size_t)me * U.ldg, lane, D, valid);
    if (valid) {                                                     // (an invalid row is no anchor and in nobody's gallery: zeros)
        for (int q = 0; q < 4; ++q) {                                // the quarters in wave order
            load_row(w, part + ((size_t)q * GO + wave) * D, lane, D);
#pragma unroll
            for (int v = 0; v < NV; ++v) g[v] = g[v] + w[v];
        }
        if (normalize) {
            if (norm[ur] >= eps) {                                   // dx = (G - x^ (x^ . G)) / max(|x|, eps); the same block as in
                float dot = 0.f;                                     // cross_triplet.hip's xt_bwd_kernel
#pragma unroll
                for (int v = 0; v < NV; ++v) dot += xi[v][0] * g[v][0] + xi[v][1] * g[v][1] + xi[v][2] * g[v][2] + xi[v][3] * g[v][3];
                dot = wave_sum(dot);
                const float iv = inv[ur];
#pragma unroll
                for (int v = 0; v < NV; ++v) g[v] = (g[v] - xi[v] * dot) * iv;
            } else {                                                 // x / norm.clamp_min(eps) is linear in x there: dx = G / eps
#pragma unroll
                for (int v = 0; v < NV; ++v) g[v] = g[v] / eps;
            }
        }
    }
    store_row(is_q ? Hq + ((size_t)p * N + me) * D : Hg + ((size_t)p * Mg + me) * D, g, lane, D);
}

// one wave per output row: rows [0, P N) of dq, then rows [0, Mg) of dg
__global__ __launch_bounds__(256) void sap_bwd_kernel(const uint8_t* __restrict__ q_valid, const uint8_t* __restrict__ g_valid, int P, int N, int Mg,
                                                      int D, const float* __restrict__ Hq, const float* __restrict__ Hg,
                                                      const float* __restrict__ gscale, float* __restrict__ dq, int lddq,
                                                      float* __restrict__ dg, int lddg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int PN = P * N;
    if (row >= PN + Mg) return;
    const bool is_q = row < PN;
    const int me = is_q ? row : row - PN;
    f32x4 acc[NV], h[NV];
    zero_acc(acc);
    if (is_q ? (!q_valid || q_valid[me]) : (!g_valid || g_valid[me])) {
        for (int p = is_q ? row / N : 0; p < (is_q ? row / N + 1 : P); ++p) {
            load_row(h, is_q ? Hq + (size_t)me * D : Hg + ((size_t)p * Mg + me) * D, lane, D);
            const float gs = gscale[p];
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[v][e] = fmaf(gs, h[v][e], acc[v][e]);
        }
    }
    store_row(is_q ? dq + (size_t)me * lddq : dg + (size_t)me * lddg, acc, lane, D);
}

int check_galleries(const char* who, int32_t Ga, int32_t Gb, int32_t with_grad) {
    REID_CHECK_ARG(Ga >= 1 && Ga <= MAX_ROWS, "%s: Ga=%d (1..8192)", who, Ga);
    REID_CHECK_ARG(Gb >= 1 && Gb <= MAX_ROWS, "%s: Gb=%d (1..8192)", who, Gb);
    REID_CHECK_ARG(with_grad == 0 || with_grad == 1, "%s: with_grad=%d (0 or 1)", who, with_grad);
    return REID_OK;
}

}  // namespace

extern "C" int64_t reid_smooth_ap_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D, int32_t Ga, int32_t Gb, int32_t with_grad) {
    const char* who = "reid_smooth_ap_ws_floats";
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_galleries(who, Ga, Gb, with_grad)) return rc;
    return Ws(P, N, Mg, D, Ga, Gb, with_grad).total;
}

extern "C" int reid_smooth_ap_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label, const int64_t* g_label,
                                  const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg, int32_t D, float tau,
                                  int32_t normalize, float eps, const float* ga, int32_t ldga, const int64_t* ga_label,
                                  const uint8_t* ga_valid, int32_t Ga, const float* gb, int32_t ldgb, const int64_t* gb_label,
                                  const uint8_t* gb_valid, int32_t Gb, int32_t gallery_grad, int32_t with_grad, float* q_ap,
                                  int32_t* q_npos, float* g_ap, int32_t* g_npos, float* ws, float* result, void* stream) {
    const char* who = "reid_smooth_ap_fwd";
    REID_CHECK_ARG(q && g && q_label && g_label && ga && ga_label && gb && gb_label && q_ap && q_npos && g_ap && g_npos && ws && result,
                   "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_galleries(who, Ga, Gb, with_grad)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, ldq, "ldq")) return rc;
    if (int rc = check_ld(who, Mg, D, ldg, "ldg")) return rc;
    if (int rc = check_ld(who, Ga, D, ldga, "ldga")) return rc;
    if (int rc = check_ld(who, (int64_t)P * Gb, D, ldgb, "ldgb")) return rc;
    if (int rc = check_scalars(who, 0.f, normalize, eps)) return rc;
    REID_CHECK_ARG(tau > 0.f && tau <= 3.402823466e38f, "%s: tau=%g (finite, > 0)", who, (double)tau);
    REID_CHECK_ARG(gallery_grad == 0 || gallery_grad == 1, "%s: gallery_grad=%d (0 or 1)", who, gallery_grad);
    REID_CHECK_ARG(!gallery_grad || (ga == g && ldga == ldg && ga_label == g_label && ga_valid == g_valid && Ga == Mg && gb == q && ldgb == ldq &&
                                     gb_label == q_label && gb_valid == q_valid && Gb == N),
                   "%s: gallery_grad=1 needs the batch itself as the galleries (ga = g, gb = q, with their labels, validity and counts)", who);
    REID_CHECK_ARG(aligned16(q) && aligned16(g) && aligned16(ga) && aligned16(gb) && aligned16(ws), "%s: q, g, ga, gb or ws is not 16-byte aligned", who);
    const Ws w(P, N, Mg, D, Ga, Gb, with_grad);
    hipStream_t s = (hipStream_t)stream;
    const int PN = P * N;
    Sides U{q, ldq, g, ldg};
    const double* inv64 = nullptr;
    if (normalize) {
        hipLaunchKernelGGL(sap_unit_kernel, dim3((PN + Mg + 3) / 4), dim3(256), 0, s, q, ldq, g, ldg, PN, Mg, D, eps, ws + w.unit, ws + w.inv,
                           ws + w.norm, (double*)(ws + w.inv64));
        REID_CHECK_LAUNCH("reid_smooth_ap_fwd(unit rows)");
        U = Sides{ws + w.unit, D, ws + w.unit + (size_t)PN * D, D};
        inv64 = (const double*)(ws + w.inv64);
    }
    // the galleries' own reciprocal norms: the batch's in the batch form; ring rows are taken as they are
    const bool own = normalize && gallery_grad;
    const Dir d0{q, ldq, N, N, ga, ldga, Ga, 0, inv64, own ? inv64 + PN : nullptr, q_label, q_valid, ga_label, ga_valid,
                 ws + w.s0, with_grad ? ws + w.ds0 : nullptr, q_ap, q_npos};
    const Dir d1{g, ldg, Mg, 0, gb, ldgb, Gb, Gb, inv64 ? inv64 + PN : nullptr, own ? inv64 : nullptr, g_label, g_valid, gb_label, gb_valid,
                 ws + w.s1, with_grad ? ws + w.ds1 : nullptr, g_ap, g_npos};
    const int gmax = Ga > Gb ? Ga : Gb, amax = N > Mg ? N : Mg;
    hipLaunchKernelGGL(sap_score_kernel, dim3((gmax + CB - 1) / CB, (amax + SA - 1) / SA, 2 * P), dim3(256), 0, s, d0, d1, D);
    REID_CHECK_LAUNCH("reid_smooth_ap_fwd(scores)");
    const int lds = rank_lds_bytes(gmax, with_grad);
    const float inv_tau = 1.f / tau;
    if (with_grad) {
        if (lds > 65536) REID_MAX_LDS(sap_rank_kernel<true>, lds);
        hipLaunchKernelGGL(sap_rank_kernel<true>, dim3(P * (N + Mg)), dim3(256), lds, s, d0, d1, P, inv_tau);
    } else {
        if (lds > 65536) REID_MAX_LDS(sap_rank_kernel<false>, lds);
        hipLaunchKernelGGL(sap_rank_kernel<false>, dim3(P * (N + Mg)), dim3(256), lds, s, d0, d1, P, inv_tau);
    }
    REID_CHECK_LAUNCH("reid_smooth_ap_fwd(ranks)");
    hipLaunchKernelGGL(sap_finalize_kernel, dim3(P), dim3(256), 0, s, q_ap, g_ap, N, Mg, result);
    REID_CHECK_LAUNCH("reid_smooth_ap_fwd(finalize)");
    if (with_grad) {
        // in the batch form the galleries of the gather are the batch's unit rows; ring slots are read as they are
        const float* G0 = gallery_grad ? U.g : ga;
        const float* G1 = gallery_grad ? U.q : gb;
        hipLaunchKernelGGL(sap_gather_kernel, dim3(P * ((N + GO - 1) / GO + (Mg + GO - 1) / GO)), dim3(256), 4 * GO * D * sizeof(float), s, d0, d1, U,
                           G0, gallery_grad ? U.ldg : ldga, G1, gallery_grad ? U.ldq : ldgb, gallery_grad, P, N, Mg, D, normalize, eps, ws + w.inv,
                           ws + w.norm, result, ws + w.hq, ws + w.hg);
        REID_CHECK_LAUNCH("reid_smooth_ap_fwd(gather)");
    }
    return REID_OK;
}

extern "C" int reid_smooth_ap_bwd(const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg, int32_t D, const float* ws,
                                  const float* gscale, float* dq, int32_t lddq, float* dg, int32_t lddg, void* stream) {
    const char* who = "reid_smooth_ap_bwd";
    REID_CHECK_ARG(ws && gscale && dq && dg, "%s: null pointer", who);
    if (int rc = check_dims(who, P, N, Mg, D)) return rc;
    if (int rc = check_ld(who, (int64_t)P * N, D, lddq, "lddq")) return rc;
    if (int rc = check_ld(who, Mg, D, lddg, "lddg")) return rc;
    REID_CHECK_ARG(aligned16(ws) && aligned16(dq) && aligned16(dg), "%s: ws, dq or dg is not 16-byte aligned", who);
    const Ws w(P, N, Mg, D, 1, 1, 1);                                // (Hq and Hg lead the workspace whatever the galleries)
    hipLaunchKernelGGL(sap_bwd_kernel, dim3((P * N + Mg + 3) / 4), dim3(256), 0, (hipStream_t)stream, q_valid, g_valid, P, N, Mg, D, ws + w.hq,
                       ws + w.hg, gscale, dq, lddq, dg, lddg);
    REID_CHECK_LAUNCH("reid_smooth_ap_bwd");
    return REID_OK;
}
