// What the triplet losses share (triplet.hip: one set of rows against itself; cross_triplet.hip: one set against another;
// hc_triplet.hip: a set of per-identity centres against itself; xbm.hip: one set against the slots of a cross-batch memory) and what
// center.hip takes of it -- the ONE copy of each piece, all fp32 unless said; on the right, who calls it:
//   Rows, mine_tile                   the mining loop                              triplet_fwd_kernel, xt_fwd_kernel, hc_mine_kernel,
//                                                                                  xbm_mine_kernel
//   row_loss_of, row_dloss_of         the row-loss forms                           mine_tile, add_own, add_chosen_by, the refine kernels,
//                                                                                  xbm_bwd_kernel
//   Sides                             the two sides as a kernel parameter          cross_triplet.hip, hc_triplet.hip, xbm.hip
//   unit_row                          the unit row of one row                      xt_unit_kernel, hc_unit_kernel, xbm_unit_kernel,
//                                                                                  xbm_enqueue_kernel
//   refine_anchor                     the kept distances re-evaluated in fp64      xt_refine_kernel, hc_refine_kernel, xbm_refine_kernel
//   load_row, zero_acc, store_row     a row as NV 16-byte chunks per lane          triplet_bwd_kernel, xt_bwd_kernel, hc_centre_kernel,
//                                                                                  hc_bwd_centre_kernel, hc_bwd_rows_kernel; xbm_enqueue_kernel,
//                                                                                  xbm_refine_kernel, xbm_bwd_kernel; center_fwd_kernel,
//                                                                                  center_update_kernel, center_bwd_kernel
//   add_term, term_scale              the gather-form backward, one term           add_own, add_chosen_by; xbm_bwd_kernel (its chosen rows
//                                                                                  are the two copies its forward kept, not rows by index)
//   add_own, add_chosen_by            the gather-form backward, an anchor's terms  triplet_bwd_kernel, xt_bwd_kernel, hc_bwd_centre_kernel
//   check_d, check_dims, check_ld, check_scalars, aligned16   the argument checks  the extern "C" entry points of triplet.hip,
//                                                                                  cross_triplet.hip, hc_triplet.hip and xbm.hip;
//                                                                                  center.hip's take check_d, check_ld and aligned16
// Shared forms of the four-line bodies of the unit kernels, of the projection through the normalisation (xt_bwd_kernel,
// hc_bwd_rows_kernel) and of the finalize kernels' ordered fp64 tails changed the machine code of their callers, so those stay written
// out in the .hip files, each copy naming the other (profiles/triplet_shared_isa_identity.md, "Left duplicated").
//
//   d2(i,j) = sum_c (x_ic - y_jc)^2   -- the DIFFERENCE form on the vector ALU (the features are mostly a common
//   mean, the Gram form loses more of d2 than the gap between the hardest and the second-hardest candidate).
//
// mine_tile: a workgroup of 256 threads owns TA = 4 anchors.  Its four waves walk the candidate rows 256 at a time, ONE CANDIDATE PER
//   LANE: a [256][32]-float piece of the candidates is staged once per workgroup in LDS (16-byte global reads into registers while the
//   previous piece is computed; rows padded by 16 bytes so that the per-lane ds_read_b128 of "my row" is conflict free) and shared by
//   the tile's anchors, whose columns sit beside them and are read as LDS broadcasts (as scalar loads they cost a scalar-cache round
//   trip per 16 bytes: 16 serial waits per piece).  Every lane keeps four partial sums per anchor (one per column mod 4): a chain of
//   D / 4 additions, well inside the D * 2^-24 bound, and the same instruction sequence for every (i, j) -- equal rows give bit-equal
//   d2.  Each lane keeps a running (key, index) best per anchor under the tie rule of rank.h (key descending, index ascending; the key
//   is d2 for the hardest positive and -d2 for the hardest negative, so equal d2 go to the lowest index for both); the lanes are merged
//   by ranking::wave_best, the four waves through LDS.  (lds_tile.h's staging helpers build 128-byte-row swizzled 16-bit tiles for
//   MFMA fragments; a padded fp32 image read row-per-lane is a different layout, so they are not used here.)
#pragma once
#include "rank.h"

namespace {

// The two sides of cross_triplet.hip and hc_triplet.hip as their kernels see them: unit rows in ws (normalize = 1) or the callers'
// rows.  A kernel parameter type, so its namespace is part of those kernels' symbols: it stays in the unnamed one, where the two
// files had it, and the symbols stay what they were.
struct Sides {
    const float* q; int ldq;
    const float* g; int ldg;
};

}  // namespace

namespace triplet {

constexpr int TA = 4;                    // anchors per workgroup
constexpr int DK = 32;                   // columns per staged piece
constexpr int PITCH = DK + 4;            // padded LDS row (floats)
constexpr int CB = 256;                  // candidates per piece: one per thread
constexpr float D2_MIN = 1e-12f;         // clamp(min=1e-12).sqrt()
// "no candidate yet": ranks behind every real index at an equal key, so a candidate whose d2 overflowed to +inf (key -inf for a
// negative) is still taken when it is the only one
constexpr int NONE = 0x7fffffff;
constexpr int NO_SELF = -0x40000000;     // mine_tile's excl0 when no candidate is the anchor itself
constexpr int NV = 4;                    // 16-byte chunks per lane where one wave owns a row: D <= 64 * 4 * NV = 1024
constexpr int MAX_D = 64 * 4 * NV;
constexpr int MAX_ROWS = 8192;           // rows per side

// l = max(0, z + margin) (margin >= 0) or softplus(z) (margin < 0), z = d_ap - d_an; dl = its derivative
__device__ __forceinline__ float row_loss_of(float z, float margin) {
    if (margin >= 0.f) return fmaxf(z + margin, 0.f);
    return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
}
__device__ __forceinline__ float row_dloss_of(float z, float margin) {
    if (margin >= 0.f) return z + margin > 0.f ? 1.f : 0.f;
    const float e = expf(-fabsf(z));
    return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// one side of the mining: rows x [rows, ld], their labels, and which of them take part (NULL: all)
struct Rows {
    const float* x;
    int ld;
    const int64_t* labels;
    const uint8_t* valid;
    int rows;
};

// Anchors a0 .. a0 + TA - 1 of A against every candidate of C, by the whole workgroup.  Candidate excl0 + a is skipped as a positive
// of anchor a0 + a (the anchor itself when A and C are the same rows: excl0 = a0; NO_SELF otherwise).  Thread t < TA writes the five
// outputs of anchor a0 + t.
__device__ __forceinline__ void mine_tile(const Rows A, const Rows C, int a0, int excl0, int D, float margin, float* __restrict__ d_ap,
                                          float* __restrict__ d_an, int* __restrict__ idx_p, int* __restrict__ idx_n,
                                          float* __restrict__ row_loss) {
    __shared__ __attribute__((aligned(16))) float cand[CB * PITCH];
    __shared__ __attribute__((aligned(16))) float anch[TA * DK];
    __shared__ float m_key[4][TA][2];
    __shared__ int m_idx[4][TA][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float bp[TA], bn[TA];
    int ip[TA], in[TA];
#pragma unroll
    for (int a = 0; a < TA; ++a) { bp[a] = -1.f; ip[a] = NONE; bn[a] = -INFINITY; in[a] = NONE; }
    int64_t alab[TA];                    // the anchors' labels, read once
#pragma unroll
    for (int a = 0; a < TA; ++a) alab[a] = A.labels[min(a0 + a, A.rows - 1)];

    // One piece = DK columns of CB candidates.  The next piece travels global -> registers while this one is computed from LDS.
    // (columns past D are staged as zeros on both sides: they add exactly 0 to every sum, and the inner loop has one shape)
    constexpr int NST = CB * (DK / 4) / 256;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 stage[NST], astage = zero4;
#pragma unroll
    for (int u = 0; u < NST; ++u) stage[u] = zero4;
    auto fetch = [&](int c0, int k0) {
        const int nc4 = min(DK / 4, (D - k0) >> 2);                  // 16-byte chunks of this piece
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int e = tid + 256 * u, r = e >> 3, c4 = e & 7;
            if (c0 + (r & ~63) < C.rows) stage[u] = c4 < nc4 ? *(const f32x4*)(C.x + min(c0 + r, C.rows - 1) * C.ld + k0 + 4 * c4) : zero4;
        }
        if (tid < TA * (DK / 4))                                     // the anchors' columns (rows past the end: clamped, dropped later)
            astage = (tid & 7) < nc4 ? *(const f32x4*)(A.x + min(a0 + (tid >> 3), A.rows - 1) * A.ld + k0 + 4 * (tid & 7)) : zero4;
    };
    float acc[TA][4];
#pragma unroll
    for (int a = 0; a < TA; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.f;
    int c0 = 0, k0 = 0;
    fetch(0, 0);
    for (;;) {
        __syncthreads();                                             // the previous piece has been read
#pragma unroll
        for (int u = 0; u < NST; ++u) {                              // (slots fetch() skipped hold stale values nobody reads)
            const int e = tid + 256 * u;
            *(f32x4*)(cand + (e >> 3) * PITCH + 4 * (e & 7)) = stage[u];
        }
        if (tid < TA * (DK / 4)) *(f32x4*)(anch + 4 * tid) = astage;
        __syncthreads();
        int c0n = c0, k0n = k0 + DK;
        if (k0n >= D) { k0n = 0; c0n += CB; }
        const bool more = c0n < C.rows;
        if (more) fetch(c0n, k0n);
        if (c0 + wave * 64 < C.rows) {                               // uniform: this wave has at least one real candidate
#pragma unroll
            for (int c4 = 0; c4 < DK / 4; ++c4) {
                const f32x4 y = *(const f32x4*)(cand + tid * PITCH + 4 * c4);
#pragma unroll
                for (int a = 0; a < TA; ++a) {
                    const f32x4 xa = *(const f32x4*)(anch + a * DK + 4 * c4);      // one address per wave: an LDS broadcast
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = xa[e] - y[e];
                        acc[a][e] = fmaf(d, d, acc[a][e]);
                    }
                }
            }
        }
        if (k0n == 0) {                                              // all columns of these candidates are in
            const int j = c0 + tid;
            if (j < C.rows && (!C.valid || C.valid[j])) {
                const int64_t lj = C.labels[j];
#pragma unroll
                for (int a = 0; a < TA; ++a) {
                    const float d2 = (acc[a][0] + acc[a][1]) + (acc[a][2] + acc[a][3]);
                    if (lj == alab[a]) {
                        if (j != excl0 + a && ranking::ranks_before(d2, j, bp[a], ip[a])) { bp[a] = d2; ip[a] = j; }
                    } else if (ranking::ranks_before(-d2, j, bn[a], in[a])) { bn[a] = -d2; in[a] = j; }
                }
            }
#pragma unroll
            for (int a = 0; a < TA; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.f;
        }
        if (!more) break;
        c0 = c0n; k0 = k0n;
    }
#pragma unroll
    for (int a = 0; a < TA; ++a) {
        ranking::wave_best(bp[a], ip[a]);
        ranking::wave_best(bn[a], in[a]);
        if (lane == 0) {
            m_key[wave][a][0] = bp[a]; m_idx[wave][a][0] = ip[a];
            m_key[wave][a][1] = bn[a]; m_idx[wave][a][1] = in[a];
        }
    }
    __syncthreads();
    if (tid < TA && a0 + tid < A.rows) {
        const int i = a0 + tid;
        float kp = m_key[0][tid][0], kn = m_key[0][tid][1];
        int jp = m_idx[0][tid][0], jn = m_idx[0][tid][1];
        for (int w = 1; w < 4; ++w) {
            if (ranking::ranks_before(m_key[w][tid][0], m_idx[w][tid][0], kp, jp)) { kp = m_key[w][tid][0]; jp = m_idx[w][tid][0]; }
            if (ranking::ranks_before(m_key[w][tid][1], m_idx[w][tid][1], kn, jn)) { kn = m_key[w][tid][1]; jn = m_idx[w][tid][1]; }
        }
        const bool active = (!A.valid || A.valid[i]) && jp != NONE && jn != NONE;
        const float dp = active ? sqrtf(fmaxf(kp, D2_MIN)) : 0.f;
        const float dn = active ? sqrtf(fmaxf(-kn, D2_MIN)) : 0.f;
        d_ap[i] = dp; d_an[i] = dn;
        idx_p[i] = active ? jp : -1; idx_n[i] = active ? jn : -1;
        row_loss[i] = active ? row_loss_of(dp - dn, margin) : 0.f;
    }
}

// One wave: the unit row x * (1 / max(|x|, eps)) of x [D] into unit [D], with 1 / max(|x|, eps) and |x| beside it -- the body of
// rowops.hip's l2norm_kernel (per-lane partial sums in the same order, wave_sum, sqrtf, one division, one product), so bit-equal rows
// give bit-equal unit rows.
__device__ __forceinline__ void unit_row(const float* __restrict__ x, int D, float eps, float* __restrict__ unit, float* __restrict__ inv_out,
                                         float* __restrict__ norm_out, int lane) {
    const int nv = D >> 2;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + i * 64;
        v[i] = c < nv ? *(const f32x4*)(x + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
    const float norm = sqrtf(wave_sum(s));
    const float inv = 1.f / fmaxf(norm, eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) *(f32x4*)(unit + c * 4) = v[i] * inv;
    }
    if (lane == 0) { *inv_out = inv; *norm_out = norm; }
}

// One wave: the two distances an anchor keeps -- from its row xa to rows jp and jn of xc (leading dimension ldc), D columns -- re-
// evaluated with an fp64 sum, rounded once and clamped as the mining clamps; LANE 0 gets them, the other lanes' d_ap / d_an are left
// alone.  Mining compares the fp32 d2 (a D-term sum: a few u on d); but l'(d_ap - d_an) of the backward inherits the ABSOLUTE error
// of the saved distances, and with unnormalised rows at d = 40 those few u are already 1e-5 of the soft margin's gradient.  (3 rows
// per anchor: next to nothing beside the mining.)
__device__ __forceinline__ void refine_anchor(const float* xa, const float* xc, int ldc, int jp, int jn, int D, int lane, float& d_ap,
                                              float& d_an) {
    double sp = 0.0, sn = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = 4 * lane + 256 * v;
        if (c < D) {
            const f32x4 x = *(const f32x4*)(xa + c), p = *(const f32x4*)(xc + (size_t)jp * ldc + c), n = *(const f32x4*)(xc + (size_t)jn * ldc + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double up = (double)x[e] - (double)p[e], un = (double)x[e] - (double)n[e];
                sp = fma(up, up, sp); sn = fma(un, un, sn);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sn += __shfl_xor(sn, o, 64); }
    if (lane == 0) { d_ap = sqrtf(fmaxf((float)sp, D2_MIN)); d_an = sqrtf(fmaxf((float)sn, D2_MIN)); }
}

// A row of D columns held by one wave as NV 16-byte chunks per lane (zeros past D): load it (on = false: zeros), zero it, store it.
__device__ __forceinline__ void load_row(f32x4 (&xi)[NV], const float* __restrict__ xr, int lane, int D, bool on = true) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = 4 * lane + 256 * v;
        xi[v] = c < D && on ? *(const f32x4*)(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void store_row(float* __restrict__ o, const f32x4 (&acc)[NV], int lane, int D) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = 4 * lane + 256 * v;
        if (c < D) *(f32x4*)(o + c) = acc[v];
    }
}

// acc += s * (x_i - x_a) over this lane's columns
__device__ __forceinline__ void add_term(f32x4 (&acc)[NV], const f32x4 (&xi)[NV], const float* __restrict__ xa, float s, int lane, int D) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = 4 * lane + 256 * v;
        if (c < D) {
            const f32x4 y = *(const f32x4*)(xa + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[v][e] = fmaf(s, xi[v][e] - y[e], acc[v][e]);
        }
    }
}

// c_a / d of one saved distance; 0 for a clamped distance (d2 <= 1e-12: the saved d is the clamp value itself)
__device__ __forceinline__ float term_scale(float c, float d) { return d > sqrtf(D2_MIN) ? c / d : 0.f; }

// The two terms of row `me` (its row xi in registers) as anchor `a` of a direction whose chosen rows live in xo (leading dimension
// ldo, no rows).  Called by a whole wave.
__device__ __forceinline__ void add_own(f32x4 (&acc)[NV], const f32x4 (&xi)[NV], int a, const float* __restrict__ xo, int ldo, int no,
                                        const int* __restrict__ idx_p, const int* __restrict__ idx_n, const float* __restrict__ d_ap,
                                        const float* __restrict__ d_an, float cn, float margin, int lane, int D) {
    const int jp = idx_p[a], jn = idx_n[a];
    if (jp >= 0 && jp < no && jn >= 0 && jn < no) {
        const float dp = d_ap[a], dn = d_an[a];
        const float c = cn * row_dloss_of(dp - dn, margin);
        add_term(acc, xi, xo + (size_t)jp * ldo, term_scale(c, dp), lane, D);
        add_term(acc, xi, xo + (size_t)jn * ldo, -term_scale(c, dn), lane, D);
    }
}

// The terms of the gather form that come from OTHER rows' choices: every anchor a of [0, n) in ascending order whose idx_p[a] or
// idx_n[a] is `me` adds cn * l'(a) * (+-1 / d) * (x_me - x_a), x_a = row a of xa (leading dimension lda).  Called by a whole wave.
__device__ __forceinline__ void add_chosen_by(f32x4 (&acc)[NV], const f32x4 (&xi)[NV], int me, const float* __restrict__ xa, int lda, int n,
                                              const int* __restrict__ idx_p, const int* __restrict__ idx_n, const float* __restrict__ d_ap,
                                              const float* __restrict__ d_an, float cn, float margin, int lane, int D) {
    for (int b = 0; b < n; b += 64) {
        const int a = b + lane;
        const int pa = a < n ? idx_p[a] : -1, na = a < n ? idx_n[a] : -1;
        unsigned long long hit = __ballot(pa == me || na == me);
        while (hit) {
            const int l = __builtin_ctzll(hit);
            hit &= hit - 1;
            const int aa = b + l;
            const bool pos = __shfl(pa, l, 64) == me;
            const float dp = d_ap[aa], dn = d_an[aa];
            const float c = cn * row_dloss_of(dp - dn, margin);
            add_term(acc, xi, xa + (size_t)aa * lda, pos ? term_scale(c, dp) : -term_scale(c, dn), lane, D);
        }
    }
}

// ---- host side: the argument checks of the extern "C" entry points (`who` = the entry point's name)
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static_assert(MAX_D == 1024 && MAX_ROWS == 8192, "the limits are spelled out in the messages below");
inline int check_d(const char* who, int32_t D) {
    REID_CHECK_ARG(D % 4 == 0 && D >= 4 && D <= MAX_D, "%s: D=%d (a multiple of 4, 4..1024)", who, D);
    return REID_OK;
}
inline int check_dims(const char* who, int32_t P, int32_t N, int32_t Mg, int32_t D) {
    REID_CHECK_ARG(P >= 1 && P <= 8, "%s: P=%d (1..8)", who, P);
    REID_CHECK_ARG(N >= 1 && N <= MAX_ROWS, "%s: N=%d (1..8192)", who, N);
    REID_CHECK_ARG(Mg >= 1 && Mg <= MAX_ROWS, "%s: Mg=%d (1..8192)", who, Mg);
    return check_d(who, D);
}
inline int check_ld(const char* who, int64_t rows, int32_t D, int32_t ld, const char* ld_name) {
    REID_CHECK_ARG(ld >= D && ld % 4 == 0, "%s: %s=%d (a multiple of 4, >= D=%d)", who, ld_name, ld, D);
    REID_CHECK_ARG(rows * ld < (1ll << 31), "%s: rows * %s beyond 2^31 elements", who, ld_name);
    return REID_OK;
}
inline int check_scalars(const char* who, float margin, int32_t normalize, float eps) {
    REID_CHECK_ARG(margin == margin, "%s: margin is NaN", who);
    REID_CHECK_ARG(normalize == 0 || normalize == 1, "%s: normalize=%d (0 or 1)", who, normalize);
    REID_CHECK_ARG(eps >= 0.f, "%s: eps=%g (>= 0)", who, (double)eps);
    return REID_OK;
}

}  // namespace triplet
