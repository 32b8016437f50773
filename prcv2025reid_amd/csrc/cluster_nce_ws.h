// What cluster_nce.hip and hybrid_nce.hip share: the layout of the workspace reid_cluster_nce_fwd leaves behind (hybrid_nce.hip reads
// the unit rows x^ out of it) and the shape checks of their extern "C" entry points -- the ONE copy of each.
#pragma once
#include "triplet_mine.h"

namespace cnce {

constexpr int MAX_SIDES = 9;
constexpr float EPS = 1e-12f;

// ws (floats): H R D | x^ R D | used R | inv R | target cosine R | lse R | (max, sum) splits R 2 | sum_c p C splits R D
struct Ws {
    int64_t h, xhat, used, inv, tgt, lse, part, gpart, total;
    Ws(int64_t R, int64_t D, int64_t splits) {
        int64_t o = 0;
        auto take = [&](int64_t n) { const int64_t at = o; o += (n + 3) & ~(int64_t)3; return at; };
        h = take(R * D); xhat = take(R * D); used = take(R); inv = take(R); tgt = take(R); lse = take(R);
        part = take(2 * splits * R); gpart = take(splits * R * D);
        total = o;
    }
};

inline int check_d(const char* who, int32_t D) {
    REID_CHECK_ARG(D % 32 == 0 && D >= 32 && D <= 1024, "%s: D=%d (a multiple of 32, 32..1024)", who, D);
    return REID_OK;
}

inline int check_shape(const char* who, int32_t S, int32_t N, int32_t D) {
    REID_CHECK_ARG(S >= 1 && S <= MAX_SIDES, "%s: S=%d (1..9)", who, S);
    REID_CHECK_ARG(N >= 1 && N <= triplet::MAX_ROWS, "%s: N=%d (1..8192)", who, N);
    return check_d(who, D);                                          // (S N D <= 9 * 8192 * 1024 < 2^31: x^ and H [S N, D] fit)
}

inline int check_table(const char* who, int32_t K, int32_t D) {
    REID_CHECK_ARG(K >= 1, "%s: K=%d (>= 1)", who, K);
    REID_CHECK_ARG((int64_t)K * D < (1ll << 31), "%s: K * D beyond 2^31 elements", who);
    return REID_OK;
}

}  // namespace cnce
