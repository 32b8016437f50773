"""Host restatement of reid_expand_rows (include/reid_hip.h): a float32 numpy loop that follows the definition literally, and an
independent float64 formula with the allowance of the float32 evaluation (checked against each other by test_expansion_cpu.py;
test_expansion_gpu.py compares the kernel with the loop bit for bit).  Device-agnostic numpy."""
import numpy as np

U32 = 2.0 ** -24


def weight_ref(s, alpha):
    """The definition's weight of a score (np.float32): 1 for alpha = 0, else max(s, 0) raised by alpha - 1 float32 products."""
    if alpha == 0:
        return np.float32(1.0)
    p = s if s > 0 else np.float32(0.0)
    w = p
    for _ in range(alpha - 1):
        w = np.float32(w * p)
    return w


def expand_rows_ref(x, table, nbr, score, k, alpha, self_base=-1):
    """raw f32 [rows, D]: x[i] plus w * table[nbr] of the first k eligible entries of row i's list, multiply then add in list order.
    An entry is eligible when 0 <= nbr < M, its score is not NaN and nbr != self_base + i (self_base >= 0); an eligible entry counts
    towards k whatever its weight, and is added only when the weight is not zero."""
    x = np.ascontiguousarray(x, np.float32)
    table = np.asarray(table, np.float32)
    score = np.asarray(score, np.float32)
    M = table.shape[0]
    lists = np.asarray(nbr).tolist()
    raw = np.empty_like(x)
    for i, row in enumerate(lists):
        acc = x[i].copy()
        n_elig = 0
        for t, j in enumerate(row):
            s = score[i, t]
            if not 0 <= j < M or s != s or (self_base >= 0 and j == self_base + i):
                continue
            if n_elig == k:
                break
            n_elig += 1
            w = weight_ref(s, alpha)
            if w == 0:
                continue
            acc = acc + w * table[j]          # float32 array arithmetic: the product is rounded, then the sum
        raw[i] = acc
    return raw


def expand_rows_f64(x, table, nbr, score, k, alpha, self_base=-1):
    """(raw f64 [rows, D], allow [rows, D]): x + sum w F with w = max(score, 0) ** alpha from np.power in float64 over the entries a
    vectorised restatement of the selection rule keeps (no loop shared with expand_rows_ref).
    Allowance of the float32 loop, u = 2^-24 per operation: a weight is alpha - 1 products, the term one more, and a term passes through
    at most n_used additions, so per element ((alpha - 1) + 1 + n_used) u sum|w F|; x[i] passes through the same n_used additions
    (every partial sum holds it): n_used u |x|; plus one u |raw| for the second order."""
    x = np.asarray(x, np.float64)
    table = np.asarray(table, np.float64)
    nbr = np.asarray(nbr, np.int64)
    score = np.asarray(score)
    rows, M = x.shape[0], table.shape[0]
    elig = (nbr >= 0) & (nbr < M) & ~np.isnan(score)
    if self_base >= 0:
        elig &= nbr != (self_base + np.arange(rows))[:, None]
    used = elig & (np.cumsum(elig, 1) <= k)
    w = np.where(used, np.power(np.maximum(np.nan_to_num(score.astype(np.float64)), 0.0), alpha), 0.0)
    F = table[np.clip(nbr, 0, M - 1)]                                   # [rows, kl, D]; unused entries carry w = 0
    raw = x + np.einsum('rt,rtd->rd', w, F)
    n_used = (w != 0).sum(1)[:, None]
    allow = (max(alpha - 1, 0) + 1 + n_used) * U32 * np.einsum('rt,rtd->rd', w, np.abs(F)) + n_used * U32 * np.abs(x) + U32 * np.abs(raw)
    return raw, allow


SPECIAL_SCORES = np.array([np.nan, -0.25, 0.0, -0.0, 1e-40, 1.0 + 2.0 ** -23], np.float32)


def random_lists(rng, rows, kl, M, self_base=-1, special=0.35):
    """(nbr i32 [rows, kl], score f32 [rows, kl]): distinct indices per row with scores descending in (0, 1], then the special entries
    of the hand cases at random positions: index -1, indices >= M, the row's own index (self_base >= 0), and NaN, negative, zero,
    subnormal and 1 + 2^-23 scores."""
    nbr = np.empty((rows, kl), np.int32)
    for i in range(rows):
        nbr[i] = rng.permutation(max(M, kl))[:kl] if M >= kl else rng.integers(0, M, kl)
    score = np.sort(rng.random((rows, kl)).astype(np.float32), 1)[:, ::-1].copy()
    where = rng.random((rows, kl)) < special
    kind = rng.integers(0, 4, (rows, kl))
    nbr[where & (kind == 0)] = -1
    nbr[where & (kind == 1)] = M + rng.integers(0, 3)
    if self_base >= 0:
        own = np.broadcast_to((self_base + np.arange(rows))[:, None], (rows, kl))
        sel = where & (kind == 2)
        nbr[sel] = own[sel].astype(np.int32)
    sel = where & (kind == 3)
    score[sel] = SPECIAL_SCORES[rng.integers(0, len(SPECIAL_SCORES), int(sel.sum()))]
    return nbr, score
