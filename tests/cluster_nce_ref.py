"""The float64 reference of the cluster-contrast memory loss (csrc/cluster_nce.hip; include/reid_hip.h, reid_cluster_nce_*) in numpy --
loss, row losses, dx, both update modes, the centroid initialisation -- and the tolerances the GPU tests use.

The tolerances are worst-case bounds in u = 2^-24 (fp32 unit roundoff), D, K, tau and the number of rows chained into one centroid;
every constant below is a count of roundings, nothing is fitted to what the kernels give.  First-order analysis (products of two
error terms are dropped); `exact=True` is the case whose operands make every norm, dot product and logit exact (entries in {0, +-0.5,
+-1}, unit rows, 1 / tau a power of two), where only exp, log and the sums round.

  e_n(D)      relative error of an element of x^ = x * (1 / max(|x|, eps)): the sum of D squares (D u), its square root (u / 2 of half
              of it: D / 2 + 1), the reciprocal, the product -> (D / 2 + 4) u.
  e_cos(D)    x^ . C_c: an fp32 chain of D products and additions of two unit rows (D u, Cauchy-Schwarz on sum |x^_i c_i|) plus the two
              normalisations (the row's, and the centroid's, which makes |C_c| = 1 only to e_n) -> (D + 2 e_n / u) u = (2 D + 8) u.
  e_logit     e_cos / tau, plus tau as fp32, 1 / tau and the product: 3 u |l| <= 3 u / tau.
  merges(K)   how many (max, sum) merges a term of sum_c exp(l_c - max) can pass through: the class tiles one workgroup may walk
              (ceil(K / 64)), 5 butterfly levels, the two waves of a row, at most 64 splits.
  e_merge     one merge: exp (libm: 1 ulp, taken as 2 u) of a difference of two logits (|.| <= 2 / tau, rounded: 2 u / tau relative to the
              exp), a product and an addition -> (4 + 2 / tau) u relative to the (all positive) sum.
  e_lse       e_logit (lse is 1-Lipschitz in the largest logit error) + merges * e_merge + log (u (1 + log K)) + the final addition
              (u (1 / tau + log K)).
  e_row       lse - l_y: e_lse + e_logit + the subtraction u (|lse| + |l_y|) <= u (3 / tau + log K).
  e_loss      the used rows' mean in fp64 rounded once: e_row + u (2 / tau + log K).
"""
import math

import numpy as np

U = 2.0 ** -24
EPS = 1e-12
CLASS_TILE = 64
MAX_SPLITS = 64


def e_n(D, exact=False):
    return 0.0 if exact else (D / 2 + 4) * U


def e_logit(D, tau, exact=False):
    return 0.0 if exact else ((2 * D + 8) * U + 3 * U) / tau


def merges(K):
    return math.ceil(K / CLASS_TILE) + 5 + 1 + MAX_SPLITS


def e_merge(tau, exact=False):
    return (4 + (0 if exact else 2 / tau)) * U


def e_lse(D, K, tau, exact=False):
    return e_logit(D, tau, exact) + merges(K) * e_merge(tau, exact) + U * (1 + math.log(K)) + U * (1 / tau + math.log(K))


def row_bound(D, K, tau, exact=False):
    return e_lse(D, K, tau, exact) + e_logit(D, tau, exact) + U * (3 / tau + math.log(K))


def loss_bound(D, K, tau, exact=False):
    return row_bound(D, K, tau, exact) + U * (2 / tau + math.log(K))


def cos_bound(D, exact=False):
    return 0.0 if exact else (2 * D + 8) * U


def dx_bound(f, D, K, tau, dloss, cmax, exact=False):
    """Per-row absolute bound [R] of an element of dx = coef * H, H = (G - x^ (x^ . G)) / max(|x|, eps), G = (sum_c p_c C_c - C_y) / tau:
      eps_p   relative error of p_c = exp(l_c - lse): the exponent's (e_logit + e_lse + its subtraction u) plus exp's 2 u;
      A = sum_c p_c C_c on the matrix cores: a chain of at most K + 64 + 64 additions (the padded last tile, the splits), every term
              below cmax = max |C_cd| -> per element eps_p cmax + (K + 128) u cmax; in the 2-norm eps_p (|C_c| = 1) + sqrt(D) (K + 128) u cmax;
      G       (A - C_y) * (1 / tau): the subtraction, 1 / tau and the product: 6 u / tau of elements below 2;
      dot     x^ . G <= |dG|_2 + (e_n + (D + 1) u) |G|_2, |G|_2 <= 2 / tau;
      H       G_i - x^_i dot, times 1 / max(|x|, eps), times coef (a division and a product): with xmax = max_i |x^_i| of the row,
              |G_i| and |dot| <= 2 / tau, |G_i - x^_i dot| <= 4 / tau."""
    en = e_n(D, exact)
    eps_p = e_logit(D, tau, exact) + e_lse(D, K, tau, exact) + 3 * U
    chain = (K + 128) * U * cmax
    eG_el = (eps_p * cmax + chain + 6 * U) / tau
    eG_2 = (eps_p + math.sqrt(D) * (chain + 6 * U)) / tau
    e_dot = eG_2 + (en + (D + 1) * U) * 2 / tau
    xmax = np.abs(f['xhat']).max(axis=1)
    eH = eG_el + xmax * e_dot + (en + 4 * U) * 2 / tau
    coef = abs(dloss) / max(1, f['n_used'])
    return coef * f['inv'] * (eH + (4 / tau) * (en + 4 * U))


def unit_rows(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    return x / np.maximum(n, EPS), 1.0 / np.maximum(n[..., 0], EPS)


def forward(x, labels, valid, table, tau, dloss=1.0):
    """x [S, N, D], labels [N], valid [S, N] or None, table [K, D] (any float arrays).  Everything in float64: used [R], xhat [R, D],
    inv [R], row_loss / target_cos [R] (unused rows 0), loss, n_used, dx [R, D] for the upstream gradient dloss."""
    x = np.asarray(x, dtype=np.float64)
    S, N, D = x.shape
    C = np.asarray(table, dtype=np.float64)
    K = C.shape[0]
    y = np.tile(np.asarray(labels, dtype=np.int64), S)
    v = np.ones(S * N, dtype=bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    used = v & (y >= 0) & (y < K)
    xhat, inv = unit_rows(x.reshape(S * N, D))
    with np.errstate(invalid='ignore', over='ignore'):
        l = xhat @ C.T / tau
        m = np.nanmax(np.where(np.isnan(l), -np.inf, l), axis=1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(l - m)
        lse = m[:, 0] + np.log(e.sum(axis=1))
        p = e / e.sum(axis=1, keepdims=True)
    yc = np.where(used, y, 0)
    tcos = np.where(used, (xhat * C[yc]).sum(axis=1), 0.0)
    row_loss = np.where(used, lse - tcos / tau, 0.0)
    n_used = int(used.sum())
    loss = float(row_loss[used].sum() / max(1, n_used))
    G = (p @ C - C[yc]) / tau
    H = (G - xhat * (xhat * G).sum(axis=1, keepdims=True)) * inv[:, None]
    dx = np.where(used[:, None], dloss / max(1, n_used) * H, 0.0)
    return dict(used=used, y=y, xhat=xhat, inv=inv, row_loss=row_loss, target_cos=tcos, loss=loss, n_used=n_used, dx=dx, lse=lse)


def contributing(f):
    return f['used'] & np.isfinite(f['row_loss'])


def update(table, f, momentum, mode, D=None, exact=False, err0=None, xhat_dev=0.0):
    """The table after the update of the forward ``f`` (float64) and err [K]: the 2-norm bound of every centroid's deviation.  Per blend
    c' = normalise(m c + (1 - m) x^): the incoming deviation is scaled by m / nu (nu = |m c + (1 - m) x^|, the normalisation's Jacobian
    is 1 / nu), the blend adds (e_n + 4 u) / nu (x^'s error, 1 - m, two products and a sum of vectors of norm <= 1) and the
    normalisation e_n + u of a unit vector -- so the bound grows linearly with the rows applied to the centroid (times m / nu <= 1 for
    the blends the tests make).  ``err0`` [K]: the deviation the centroids start with, ``xhat_dev``: the 2-norm by which the unit rows
    of the form under test may differ from the reference's (a chained comparison: both 0 for one step from the same state)."""
    C = np.array(table, dtype=np.float64)
    D = C.shape[1] if D is None else D
    err = np.zeros(C.shape[0]) if err0 is None else np.array(err0, dtype=np.float64)
    con = contributing(f)
    en = e_n(D, exact)
    for k in sorted(set(f['y'][con].tolist())):
        rows = [r for r in range(len(con)) if con[r] and f['y'][r] == k]
        if mode == 'hard':
            best = rows[0]
            for r in rows[1:]:
                if f['target_cos'][r] < f['target_cos'][best]:
                    best = r
            rows = [best]
        for r in rows:
            c = momentum * C[k] + (1 - momentum) * f['xhat'][r]
            nu = math.sqrt(float((c * c).sum()))
            C[k] = c / max(nu, EPS)
            err[k] = (momentum * err[k] + (1 - momentum) * xhat_dev + (en + 4 * U)) / max(nu, EPS) + (D / 2 + 4) * U + U
    return C, err


def literal_update(table, f, momentum):
    """Cluster-Contrast's sequential loop, literally: every contributing row in ascending row order blends into its centroid."""
    C = np.array(table, dtype=np.float64)
    con = contributing(f)
    for r in range(len(con)):
        if con[r]:
            k = f['y'][r]
            C[k] = momentum * C[k] + (1 - momentum) * f['xhat'][r]
            C[k] = C[k] / max(np.linalg.norm(C[k]), EPS)
    return C


def hard_pick_gap(f):
    """The smallest gap between the two smallest target cosines of a label with two or more contributing rows (inf when there is none):
    a 'hard' test case must keep it above 2 * cos_bound(D), or the pick is not determined by the inputs."""
    con = contributing(f)
    gap = math.inf
    for k in set(f['y'][con].tolist()):
        t = np.sort(f['target_cos'][con & (f['y'] == k)])
        if len(t) >= 2:
            gap = min(gap, float(t[1] - t[0]))
    return gap


def centroids(feats, labels):
    """([K, D] float64: the normalised mean of the rows with label k (labels of -1 skipped), K = max + 1; err [K]: the 2-norm bound of
    the fp32 form).  An empty cluster raises.  The fp32 sum of n rows in any order is off by at most (n - 1) u sum_r |x_r| in the
    2-norm, the division by n adds u |mean|; an error d of the mean moves the unit centroid by at most d / |mean|; the normalisation
    of the mean adds its e_n + u (the square root's input is exact here only to D u, as for x^)."""
    feats = np.asarray(feats, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    K, D = int(labels.max()) + 1, feats.shape[1]
    out, err = np.zeros((K, D)), np.zeros(K)
    for k in range(K):
        rows = feats[labels == k]
        n = len(rows)
        if n == 0:
            raise ValueError(f'cluster {k} has no row')
        mean = rows.sum(axis=0) / n
        nm = max(np.linalg.norm(mean), EPS)
        out[k] = mean / nm
        err[k] = ((n - 1) * U * np.linalg.norm(rows, axis=1).sum() / n + U * nm) / nm + (D / 2 + 4) * U + U
    return out, err


# ---------------------------------------------------------------------------------------------------------------- cases
def make_case(S, N, D, K, seed, noise=True, spread=0.5):
    """x [S, N, D] fp32 around the centroids of their labels, labels [N] (with -1 and K among them when noise), valid [S, N] uint8 (some
    zeros when S * N >= 5), table [K, D] fp32 unit rows."""
    g = np.random.default_rng(seed)
    table = g.standard_normal((K, D))
    table = (table / np.linalg.norm(table, axis=1, keepdims=True)).astype(np.float32)
    labels = g.integers(0, K, size=N).astype(np.int64)
    if noise and N >= 5:
        labels[1] = -1
        labels[N - 2] = K
    x = table[np.clip(labels, 0, K - 1)][None] * g.uniform(0.5, 3.0, size=(S, N, 1)) + spread * g.standard_normal((S, N, D)) / math.sqrt(D)
    valid = np.ones((S, N), dtype=np.uint8)
    if S * N >= 5:
        valid.reshape(-1)[2::7] = 0
    return x.astype(np.float32), labels, valid, table


def random_case(S, N, D, K, seed):
    """As make_case, but the rows are random directions (norms 0.5 .. 3) unrelated to their labels: the logits of a row are then of one
    size, its loss is about log K or more and its gradient large -- both orders of magnitude above the bounds, so that a comparison
    within the bounds says something (a row next to its centroid has p_y = 1 to the last bit: loss and gradient vanish)."""
    _, labels, valid, table = make_case(S, N, D, K, seed)
    g = np.random.default_rng(seed + 1)
    x = g.standard_normal((S, N, D)) * g.uniform(0.5, 3.0, size=(S, N, 1))
    return x.astype(np.float32), labels, valid, table


def signal_ratios(f, D, K, tau, dloss, cmax):
    """(largest row loss / row_bound, largest over the rows of max |dx| / dx_bound) of a reference forward: how far the quantities a
    test compares stand above the tolerance it compares them with."""
    u = f['used']
    b = dx_bound(f, D, K, tau, dloss, cmax)
    return float(f['row_loss'][u].max() / row_bound(D, K, tau)), float((np.abs(f['dx'][u] * dloss).max(axis=1) / b[u]).max())


def exact_case(N, D, K, seed):
    """Rows and centroids with entries in {0, +-0.5, +-1} that are exactly unit (one +-1, or four +-0.5): every norm and dot product is
    exact in fp32; with tau = 1 / 16 the logits are too."""
    g = np.random.default_rng(seed)

    def rows(n):
        out = np.zeros((n, D), dtype=np.float32)
        for r in range(n):
            if g.random() < 0.3:
                out[r, g.integers(0, D)] = g.choice([-1.0, 1.0])
            else:
                out[r, g.choice(D, size=4, replace=False)] = g.choice([-0.5, 0.5], size=4)
        return out
    return rows(N)[None], g.integers(0, K, size=N).astype(np.int64), rows(K)
