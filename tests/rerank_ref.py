"""numpy restatement of the k-reciprocal re-ranking definition (DESIGN.md "k-reciprocal re-ranking"), in the dtype asked for, and
the seeded fixtures the re-ranking tests share.  Written from the definition, loops and sets, nothing shared with the package."""
import numpy as np


def kh_of(k1):
    return int(np.round(k1 / 2))                      # numpy rounds half to even


def ranking(S):
    """Row-wise order: score descending, index ascending on ties."""
    return np.argsort(-S, axis=1, kind='stable')


def rerank_ref(X, Nq, k1=20, k2=6, lam=0.3, dtype=np.float64, nbr=None):
    """All stages for pooled unit rows X = [Q; G].  ``nbr``: take the pooled ranking as given (the fp32 run of a test uses the fp64
    run's, so that both weigh the same sets).  Returns cos, nbr, R (the R(i, k1)), Rh (the R(i, kh)), Rstar, V, V2, s."""
    X = np.asarray(X, dtype=dtype)
    N = X.shape[0]
    kh = kh_of(k1)
    cos = X @ X.T
    d = 1 - cos
    if nbr is None:
        nbr = ranking(cos)

    def recip(i, k):
        return [int(j) for j in nbr[i, :k + 1] if i in nbr[j, :k + 1]]
    R = [recip(i, k1) for i in range(N)]
    Rh = [recip(i, kh) for i in range(N)]
    Rstar = []
    V = np.zeros((N, N), dtype)
    for i in range(N):
        members, base = list(R[i]), set(R[i])
        for j in R[i]:
            if 3 * len(base & set(Rh[j])) > 2 * len(Rh[j]):
                members += [c for c in Rh[j] if c not in members]
        Rstar.append(members)
        e = np.exp(-d[i, members])
        V[i, members] = e / e.sum(dtype=dtype)
    V2 = np.stack([V[nbr[i, :k2]].mean(0, dtype=dtype) for i in range(N)])
    s = jaccard_ref(V2[:Nq], V2[Nq:], cos[:Nq, Nq:], lam, dtype)
    return {'cos': cos, 'nbr': nbr, 'R': R, 'Rh': Rh, 'Rstar': Rstar, 'V': V, 'V2': V2, 's': s}


def jaccard_ref(A, B, cos, lam, dtype=np.float64):
    A, B, cos = (np.asarray(t, dtype=dtype) for t in (A, B, cos))
    m = np.stack([np.minimum(a[None, :], B).sum(1, dtype=dtype) for a in A])
    J = m / (2 - m)
    return (dtype(1) - dtype(lam)) * J + dtype(lam) * cos


def gate(ref64, ref32, keys=('V', 'V2', 's')):
    """Tolerance of the continuous outputs: 8 x the largest fp64-vs-fp32 difference of the reference itself, at least 4 fp32 ulps of 1."""
    worst = max(float(np.abs(ref64[k] - ref32[k].astype(np.float64)).max()) for k in keys)
    return max(8 * worst, 4 * float(np.finfo(np.float32).eps))


def min_gap_in_top(S, k):
    """Smallest difference between adjacent entries of the first k of every row's descending order."""
    top = -np.sort(-S, axis=1)[:, :k]
    return float((top[:, :-1] - top[:, 1:]).min())


def ap_cmc(s_row, g_pid, q_pid, keep):
    """(AP, rank of the first positive, #positives) of one query over the kept gallery rows, ranking as ``ranking``."""
    order = [j for j in ranking(s_row[None])[0] if keep[j]]
    hits = [r + 1 for r, j in enumerate(order) if g_pid[j] == q_pid]
    if not hits:
        return 0.0, 0, 0
    return float(np.mean([(n + 1) / r for n, r in enumerate(hits)])), hits[0], len(hits)


# ----------------------------------------------------------------------------------------------------------------- fixtures
def exact_fixture(seed=0, Nq=32, Ng=224, D=64, nid=24, flip=0.3):
    """Entries +-1/8 at D = 64: unit rows, exact in bf16 / f16 / fp32, every dot product a multiple of 1/32 -- ties everywhere."""
    rng = np.random.default_rng(seed)
    cent = rng.choice([-1.0, 1.0], size=(nid, D))
    pid = np.concatenate([np.arange(Nq) % nid, np.arange(Ng) % nid])
    X = cent[pid] * np.where(rng.random((Nq + Ng, D)) < flip, -1.0, 1.0) / 8.0
    return X, pid[:Nq], pid[Nq:]


def gaussian_fixture(seed, Nq, Ng, D, nid, noise, spread=0.0):
    """Identity centroid plus noise, normalised (fp32 values, so every run sees the same rows).  ``spread``: the noise level of a row
    is noise * U(1 - spread, 1 + spread), which widens the range of the similarities inside a neighbour list."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nid, D))
    pid = np.concatenate([rng.integers(0, nid, Nq), np.arange(Ng) % nid])
    X = noise * rng.standard_normal((Nq + Ng, D))
    if spread:
        X *= rng.uniform(1 - spread, 1 + spread, (Nq + Ng, 1))
    X += cent[pid]
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    X = (X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return X, pid[:Nq], pid[Nq:]


def sparse_rows(rng, rows, N, nnz):
    """Non-negative fp32 rows with ``nnz`` non-zeros each that sum to 1 (the shape of V2's rows)."""
    M = np.zeros((rows, N), np.float32)
    for r in range(rows):
        c = rng.choice(N, size=min(nnz, N), replace=False)
        w = rng.random(c.size) + 0.05
        M[r, c] = (w / w.sum()).astype(np.float32)
    return M
