"""List / dictionary restatement of steps 2-6 of the k-reciprocal re-ranking definition (DESIGN.md "k-reciprocal re-ranking") that
takes the pooled kNN lists as given and never forms an N x N array: R* from the lists, V rows as {column: value} from single dot
products, V2 rows by merging, m through an inverted dictionary of the gallery rows.  In the dtype asked for, like rerank_ref; written
from the definition, nothing shared with the package."""
import numpy as np

from rerank_ref import kh_of


def reciprocal_sets(nbr, k):
    """R(i, k) = [j in nbr[i, :k+1] if i in nbr[j, :k+1]] for every i, in list order (the masks in one numpy expression)."""
    L = nbr[:, :k + 1]
    back = (nbr[L][:, :, :k + 1] == np.arange(nbr.shape[0])[:, None, None]).any(2)
    return [L[i][back[i]].tolist() for i in range(nbr.shape[0])]


def sparse_ref(X, nbr, Nq, k1=20, k2=6, lam=0.3, dtype=np.float64):
    """Returns R, Rh, Rstar (lists), V and V2 (a {column: value} dictionary per pooled row, V in R* order), m and s ([Nq, Ng])."""
    X = np.asarray(X, dtype=dtype)
    nbr = np.asarray(nbr)
    N = X.shape[0]
    R, Rh = reciprocal_sets(nbr, k1), reciprocal_sets(nbr, kh_of(k1))
    Rstar, V = [], []
    for i in range(N):
        members, base = list(R[i]), set(R[i])
        for j in R[i]:
            if 3 * len(base & set(Rh[j])) > 2 * len(Rh[j]):
                seen = set(members)
                members += [c for c in Rh[j] if c not in seen]
        Rstar.append(members)
        e = np.exp(-(1 - X[members] @ X[i]))
        V.append(dict(zip(members, e / e.sum(dtype=dtype))))
    V2 = []
    for i in range(N):
        acc = {}
        for j in nbr[i, :k2]:
            for c, v in V[int(j)].items():
                acc[c] = acc[c] + v if c in acc else v
        V2.append({c: v / dtype(k2) for c, v in acc.items()})
    inverted = {}
    for g in range(N - Nq):
        for c, v in V2[Nq + g].items():
            inverted.setdefault(c, []).append((g, v))
    m = np.zeros((Nq, N - Nq), dtype)
    for q in range(Nq):
        for c in sorted(V2[q]):
            a = V2[q][c]
            for g, b in inverted.get(c, ()):
                m[q, g] += min(a, b)
    cos = X[:Nq] @ X[Nq:].T
    s = (dtype(1) - dtype(lam)) * (m / (2 - m)) + dtype(lam) * cos
    return {'R': R, 'Rh': Rh, 'Rstar': Rstar, 'V': V, 'V2': V2, 'm': m, 's': s}


def rows_max_diff(A, B):
    """Largest |A[i][c] - B[i][c]| over rows of dictionaries with equal key sets."""
    worst = 0.0
    for a, b in zip(A, B):
        assert a.keys() == b.keys()
        worst = max([worst] + [abs(float(a[c]) - float(b[c])) for c in a])
    return worst


def gate(ref64, ref32):
    """rerank_ref.gate on this module's results: 8 x the largest fp64-vs-fp32 difference of V, V2 and s, at least 4 fp32 ulps of 1."""
    worst = max(rows_max_diff(ref64['V'], ref32['V']), rows_max_diff(ref64['V2'], ref32['V2']),
                float(np.abs(ref64['s'] - ref32['s'].astype(np.float64)).max()))
    return max(8 * worst, 4 * float(np.finfo(np.float32).eps))
