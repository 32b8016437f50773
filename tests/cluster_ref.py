"""numpy restatement of the DBSCAN definition and the seeded fixtures the clustering tests share.  Written from the
definition, plain loops and a union-find, nothing shared with the package.  test_cluster_cpu.py checks it against sklearn."""
import functools

import numpy as np

import rerank_ref as R


def dbscan_reference(S, thr, min_samples, order=None):
    """(labels i64 [N], core bool [N], neighbour lists) of the N rows of the similarity matrix S (larger = closer; columns >= N are
    ignored).  j is a neighbour of i when S[i, j] >= thr in S's own dtype (NaN never, +inf always) or j == i.  ``order``: the order in
    which the rows are visited when the cores are joined; the result does not depend on it."""
    S = np.asarray(S)
    N = S.shape[0]
    thr = S.dtype.type(thr)
    nbrs = []
    for i in range(N):
        with np.errstate(invalid='ignore'):
            near = S[i, :N] >= thr
        near[i] = True
        nbrs.append([int(j) for j in np.nonzero(near)[0]])                 # ascending
    core = np.array([len(nb) >= min_samples for nb in nbrs], bool)

    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in (range(N) if order is None else order):
        if core[i]:
            for j in nbrs[i]:
                if core[j]:                                                  # joined iff j in N(i) or i in N(j): the undirected union
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    smallest = {}                                                            # component -> its smallest core row
    for i in range(N):
        if core[i]:
            smallest.setdefault(find(i), i)                                  # i ascends: the first core seen is the smallest
    number = {c: k for k, c in enumerate(sorted(smallest, key=smallest.get))}
    labels = np.full(N, -1, np.int64)
    for i in range(N):
        if core[i]:
            labels[i] = number[find(i)]
    for i in range(N):
        if core[i]:
            for j in nbrs[i]:
                if not core[j] and (labels[j] < 0 or labels[i] < labels[j]):
                    labels[j] = labels[i]
    return labels, core, nbrs


def csr_of(nbrs):
    """(rowptr i64 [N + 1], cols i32) of neighbour lists."""
    rowptr = np.concatenate([[0], np.cumsum([len(nb) for nb in nbrs])]).astype(np.int64)
    return rowptr, np.array([j for nb in nbrs for j in nb], np.int32)


def pair_scores(labels, pids):
    """(precision, recall, F1) by counting every pair of rows; a noise row (label < 0) shares a cluster with nobody; a side
    without a pair scores 1."""
    n = len(labels)
    both = predicted = true = 0
    for i in range(n):
        for j in range(i + 1, n):
            p = labels[i] >= 0 and labels[i] == labels[j]
            t = pids[i] == pids[j]
            predicted += p
            true += t
            both += p and t
    precision = both / predicted if predicted else 1.0
    recall = both / true if true else 1.0
    return precision, recall, (2 * precision * recall / (precision + recall) if precision + recall else 0.0)


# ----------------------------------------------------------------------------------------------------------------- fixtures
def point_similarity(rng, N, dim=2, step=1 / 64):
    """-(Euclidean distance) of N random points, rounded to multiples of ``step``: symmetric, fp32, many equal values."""
    P = rng.random((N, dim))
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    return (-np.round(d / step) * step).astype(np.float32)


def threshold_for_degree(S, degree):
    """A value that occurs in S (so that >= is exercised on equality) below which about ``degree`` entries per row lie."""
    v = np.sort(S[np.isfinite(S)].ravel())[::-1]
    return float(v[min(v.size - 1, int(degree * S.shape[0]))])


FIXTURE = dict(nid=40, per=8, outliers=20, D=64, noise=0.35, k1=10, k2=3, lam=0.0, eps=0.6, min_samples=4)


def identity_fixture(seed):
    """(X f32 [340, 64] unit rows, pid [340]): 40 identities x 8 rows, each a Gaussian centroid plus 0.35 N(0, 1), and 20 outlier
    rows (pid -1, -2, ..), in a permuted order.  An outlier is far from every identity and from every other outlier: the outliers
    are orthonormal directions of the complement of the centroids' span, so the rows nearest to one are a few unrelated identity
    rows, by the noise alone.  (A random direction instead leans towards one centroid; its two nearest rows are then of one identity,
    the k2 = 3 expansion hands it two thirds of their weight, and it is a legitimate border row of that cluster.)"""
    f = FIXTURE
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((f['nid'], f['D']))
    pid = np.concatenate([np.repeat(np.arange(f['nid']), f['per']), -1 - np.arange(f['outliers'])])
    basis = np.linalg.qr(np.concatenate([cent, rng.standard_normal((f['D'] - f['nid'], f['D']))]).T)[0].T      # rows nid.. : the complement
    X = np.concatenate([cent[pid[pid >= 0]] + f['noise'] * rng.standard_normal((f['nid'] * f['per'], f['D'])),
                        basis[f['nid']:f['nid'] + f['outliers']]])
    perm = rng.permutation(X.shape[0])
    X, pid = X[perm], pid[perm]
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    X = (X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return X, pid


@functools.lru_cache(maxsize=None)
def pooled_reference(seed):
    """The fixture through the fp64 restatement of the pooled pipeline, computed once and shared: X, pid, the fp64 and fp32 runs
    ({'cos', 'nbr', 'V', 'V2', 's'}: 's' = the pooled s* [N, N], every row against every row), the gate of rerank_ref, the threshold
    float32(1 - eps) and the labels of both runs.  rerank_ref cannot take Nq = 0: it is called with Nq = 1 and its 's' replaced."""
    f = FIXTURE
    X, pid = identity_fixture(seed)
    runs = []
    for dtype, nbr in ((np.float64, None), (np.float32, 'of the fp64 run')):
        r = R.rerank_ref(X, 1, f['k1'], f['k2'], f['lam'], dtype, nbr=runs[0]['nbr'] if nbr else None)
        r['s'] = R.jaccard_ref(r['V2'], r['V2'], r['cos'], f['lam'], dtype)
        runs.append(r)
    r64, r32 = runs
    thr = np.float32(1.0 - f['eps'])
    return dict(X=X, pid=pid, r64=r64, r32=r32, gate=R.gate(r64, r32), thr=thr,
                labels64=dbscan_reference(r64['s'], thr, f['min_samples'])[0],
                labels32=dbscan_reference(r32['s'], thr, f['min_samples'])[0])
