"""The reference of the hybrid memory loss (csrc/hybrid_nce.hip; include/reid_hip.h, reid_class_means / reid_hybrid_*) in numpy, and the
tolerances the GPU tests use.

Two things are stated here in fp32, operation by operation, because the kernels must reproduce them BIT FOR BIT: the table formula
(class_means: the members' entries added one by one in ascending instance index, starting from the first member, divided once by the
count -- numpy rounds every fp32 addition and the division on their own, nothing is fused) and the blend loop (blend_f32: two rounded
products, their rounded sum, the norm, the division).  Only the table is compared by bits; an entry after a blend is compared with the
fp64 recurrence within its bound, since the order of the additions inside the norm is the kernel's own.

Everything else is fp64 and comes from cluster_nce_ref.py: the loss IS the cluster-contrast forward against the table of class means
(the mean of dot products is the dot product with the mean), so forward() calls R.forward with the fp32 table the device holds (which
class_means reproduces bit for bit) and the gathered labels, and row_bound / loss_bound / dx_bound are R's with cmax = the largest
table-row norm (<= 1 up to rounding: R's bounds assume unit centroids, every term of theirs scales with |C_c|, so they hold for the
shorter rows of a mean; the row norm bounds the largest element dx_bound asks for).  The update of an entry is R.update's blend
recurrence keyed by instance instead of label.
"""
import numpy as np

import cluster_nce_ref as R

U, EPS = R.U, R.EPS
row_bound, loss_bound, cos_bound, dx_bound, contributing = R.row_bound, R.loss_bound, R.cos_bound, R.dx_bound, R.contributing


# ---------------------------------------------------------------------------------------------------------------- the table
def csr(cls, C=None):
    """(order [M], offsets [C + 1], counts [C]) of the classes ``cls`` [M]: the members of every class in ascending instance index."""
    cls = np.asarray(cls, dtype=np.int64)
    C = int(cls.max()) + 1 if C is None else C
    counts = np.bincount(cls, minlength=C).astype(np.int64)
    return np.argsort(cls, kind='stable').astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), counts


def class_means(V, cls, C=None):
    """T [C, D] fp32 by the table formula, in fp32: T_c = fl(fl(sum over the members, one by one, ascending) / float(n_c))."""
    V = np.asarray(V)
    assert V.dtype == np.float32
    order, offsets, counts = csr(cls, C)
    T = np.zeros((len(counts), V.shape[1]), dtype=np.float32)
    for c in range(len(counts)):
        members = order[offsets[c]:offsets[c + 1]]
        assert len(members) > 0, f'class {c} has no member'
        acc = V[members[0]].copy()
        for i in members[1:]:
            acc = acc + V[i]                                       # fp32 + fp32, rounded once per element
        T[c] = acc / np.float32(len(members))
    return T


def class_means64(V, cls, C=None):
    """The same means in fp64 (for the comparison with SpCL's literal form)."""
    V = np.asarray(V, dtype=np.float64)
    order, offsets, counts = csr(cls, C)
    return np.stack([V[order[offsets[c]:offsets[c + 1]]].mean(axis=0) for c in range(len(counts))])


def table_norm(T):
    return float(np.linalg.norm(np.asarray(T, dtype=np.float64), axis=1).max())


# ---------------------------------------------------------------------------------------------------------------- the loss
def gather_labels(index, cls):
    index = np.asarray(index, dtype=np.int64)
    ok = (index >= 0) & (index < len(cls))
    return np.where(ok, np.asarray(cls, dtype=np.int64)[np.clip(index, 0, len(cls) - 1)], -1)


def forward(x, index, valid, T, cls, tau, dloss=1.0):
    """The fp64 forward of x [S, N, D] for the dataset rows ``index`` [N] against the table ``T`` [C, D] (the fp32 class means, or any
    float array): R.forward's dict, plus 'index' [R] = the instance of every row (-1: outside the memory)."""
    S = np.asarray(x).shape[0]
    index = np.asarray(index, dtype=np.int64)
    f = R.forward(x, gather_labels(index, cls), valid, T, tau, dloss)
    f['index'] = np.tile(np.where((index >= 0) & (index < len(cls)), index, -1), S)
    return f


# ---------------------------------------------------------------------------------------------------------------- the update
def blend_f32(v, rows, momentum):
    """The blend loop of one entry in fp32, products and sums un-fused: v <- fl(fl(m v) + fl((1 - m) x)); v <- v / max(|v|, 1e-12),
    over ``rows`` (unit rows, fp32) in the order given."""
    v = np.asarray(v, dtype=np.float32).copy()
    m = np.float32(momentum)
    keep = np.float32(1) - m
    for xr in rows:
        v = v * m + np.asarray(xr, dtype=np.float32) * keep
        v = v / np.maximum(np.sqrt((v * v).sum(dtype=np.float32)), np.float32(EPS))
    return v


def update_instances(V, f, momentum, D=None, err0=None, xhat_dev=0.0):
    """(V' [M, D] fp64, err [M]): the entries after the update of the forward ``f`` and the 2-norm bound of every entry's deviation --
    R.update's blend recurrence with the instance of a row in the place of its label ('mean': every contributing row, ascending)."""
    return R.update(V, dict(f, y=f['index']), momentum, 'mean', D=D, err0=err0, xhat_dev=xhat_dev)


def touched(f, cls):
    """(instances, classes) with a contributing row, as sorted lists."""
    con = contributing(f)
    inst = sorted(set(f['index'][con].tolist()))
    return inst, sorted(set(np.asarray(cls)[inst].tolist()))


# ---------------------------------------------------------------------------------------------------------------- cases
def memory_case(M, D, C, seed, spread=0.5):
    """(V [M, D] fp32 unit entries, cls [M]): C classes interleaved through the M instances -- about half of them singletons (SpCL's
    outliers), the rest sharing the remaining instances; the members of a class lie around a common direction, so that the mean of a
    large class is not short."""
    g = np.random.default_rng(seed)
    assert M >= C >= 1
    n_single = C // 2 if M > C else C
    multi = C - n_single
    cls = np.concatenate([np.arange(C), g.integers(0, multi, size=M - C) if multi else np.zeros(0, dtype=np.int64)]).astype(np.int64)
    cls = cls[g.permutation(M)]
    cent = g.standard_normal((C, D))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    V = cent[cls] + spread * g.standard_normal((M, D)) / np.sqrt(D)
    return (V / np.linalg.norm(V, axis=1, keepdims=True)).astype(np.float32), cls


def batch_case(S, N, D, V, cls, seed, noise=True):
    """(x [S, N, D] fp32, index [N], valid [S, N] uint8): random directions with norms 0.5 .. 3, unrelated to their instances (as
    R.random_case: the loss of a row is then about log C or more and its gradient large); row 0 is an instance of a singleton class
    and row 2 one of a multi-member class when there are such; with ``noise`` and N >= 5, index[1] = -1 and index[N - 2] = M, and
    some rows are invalid when S * N >= 5."""
    g = np.random.default_rng(seed)
    M = len(cls)
    counts = np.bincount(cls)
    index = g.integers(0, M, size=N).astype(np.int64)
    single, multi = np.flatnonzero(counts[cls] == 1), np.flatnonzero(counts[cls] > 1)
    if len(single):
        index[0] = single[seed % len(single)]
    if N >= 3 and len(multi):
        index[2] = multi[seed % len(multi)]
    if noise and N >= 5:
        index[1], index[N - 2] = -1, M
    x = g.standard_normal((S, N, D)) * g.uniform(0.5, 3.0, size=(S, N, 1))
    valid = np.ones((S, N), dtype=np.uint8)
    if S * N >= 5:
        valid.reshape(-1)[3::7] = 0
    return x.astype(np.float32), index, valid


def signal(f, D, C, tau, dloss, cmax):
    """(smallest row loss / row_bound, smallest over the used rows of max |dx| / dx_bound) of a reference forward (formed with
    dloss = 1): how far what a test compares stands above what it compares it within -- for EVERY used row."""
    u = f['used']
    b = dx_bound(f, D, C, tau, dloss, cmax)
    return float(f['row_loss'][u].min() / row_bound(D, C, tau)), float((np.abs(f['dx'][u] * dloss).max(axis=1) / b[u]).min())
