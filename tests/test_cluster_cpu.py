"""Clustering without a GPU: the numpy restatement of the DBSCAN definition (cluster_ref.py) against sklearn, its independence of
the row order on asymmetric rows, the argument checks of the new entry points through the built libraries, the host-side checks of
prcv2025reid_amd.cluster, cluster_scores against a pair count, and the preconditions of the fixture the GPU tests cluster."""
import ctypes

import numpy as np
import pytest
import torch

import cluster_ref as CR

GPU_SEED = 51                 # the fixture test_cluster_gpu.py runs (picked here, on the fp64 restatement, for the preconditions below)


# ------------------------------------------------------------------------------------------- 1. the reference against sklearn
def sklearn_labels(S, thr, min_samples):
    DBSCAN = pytest.importorskip('sklearn.cluster').DBSCAN
    # d = top - S, eps = top - thr: the entries here are small multiples of 1/64, so both differences are exact and d <= eps <=> S >= thr
    top = float(max(S.max(), thr)) + 1.0
    model = DBSCAN(eps=top - float(np.float32(thr)), min_samples=min_samples, metric='precomputed').fit(top - S.astype(np.float64))
    core = np.zeros(S.shape[0], bool)
    core[model.core_sample_indices_] = True
    return model.labels_.astype(np.int64), core


def contested_borders(S, thr, labels, core, nbrs):
    """Non-core rows that cores of more than one cluster reach."""
    return [j for j in range(len(labels)) if not core[j] and len({labels[i] for i in range(len(labels)) if core[i] and j in nbrs[i]}) > 1]


def test_reference_is_sklearn_on_symmetric_matrices():
    rng = np.random.default_rng(0)
    contested = cases = 0
    for trial in range(160):
        N = int(rng.integers(1, 121))
        S = CR.point_similarity(rng, N)
        assert np.array_equal(S, S.T)
        thr = CR.threshold_for_degree(S, rng.uniform(1.5, 6.0))            # a value of the matrix: the >= boundary
        for min_samples in (1, int(rng.integers(2, 7))):
            labels, core, nbrs = CR.dbscan_reference(S, thr, min_samples)
            want, want_core = sklearn_labels(S, thr, min_samples)
            assert np.array_equal(core, want_core) and np.array_equal(labels, want), (trial, N, min_samples)
            assert min_samples > 1 or core.all()
            contested += len(contested_borders(S, thr, labels, core, nbrs))
            cases += 1
    print(f'  {cases} cases, {contested} border rows reachable from more than one cluster')
    assert contested >= 1


def test_reference_on_constructed_cases():
    # all noise; one cluster; a border row between two clusters takes the lower label
    S = CR.point_similarity(np.random.default_rng(1), 50) - 1 + np.eye(50, dtype=np.float32)
    labels, core, _ = CR.dbscan_reference(S, -0.5, 2)                     # nothing but the row itself clears the threshold
    assert (labels == -1).all() and not core.any() and np.array_equal(labels, sklearn_labels(S, -0.5, 2)[0])
    labels, core, _ = CR.dbscan_reference(S, -10.0, 4)
    assert (labels == 0).all() and core.all() and np.array_equal(labels, sklearn_labels(S, -10.0, 4)[0])
    # rows 0-3 and 5-8 are two cliques; row 4 touches row 3 and row 5 only: 3 neighbours with itself, not a core at min_samples = 4
    S = np.zeros((9, 9), np.float32)
    S[:4, :4] = S[5:, 5:] = 1
    S[4, 3] = S[3, 4] = S[4, 5] = S[5, 4] = 1
    labels, core, nbrs = CR.dbscan_reference(S, 0.5, 4)
    assert core.tolist() == [True] * 4 + [False] + [True] * 4 and labels.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert contested_borders(S, 0.5, labels, core, nbrs) == [4]
    assert np.array_equal(labels, sklearn_labels(S, 0.5, 4)[0])
    mirrored = S[::-1, ::-1].copy()                                           # the same graph with the cliques' indices swapped
    assert CR.dbscan_reference(mirrored, 0.5, 4)[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]


def test_reference_ignores_the_row_order_on_asymmetric_rows():
    rng = np.random.default_rng(2)
    differ = 0
    for N in (1, 7, 40, 90):
        S = (rng.integers(0, 32, (N, N)) / 32).astype(np.float32)
        S[rng.random((N, N)) < 0.02] = np.nan
        S[rng.random((N, N)) < 0.02] = np.inf
        thr = 1 - 3.0 / max(N, 4)
        for min_samples in (1, 3, 4):
            want = CR.dbscan_reference(S, thr, min_samples)
            for _ in range(4):
                got = CR.dbscan_reference(S, thr, min_samples, order=rng.permutation(N))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
            with np.errstate(invalid='ignore'):
                differ += int(((S >= thr) != (S.T >= thr)).sum())
            # +inf is a neighbour, NaN is not, the row itself always is
            assert all(i in nb for i, nb in enumerate(want[2]))
            assert all((j in want[2][i]) == (i == j or S[i, j] >= thr) for i in range(N) for j in range(N))
    assert differ > 100                                                       # the rows are far from symmetric


# ------------------------------------------------------------------------------------------- 2. the entry points' argument checks
@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    return {f: _lib.bind(ctypes.CDLL(p)) for f, p in _lib.LIB_PATHS.items()}


@pytest.mark.parametrize('flavor', ['bf16', 'f16'])
def test_entry_points_check_their_arguments_without_a_device(libs, flavor):
    h = libs[flavor]
    buf = (ctypes.c_float * 64)()                         # host memory: only its (16-byte aligned) address is looked at before the refusal
    p = ctypes.addressof(buf)
    p += (-p) % 16
    nan = float('nan')

    def count(scores=p, ld=8, nr=2, n=8, row0=0, thr=0.4, min_samples=4, count=p, core=p):
        return h.reid_dbscan_count(scores, ld, nr, n, row0, thr, min_samples, count, core, None)

    def fill(scores=p, ld=8, nr=2, n=8, row0=0, thr=0.4, rowptr=p, cols=p, cap=16):
        return h.reid_dbscan_fill(scores, ld, nr, n, row0, thr, rowptr, cols, cap, None)

    def refused(rc, *words):
        msg = h.reid_last_error()
        return rc == -1 and all(w in msg for w in words)

    for call, name in ((count, b'reid_dbscan_count'), (fill, b'reid_dbscan_fill')):
        assert refused(call(scores=None), name, b'null pointer')
        assert refused(call(n=0), name, b'n=0') and refused(call(nr=0), name, b'nr=0')
        assert refused(call(ld=4), name, b'ld=4') and refused(call(ld=10, n=8), name, b'ld=10')          # < n; not a multiple of 4
        assert refused(call(scores=p + 4), name, b'16-byte aligned') and refused(call(scores=p + 8), name, b'16-byte aligned')
        assert refused(call(thr=nan), name, b'thr is NaN')
        assert refused(call(row0=-1), name, b'row0=-1') and refused(call(row0=7), name, b'row0=7')      # rows 7, 8 of an 8 x 8 matrix
    assert refused(count(count=None), b'null pointer') and refused(count(core=None), b'null pointer')
    for m in (0, -3):
        assert refused(count(min_samples=m), b'reid_dbscan_count', b'min_samples=%d' % m)
    assert refused(fill(rowptr=None), b'null pointer') and refused(fill(cols=None), b'reid_dbscan_fill', b'null array of columns')
    assert refused(fill(cap=-1), b'reid_dbscan_fill', b'cap=-1')

    def hook(rowptr=p, cols=p, nnz=4, core=p, parent=p, N=4, changed=p):
        return h.reid_dbscan_hook(rowptr, cols, nnz, core, parent, N, changed, None)

    def border(rowptr=p, cols=p, nnz=4, core=p, parent=p, label=p, N=4):
        return h.reid_dbscan_border(rowptr, cols, nnz, core, parent, label, N, None)

    for call, name in ((hook, b'reid_dbscan_hook'), (border, b'reid_dbscan_border')):
        for arg in ('rowptr', 'core', 'parent'):
            assert refused(call(**{arg: None}), name, b'null pointer')
        assert refused(call(cols=None), name, b'null array of columns') and refused(call(nnz=-1), name, b'nnz=-1')
        assert refused(call(N=0), name, b'N=0')
    assert refused(hook(changed=None), b'null pointer') and refused(border(label=None), b'null pointer')
    assert refused(h.reid_dbscan_compress(None, 4, None), b'reid_dbscan_compress', b'null pointer')
    assert refused(h.reid_dbscan_compress(p, 0, None), b'reid_dbscan_compress', b'N=0')


# ------------------------------------------------------------------------------------------- 3. the host side of the public module
def test_cluster_params_ranges():
    from prcv2025reid_amd import _lib, rerank
    from prcv2025reid_amd.cluster import ClusterParams
    p = ClusterParams()
    assert (p.k1, p.k2, p.eps, p.min_samples, p.lambda_value, p.sparse) == (30, 6, 0.6, 4, 0.0, None)
    assert p.threshold == float(np.float32(1.0 - 0.6)) and ClusterParams(eps=0.0).threshold == 1.0 and ClusterParams(eps=1.0).threshold == 0.0
    for eps in (-0.01, 1.01, float('nan')):
        with pytest.raises(_lib.ReidHipError, match='eps='):
            ClusterParams(eps=eps)
    for m in (0, -1, 2.5):
        with pytest.raises(_lib.ReidHipError, match='min_samples='):
            ClusterParams(min_samples=m)
    # sparse=None: dense up to the dense form's row limit, sparse beyond
    assert p.rerank_params(rerank.MAX_ROWS).sparse is False and p.rerank_params(rerank.MAX_ROWS + 1).sparse is True
    assert ClusterParams(sparse=True).rerank_params(100).sparse is True and ClusterParams(sparse=False).rerank_params(10 ** 6).sparse is False
    assert p.rerank_params(100) == rerank.RerankParams(k1=30, k2=6, lambda_value=0.0, sparse=False)


def test_public_calls_check_before_the_device():
    from prcv2025reid_amd import _lib, rerank
    from prcv2025reid_amd.cluster import ClusterParams, dbscan_rows, jaccard_dbscan, round_cap
    X = torch.randn(64, 16)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        jaccard_dbscan(X)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        dbscan_rows([(0, torch.zeros(4, 4))], 4, 0.5, 2)
    # the other fields are the re-ranker's, checked with the pool's N
    for N, params, word in ((64, ClusterParams(k1=64), 'k1 [+] 1 = 65 neighbours asked of N = 64'), (128, ClusterParams(k1=65), 'k1=65 outside'),
                            (128, ClusterParams(k2=32), 'k2=32 outside'), (128, ClusterParams(lambda_value=1.5), 'lambda=1.5'),
                            (128, ClusterParams(k1=64, k2=8, sparse=True), 'merge')):
        with pytest.raises(_lib.ReidHipError, match=word):
            jaccard_dbscan(torch.randn(N, 16), params)
    with pytest.raises(_lib.ReidHipError, match='exceeds 65536 rows'):
        rerank.check_pool(rerank.MAX_ROWS + 1, rerank.RerankParams())
    with pytest.raises(_lib.ReidHipError, match='at least one pooled row'):
        rerank.check_pool(0, rerank.RerankParams())
    with pytest.raises(_lib.ReidHipError, match='at least one query and one gallery row'):       # the existing constructors still refuse Nq = 0
        rerank.check_shapes(0, 100, rerank.RerankParams())
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        rerank.Reranker.for_pool(torch.randn(64, 16), rerank.RerankParams())
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        rerank.SparseReranker.for_pool(torch.randn(64, 16), rerank.RerankParams(sparse=True))
    # dbscan_rows: the scalar arguments, and chunks that do not cover 0 .. N - 1 in order (refused before the chunk is looked at)
    for N, thr, m, word in ((0, 0.5, 2, 'N=0'), (4, float('nan'), 2, 'NaN'), (4, 0.5, 0, 'min_samples=0')):
        with pytest.raises(_lib.ReidHipError, match=word):
            dbscan_rows([], N, thr, m)
    with pytest.raises(_lib.ReidHipError, match='end at row 0 of 4'):
        dbscan_rows([], 4, 0.5, 2)
    for chunks in ([(1, torch.zeros(3, 4))], [(0, torch.zeros(5, 8))], [(0, torch.zeros(4))], [(0, None)]):
        with pytest.raises(_lib.ReidHipError, match='chunks ascend and cover every row once'):
            dbscan_rows(chunks, 4, 0.5, 2)
    assert [round_cap(n) for n in (1, 4095, 4096, 65536)] == [12, 56, 60, 76]      # 4 ceil(log2(N + 1)) + 8


def test_cluster_scores_is_the_pair_count():
    from prcv2025reid_amd.cluster import cluster_scores
    rng = np.random.default_rng(3)
    for n, ncl, nid in ((1, 1, 1), (2, 1, 2), (40, 5, 7), (90, 12, 9), (60, 1, 60)):
        for noise in (0.0, 0.3):
            labels = rng.integers(0, ncl, n)
            labels[rng.random(n) < noise] = -1
            pids = rng.integers(0, nid, n) * 1000 - 5
            got = cluster_scores(torch.as_tensor(labels), torch.as_tensor(pids))
            assert got == pytest.approx(CR.pair_scores(labels, pids), abs=1e-15), (n, ncl, nid, noise)
    assert cluster_scores(torch.tensor([0, 0, 1, 1, -1, -1]), torch.tensor([7, 7, 7, 8, 9, 9])) == pytest.approx((0.5, 0.25, 1 / 3))
    assert cluster_scores(torch.tensor([-1, -1]), torch.tensor([1, 2])) == (1.0, 1.0, 1.0)      # no pair on either side
    with pytest.raises(ValueError):
        cluster_scores(torch.zeros(3), torch.zeros(4))


# ------------------------------------------------------------------------------------------- 4. the end-to-end fixture
@pytest.mark.parametrize('seed', [0, 1, 2, GPU_SEED])
def test_fixture_labels_do_not_hang_on_the_precision(seed):
    """On the fp64 restatement of the pooled pipeline (k1 = 10, k2 = 3, lambda = 0, eps = 0.6, min_samples = 4): every pooled s* is
    further from the threshold than 100 x the fp32-vs-fp64 gate, so an fp32 pipeline within the gate yields the same neighbour lists;
    the fp32 restatement yields the same labels; every identity is one whole cluster, 40 clusters.  Measured on seeds 0, 1, 2, 51:
    gap to the threshold 1.9e-2 .. 1.5e-1, gate 2.1e-6 .. 2.3e-6."""
    f = CR.FIXTURE
    p = CR.pooled_reference(seed)
    s, pid, labels = p['r64']['s'], p['pid'], p['labels64']
    assert p['X'].shape == (340, 64) and p['X'].dtype == np.float32 and p['thr'] == np.float32(0.4)
    gap = float(np.abs(s - np.float64(p['thr'])).min())
    print(f'  seed {seed}: gap to the threshold {gap:.3e}, gate {p["gate"]:.3e}')
    assert gap > 100 * p['gate']                                                                  # a)
    assert np.array_equal(labels, p['labels32'])                                                  # b)
    assert labels.max() + 1 == f['nid']                                                           # c)
    of_identity = [set(labels[pid == k].tolist()) for k in range(f['nid'])]
    assert all(len(c) == 1 and min(c) >= 0 for c in of_identity) and len(set.union(*of_identity)) == f['nid']
    if seed == GPU_SEED:
        # what the GPU tests lean on besides: the kNN lists that are read are settled in fp32, and no outlier joins a cluster
        import rerank_ref as R
        assert R.min_gap_in_top(p['r64']['cos'], f['k1'] + 3) >= 1e-5
        assert (labels[pid < 0] == -1).all() and CR.pair_scores(labels[labels >= 0], pid[labels >= 0])[0] == 1.0
