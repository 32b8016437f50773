"""GPU: DBSCAN on the device (csrc/cluster.hip, prcv2025reid_amd/cluster.py).  Every comparison of labels, core flags and the
neighbour CSR is exact; the reference is cluster_ref.dbscan_reference (checked against sklearn in test_cluster_cpu.py).  The pooled
re-ranker's rows are compared with the fp64 restatement within rerank_ref.gate, as test_rerank_gpu.py does for the two-set form.

Sizes are the smallest at which the logic can break: rows shorter than one 16-byte load, rows of several 1024-column steps of the
fill pass with a ragged end, chunks of 7 rows (row0 not a multiple of anything), more than one workgroup in every pass."""
import functools

import numpy as np
import pytest
import torch

import cluster_ref as CR
import rerank_ref as R
from test_cluster_cpu import GPU_SEED

pytestmark = pytest.mark.gpu
MARK = -7777


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def padded(S):
    """S on the device in a buffer of ld = N rounded up to 4, + 4 when that adds nothing: NaN and +inf in the padding columns."""
    N = S.shape[0]
    ld = (N + 3) // 4 * 4 + (4 if N % 4 == 0 else 0)
    P = np.empty((N, ld), np.float32)
    P[:, 0::2], P[:, 1::2] = np.nan, np.inf
    P[:, :N] = S
    return dev(P)


def chunks_of(Sd, chunk):
    return ((a, Sd[a:a + chunk]) for a in range(0, Sd.shape[0], chunk))


def assert_is_reference(got, want, what):
    labels, core, nbrs = want
    rowptr, cols = CR.csr_of(nbrs)
    assert got.labels.dtype == torch.int64 and got.core.dtype == torch.bool and got.rowptr.dtype == torch.int64 and got.cols.dtype == torch.int32
    assert np.array_equal(got.rowptr.cpu().numpy(), rowptr), what
    assert np.array_equal(got.cols.cpu().numpy(), cols), what
    assert np.array_equal(got.core.cpu().numpy(), core), what
    assert np.array_equal(got.labels.cpu().numpy(), labels), what
    assert got.n_clusters == labels.max() + 1, what


# ------------------------------------------------------------------------------------------------------- 1. the precomputed form
@functools.lru_cache(maxsize=None)
def matrix(N, kind):
    """(S f32 [N, N], thr): 'sym' = rounded point distances, 'asym' = unrelated entries per direction; both with a +inf and NaNs
    inside (one NaN on a diagonal) and a threshold that is a value of the matrix; 'far' = nothing clears the threshold."""
    rng = np.random.default_rng(1000 + N)
    if kind == 'asym':
        S = (rng.integers(0, 16 * N, (N, N)) / (16 * N)).astype(np.float32)    # each value about N / 16 times
        thr = CR.threshold_for_degree(S, 1.2)
    else:
        S = CR.point_similarity(rng, N)
        thr = CR.threshold_for_degree(S, 4.0)
    if kind == 'far':
        return S, float(S.max()) + 1.0
    for value in (np.nan, np.inf, np.nan):
        i, j = rng.integers(0, N, 2)
        S[i, j] = value
        if kind == 'sym':
            S[j, i] = value
    S[N // 2, N // 2] = np.nan                                # the row still counts itself
    return S, thr


@pytest.mark.parametrize('N', [1, 5, 64, 257, 1000])
def test_precomputed_form_is_the_reference(N):
    from prcv2025reid_amd.cluster import dbscan_rows, round_cap
    for kind in ('sym', 'asym', 'far'):
        S, thr = matrix(N, kind)
        Sd = padded(S)
        for min_samples in (1, 4):
            want = CR.dbscan_reference(S, thr, min_samples)
            if kind == 'far':                                       # every row alone: all noise, or all clusters of one core
                assert np.array_equal(want[0], np.arange(N) if min_samples == 1 else np.full(N, -1))
            elif N >= 64:
                assert np.isinf(S).any() and np.isnan(S).sum() >= 2 and (S == np.float32(thr)).sum() >= 2     # the >= boundary is met
                if min_samples == 4:                                # the case is a mixture: clusters, border rows, noise
                    assert want[0].max() >= 1 and (want[0] == -1).any() and (~want[1] & (want[0] >= 0)).any(), (N, kind)
            for chunk in sorted({7, 256, N}):
                got = dbscan_rows(chunks_of(Sd, chunk), N, thr, min_samples)
                assert_is_reference(got, want, (N, kind, min_samples, chunk))
                assert 1 <= got.rounds <= round_cap(N)
                index, labels = got.kept()
                assert np.array_equal(index.cpu().numpy(), np.nonzero(want[0] >= 0)[0]) and torch.equal(labels, got.labels[index])
    if N >= 64:
        S, thr = matrix(N, 'asym')
        with np.errstate(invalid='ignore'):
            assert ((S >= thr) != (S.T >= thr)).sum() > N               # the asymmetric case is asymmetric


def test_count_and_fill_write_their_rows_only():
    # sentinels around everything the two row kernels write; a row chunk in the middle of the matrix, rows of 2.5 steps of the fill pass
    from prcv2025reid_amd import ops
    N, a, nr = 2500, 1203, 9
    rng = np.random.default_rng(5)
    S = (rng.integers(0, 64, (nr, N)) / 64).astype(np.float32)
    thr = 0.75
    Sd = dev(np.concatenate([S, np.full((nr, 4), np.inf, np.float32)], 1))
    count = torch.full((nr + 2,), MARK, dtype=torch.int32, device='cuda')
    core = torch.full((nr + 2,), 77, dtype=torch.uint8, device='cuda')
    want = [sorted(set(np.nonzero(S[r] >= thr)[0].tolist()) | {a + r}) for r in range(nr)]
    median = sorted(len(w) for w in want)[nr // 2]
    ops.dbscan_count(Sd, N, a, thr, median, count[1:-1], core[1:-1])
    assert count.tolist() == [MARK] + [len(w) for w in want] + [MARK]
    assert core.tolist() == [77] + [int(len(w) >= median) for w in want] + [77] and 0 < int(core[1:-1].sum()) < nr
    rowptr = torch.zeros(nr + 1, dtype=torch.int64, device='cuda')
    rowptr[1:] = count[1:-1].long().cumsum(0)
    nnz = int(rowptr[-1])
    cols = torch.full((nnz + 8,), MARK, dtype=torch.int32, device='cuda')
    ops.dbscan_fill(Sd, N, a, thr, rowptr, cols)
    assert cols.tolist() == [j for w in want for j in w] + [MARK] * 8
    # a rowptr that leaves a row too little room, and an array shorter than rowptr says: nothing lands outside either
    short = rowptr.clone()
    short[1:] -= 3
    cols2 = torch.full((nnz,), MARK, dtype=torch.int32, device='cuda')
    ops.dbscan_fill(Sd, N, a, thr, short, cols2[:nnz - 40])
    torch.cuda.synchronize()
    got = cols2.tolist()
    assert got[:len(want[0]) - 3] == want[0][:-3] and got[nnz - 40:] == [MARK] * 40


# ------------------------------------------------------------------------------------------------------- 2. components
def chain_matrix(order, N, extra=()):
    """S on the device: 1 between consecutive rows of ``order`` (both directions), 1 at the directed pairs ``extra``, else 0."""
    S = torch.zeros(N, (N + 3) // 4 * 4, device='cuda')
    o = torch.as_tensor(np.asarray(order), device='cuda')
    S[o[:-1], o[1:]] = 1
    S[o[1:], o[:-1]] = 1
    for i, j in extra:
        S[i, j] = 1
    return S


def test_a_permuted_chain_is_one_cluster_within_the_round_cap():
    from prcv2025reid_amd.cluster import dbscan_rows, round_cap
    N = 4096
    order = np.random.default_rng(7).permutation(N)
    S = chain_matrix(order, N)
    got = dbscan_rows(chunks_of(S, 1024), N, 0.5, 2)
    print(f'  permuted chain of {N} cores: {got.rounds} rounds (cap {round_cap(N)})')
    assert got.rounds <= round_cap(N) == 60
    assert got.n_clusters == 1 and bool(got.core.all()) and bool((got.labels == 0).all())
    assert int(got.rowptr[-1]) == got.cols.numel() == 3 * N - 2          # every row: itself and two links, the two ends one
    # at min_samples = 3 the two ends are border rows of the same cluster; at 4 nothing is a core
    ends = dbscan_rows(chunks_of(S, 1024), N, 0.5, 3)
    assert ends.n_clusters == 1 and int(ends.core.sum()) == N - 2 and bool((ends.labels == 0).all())
    assert not bool(ends.core[int(order[0])]) and not bool(ends.core[int(order[-1])])
    none = dbscan_rows(chunks_of(S, 1024), N, 0.5, 4)
    assert none.n_clusters == 0 and bool((none.labels == -1).all()) and none.rounds == 1


def test_two_chains_that_share_a_border_row_stay_two_clusters():
    from prcv2025reid_amd.cluster import dbscan_rows
    N = 301
    perm = np.random.default_rng(8).permutation(N)
    first, second, shared = perm[:150], perm[150:300], int(perm[300])
    # cores of both chains reach the shared row; its own row reaches nobody, so it is not a core and joins nothing
    extra = [(int(first[40]), shared), (int(second[70]), shared), (int(second[71]), shared)]
    S = chain_matrix(first, N, extra)
    S += chain_matrix(second, N)
    want = CR.dbscan_reference(S[:, :N].cpu().numpy(), 0.5, 3)
    got = dbscan_rows(chunks_of(S, 64), N, 0.5, 3)
    assert_is_reference(got, want, 'two chains')
    labels = got.labels.cpu().numpy()
    assert got.n_clusters == 2 and not bool(got.core[shared]) and labels[shared] == 0
    assert len(set(labels[first[1:-1]])) == 1 and len(set(labels[second[1:-1]])) == 1 and labels[first[1]] != labels[second[1]]
    # the lower label is the chain with the smaller core row, whichever chain that is
    low = first if first[1:-1].min() < second[1:-1].min() else second
    assert labels[low[1]] == 0


# ------------------------------------------------------------------------------------------------------- 3. the pooled re-ranker
@functools.lru_cache(maxsize=None)
def pooled(sparse):
    """(reference bundle, the re-ranker over the pool, its s* rows on the host, the clustering) of the fixture, once per form."""
    from prcv2025reid_amd.cluster import ClusterParams, jaccard_dbscan
    from prcv2025reid_amd.rerank import Reranker, SparseReranker
    f = CR.FIXTURE
    p = CR.pooled_reference(GPU_SEED)
    params = ClusterParams(k1=f['k1'], k2=f['k2'], eps=f['eps'], min_samples=f['min_samples'], lambda_value=f['lam'], sparse=sparse)
    Xd = dev(p['X'])
    N = Xd.shape[0]
    rr = (SparseReranker if sparse else Reranker).for_pool(Xd, params.rerank_params(N))
    rows = torch.cat([rr.rows(a, min(N, a + 100))[:, :N] for a in range(0, N, 100)]).cpu().numpy()
    return p, rr, rows, jaccard_dbscan(Xd, params, normalized=True, chunk=100)


@pytest.mark.parametrize('sparse', [False, True])
def test_pooled_rows_and_labels_on_the_fixture(sparse):
    from prcv2025reid_amd.cluster import cluster_scores
    from prcv2025reid_amd.rerank import SparseReranker
    f = CR.FIXTURE
    p, rr, rows, got = pooled(sparse)
    N = p['X'].shape[0]
    assert isinstance(rr, SparseReranker) == sparse and (rr.Nq, rr.Ng, rr.N) == (0, N, N)
    assert np.array_equal(rr.nbr.cpu().numpy(), p['r64']['nbr'][:, :f['k1'] + 1])
    err = float(np.abs(rows - p['r64']['s']).max())
    print(f'  pooled rows ({"sparse" if sparse else "dense"}): max |s* - ref| = {err:.3e}, gate {p["gate"]:.3e}')
    assert err <= p['gate']
    assert_is_reference(got, CR.dbscan_reference(rows, p['thr'], f['min_samples']), 'the device\'s own rows')
    assert np.array_equal(got.labels.cpu().numpy(), p['labels64'])            # test_cluster_cpu.py: the gap is 100 gates wide
    assert got.n_clusters == f['nid']
    index, labels = got.kept()
    assert index.numel() == f['nid'] * f['per']
    precision, recall, f1 = cluster_scores(labels, dev(p['pid'])[index])
    assert (precision, recall, f1) == (1.0, 1.0, 1.0)
    assert cluster_scores(got.labels, dev(p['pid'])) == (1.0, 1.0, 1.0)      # the outliers are noise: singletons on both sides
    # ranked lists of the pooled form: rows_topk over all N columns
    idx, score = rr.topk(0, 50, 5)
    order = torch.sort(torch.as_tensor(rows[:50]), dim=1, descending=True, stable=True)[1][:, :5]
    assert torch.equal(idx.cpu().long(), order)


def test_dense_and_sparse_give_the_same_labels():
    dense, sparse = pooled(False)[3], pooled(True)[3]
    assert torch.equal(dense.labels, sparse.labels) and torch.equal(dense.core, sparse.core)
    assert torch.equal(dense.rowptr, sparse.rowptr) and torch.equal(dense.cols, sparse.cols)


# ------------------------------------------------------------------------------------------------------- 4. determinism, integration
def test_two_runs_give_the_same_bits():
    from prcv2025reid_amd.cluster import dbscan_rows
    S, thr = matrix(1000, 'sym')
    Sd = padded(S)
    runs = [dbscan_rows(chunks_of(Sd, 256), 1000, thr, 4) for _ in range(3)]
    for other in runs[1:]:
        for field in ('labels', 'core', 'rowptr', 'cols'):
            assert torch.equal(getattr(other, field), getattr(runs[0], field)), field
        assert other.n_clusters == runs[0].n_clusters


def test_kept_rows_feed_a_model_of_n_clusters_classes():
    from prcv2025reid_amd.config import TrainingConfig
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel
    got = pooled(False)[3]
    index, labels = got.kept()
    assert bool((index[1:] > index[:-1]).all()) and int(labels.min()) == 0 and int(labels.max()) == got.n_clusters - 1
    assert sorted(torch.unique(labels).tolist()) == list(range(got.n_clusters))
    cfg = TrainingConfig(device='cuda:0', mer_lora_rank=4, contrastive_weight=0.1, vision_hidden_dim=128, vision_layers=2, vision_heads=2,
                         vision_mlp_dim=256, text_layers=2, text_mlp_dim=1024, text_vocab=1024, text_eos_id=1023, text_bos_id=1022, seed=5)
    model = CLIPBasedMultiModalReIDModel(cfg)
    model.set_num_classes(got.n_clusters)
    heads = [v for k, v in model.state_dict().items() if k.startswith('bn_neck.') and v.dim() == 2]
    assert model.num_classes == got.n_clusters and heads and all(v.shape[0] == got.n_clusters for v in heads)


def test_rerank_scores_is_untouched_by_the_pooled_form():
    # the two-set form before and after a pooled re-ranker was built in the same process, against the constructor used directly
    from prcv2025reid_amd.rerank import Reranker, RerankParams, SparseReranker, rerank_scores
    X, _, _ = R.gaussian_fixture(422, 32, 219, 64, 24, 2.2)
    Xd = dev(X)
    for sparse, cls in ((False, Reranker), (True, SparseReranker)):
        params = RerankParams(8, 3, 0.3, sparse=sparse)
        direct = cls(Xd[:32], Xd[32:], params).rows(0, 32)
        cls.for_pool(Xd, params).rows(0, 5)
        chunks = list(rerank_scores(Xd[:32], Xd[32:], params, normalized=True, chunk=20))
        assert [a for a, _ in chunks] == [0, 20]
        got = torch.cat([S for _, S in chunks])
        assert torch.equal(got[:, :219].view(torch.int32), direct[:, :219].view(torch.int32))
        with pytest.raises(Exception, match='at least one query and one gallery row'):
            cls(Xd[:0], Xd, params)
