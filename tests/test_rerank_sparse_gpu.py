"""GPU: the sparse form of k-reciprocal re-ranking (RerankParams(sparse=True)): its four entry points against the dense kernels bit
for bit and against the fp64 restatements (tests/rerank_ref.py, tests/rerank_sparse_ref.py) within the gate of test_rerank_gpu.py,
``rerank_scores``, the evaluator / CSV hooks, and a pooled problem of 65 552 rows, which the dense form refuses.

The fixtures, their references and the gate are test_rerank_gpu.py's (computed once per session and shared).  Sizes are the
smallest at which the logic can break: N = 251 .. 385 pooled rows, lists of 2 .. 65 entries, merges of up to 21 lists, a CSC column
longer than the 128 threads that walk it."""
import functools

import numpy as np
import pytest
import torch

import rerank_ref as R
import rerank_sparse_ref as RS
from helpers import is_sentinel, sentinel_buffer
from test_rerank_gpu import EPS32, LAMBDA, assert_lists_are_settled, dev, eval_case, fixture, flavor, reference  # noqa: F401

pytestmark = pytest.mark.gpu
MARK = -7777                                                     # sentinel of the int32 outputs


def bits(t):
    return t.contiguous().view(torch.int32)


def weights_both(X, nbr, k1, pad=3):
    """(dense V [N, N], vcols, vvals, vcnt) of the two weights kernels on the same lists; the sparse outputs in sentinel buffers."""
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.rerank import list_width
    N = X.shape[0]
    Vd = torch.empty(N, (N + 3) // 4 * 4, device='cuda')
    ops.rerank_weights(nbr, X, Vd, k1)
    ldw = list_width(k1) + pad
    vcols = torch.full((N, ldw), MARK, dtype=torch.int32, device='cuda')
    vvals = sentinel_buffer(N, ldw, torch.float32)
    vcnt = torch.full((N,), MARK, dtype=torch.int32, device='cuda')
    ops.rerank_weights_sparse(nbr, X, vcols, vvals, vcnt, k1)
    torch.cuda.synchronize()
    return Vd[:, :N], vcols, vvals, vcnt


def scatter_padded(vcols, vvals, vcnt, N):
    live = torch.arange(vcols.shape[1], device='cuda')[None, :] < vcnt[:, None]
    D = torch.zeros(N, N, device='cuda')
    rows = torch.arange(N, device='cuda')[:, None].expand_as(vcols)
    D[rows[live], vcols[live].long()] = vvals[live]
    return D, live


def scatter_csr(rowptr, cols, vals, N, width):
    D = torch.zeros(N, width, device='cuda')
    rows = torch.repeat_interleave(torch.arange(N, device='cuda'), rowptr[1:] - rowptr[:-1])
    D[rows, cols[:rows.shape[0]].long()] = vals[:rows.shape[0]]
    return D


# ------------------------------------------------------------------------------------------------------------- 1. weights
@pytest.mark.parametrize('name,k1', [(n, k) for n in ('exact', 'gauss') for k in (1, 6, 8, 20)] + [('gauss2', 64)])
def test_padded_rows_hold_the_dense_weights(name, k1):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.rerank import list_width
    X, r64, _ = reference(name, k1, 1, far_row=name != 'gauss2')
    N, W = X.shape[0], list_width(k1)
    assert name != 'gauss2' or (N, W) == (385, 2210)
    nbr = dev(r64['nbr'][:, :k1 + 1], torch.int32)
    Vd, vcols, vvals, vcnt = weights_both(dev(X), nbr, k1)
    cnt = vcnt.cpu().numpy()
    assert cnt.tolist() == [len(m) for m in r64['Rstar']]
    got_cols = vcols.cpu().numpy()
    for i in range(N):
        assert sorted(got_cols[i, :cnt[i]].tolist()) == sorted(r64['Rstar'][i]), i           # once each: equal as sorted lists
    D, live = scatter_padded(vcols, vvals, vcnt, N)
    assert torch.equal(bits(D), bits(Vd))                                                     # the dense kernel's V bit for bit
    assert bool((vcols[~live] == MARK).all()) and bool(is_sentinel(vvals)[~live].all())       # positions >= vcnt[i], columns >= W
    assert int(live[:, W:].sum()) == 0
    again = weights_both(dev(X), nbr, k1)
    assert torch.equal(again[1], vcols) and torch.equal(bits(again[2]), bits(vvals)) and torch.equal(again[3], vcnt)


# ------------------------------------------------------------------------------------------------------------- 2. expand
def expand_sparse(vcols, vvals, vcnt, nbr, k1, k2, tail=8):
    from prcv2025reid_amd import ops
    N = vcnt.shape[0]
    cnt = torch.full((N,), MARK, dtype=torch.int32, device='cuda')
    ops.rerank_expand_count(vcols, vvals, vcnt, nbr, cnt, k1, k2)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device='cuda'), cnt.long().cumsum(0)])
    nnz = int(rowptr[-1])
    cols = torch.full((nnz + tail,), MARK, dtype=torch.int32, device='cuda')
    vals = sentinel_buffer(1, nnz + tail, torch.float32)[0]
    ops.rerank_expand_sparse(vcols, vvals, vcnt, nbr, rowptr, cols, vals, k1, k2)
    torch.cuda.synchronize()
    return cnt, rowptr, cols, vals, nnz


@pytest.mark.parametrize('name', ['exact', 'gauss'])
def test_csr_rows_hold_the_dense_expansion(name):
    from prcv2025reid_amd import ops
    X, r64, _ = reference(name)
    k1 = fixture(name)[4]
    N = X.shape[0]
    nbr = dev(r64['nbr'][:, :k1 + 1], torch.int32)
    Vd, vcols, vvals, vcnt = weights_both(dev(X), nbr, k1, pad=0)
    Vd = Vd.contiguous() if N % 4 == 0 else torch.nn.functional.pad(Vd, (0, 4 - N % 4)).contiguous()
    for k2 in (1, 3, 6, k1 + 1):
        V2d = torch.empty_like(Vd)
        ops.rerank_expand(Vd, nbr, V2d, k1, k2)
        cnt, rowptr, cols, vals, nnz = expand_sparse(vcols, vvals, vcnt, nbr, k1, k2)
        assert int(rowptr[0]) == 0 and bool((rowptr[1:] >= rowptr[:-1]).all())
        assert cnt.cpu().tolist() == [int(n) for n in (r64['V'][r64['nbr'][:, :k2]].sum(1) != 0).sum(1)]
        assert bool((cols[nnz:] == MARK).all()) and bool(is_sentinel(vals[nnz:]).all())        # nothing past rowptr[N]
        c, rp = cols[:nnz].cpu().numpy(), rowptr.cpu().numpy()
        inner = np.ones(nnz, bool); inner[rp[:-1][rp[:-1] < nnz]] = False                      # not the first entry of a row
        assert (c[1:][inner[1:]] > c[:-1][inner[1:]]).all() and c.min() >= 0 and c.max() < N   # strictly ascending inside a row
        assert bool((vals[:nnz] > 0).all())
        D = scatter_csr(rowptr, cols, vals, N, Vd.shape[1])
        assert torch.equal(bits(D[:, :N]), bits(V2d[:, :N])), k2                               # the dense kernel's V2 bit for bit
        if k2 == 1:
            assert torch.equal(bits(D[:, :N]), bits(Vd[nbr[:, 0].long(), :N]))
        again = expand_sparse(vcols, vvals, vcnt, nbr, k1, k2)
        assert torch.equal(again[0], cnt) and torch.equal(again[2], cols) and torch.equal(bits(again[3]), bits(vals))


# ------------------------------------------------------------------------------------------------------------- 3. jaccard
def csr_of(M):
    r, c = np.nonzero(M)
    ptr = np.concatenate([[0], np.cumsum((M != 0).sum(1))]).astype(np.int64)
    return dev(ptr), dev(c.astype(np.int32)), dev(M[r, c])


def planted_rows(rng, nq, Ng, N):
    """A [nq, N], B [Ng, N] with 12 non-zeros per row in columns < N - 3; columns N - 3 and N - 2 belong to one query alone,
    column N - 1 is in every gallery row but the empty one."""
    A = np.zeros((nq, N), np.float32); A[:, :N - 3] = R.sparse_rows(rng, nq, N - 3, 12)
    B = np.zeros((Ng, N), np.float32); B[:, :N - 3] = R.sparse_rows(rng, Ng, N - 3, 12)
    B[:, N - 1] = 0.03125
    A[0, N - 1] = 0.0625                                     # the hub column is walked by query 0 (and 3)
    B[Ng // 2] = A[0]                                        # m = sum of the row
    B[0] = 0                                                 # an empty gallery row
    if nq >= 5:
        A[1] = 0                                             # no non-zeros
        A[2] = 0; A[2, N - 3] = 0.25; A[2, N - 2] = 0.75     # columns no gallery row holds
        A[3, N - 1] = 0.125
    return A, B


@pytest.mark.parametrize('Ng', [3, 219, 257])
@pytest.mark.parametrize('nq', [1, 5, 70])
def test_sparse_jaccard_on_free_standing_matrices(nq, Ng):
    from prcv2025reid_amd import ops
    for N in (251, 320):
        rng = np.random.default_rng(1000 * nq + Ng + N)
        A, B = planted_rows(rng, nq, Ng, N)
        assert Ng < 257 or (B[:, N - 1] != 0).sum() > 128    # a column list longer than the workgroup that walks it
        cos = rng.uniform(-1, 1, (nq, Ng)).astype(np.float32)
        rowptr, cols, vals = csr_of(A)
        colptr, rows, cvals = csr_of(np.ascontiguousarray(B.T))
        lda = (N + 3) // 4 * 4
        At = torch.zeros(nq, lda, device='cuda'); At[:, :N] = dev(A)
        Bt = torch.zeros(Ng, lda, device='cuda'); Bt[:, :N] = dev(B)
        ldo = (Ng + 3) // 4 * 4 + 8                             # ldo > Ng
        for lam in (0.0, 0.3, 1.0):
            want = R.jaccard_ref(A, B, cos, lam)
            gate = max(8 * float(np.abs(want - R.jaccard_ref(A, B, cos, lam, np.float32)).max()), 4 * EPS32)
            out = sentinel_buffer(nq, ldo, torch.float32)
            ops.rerank_jaccard_sparse(rowptr, cols, vals, colptr, rows, cvals, dev(cos), out, Ng, lam)
            dense = torch.empty(nq, ldo, device='cuda')
            ops.rerank_jaccard(At, Bt, dev(cos), dense, Ng, N, lam)
            torch.cuda.synchronize()
            assert bool(is_sentinel(out[:, Ng:]).all())         # columns >= Ng are not written
            got = out[:, :Ng].cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - want).max())
            err_dense = float((out[:, :Ng] - dense[:, :Ng]).abs().max())
            print(f'  sparse jaccard nq={nq} Ng={Ng} N={N} lam={lam}: |s - ref| = {err:.3e}, |s - dense| = {err_dense:.3e}, gate {gate:.3e}')
            assert err <= gate and err_dense <= gate, (N, lam, err, err_dense, gate)
            if lam == 0.0:
                assert want[0, Ng // 2] >= 1.0                  # the pair of equal rows: m = the row's sum
            plain = np.float32(lam) * cos                       # m = 0: the fp32 product lambda cos itself (as values: at lambda = 0 its zero is +0)
            assert plain.dtype == got.dtype == np.float32 and np.array_equal(got[:, 0], plain[:, 0])      # the empty gallery row
            if nq >= 5:
                assert np.array_equal(got[1:3], plain[1:3])
                if lam:
                    assert np.array_equal(got[1:3].view(np.int32), plain[1:3].view(np.int32))
            again = sentinel_buffer(nq, ldo, torch.float32)
            ops.rerank_jaccard_sparse(rowptr, cols, vals, colptr, rows, cvals, dev(cos), again, Ng, lam)
            assert torch.equal(bits(again), bits(out))
            if nq >= 5:                                         # a chunk: rowptr + a, absolute offsets
                part = sentinel_buffer(nq - 3, ldo, torch.float32)
                ops.rerank_jaccard_sparse(rowptr[3:], cols, vals, colptr, rows, cvals, dev(cos[3:]), part, Ng, lam)
                assert torch.equal(bits(part), bits(out[3:]))


# ------------------------------------------------------------------------------------------------------------- 4. end to end
def settled_positions(s, gate):
    """[Nq, Ng] bool over the reference ranking's positions: the entry there is more than two gates from both neighbours, so every
    row within one gate of the reference has the same entry at that position."""
    order = R.ranking(s)
    v = np.take_along_axis(s, order, 1)
    far = np.ones(v.shape, bool)
    far[:, 1:] &= v[:, :-1] - v[:, 1:] > 2 * gate
    far[:, :-1] &= v[:, :-1] - v[:, 1:] > 2 * gate
    return order, far


def scores_of(Xd, Nq, Ng, params, chunk):
    from prcv2025reid_amd.rerank import rerank_scores
    got = torch.empty(Nq, Ng, device='cuda')
    for a, S in rerank_scores(Xd[:Nq], Xd[Nq:], params, normalized=True, chunk=chunk):
        assert S.shape[1] % 4 == 0 and S.shape[1] >= Ng and S.shape[0] <= chunk
        got[a:a + S.shape[0]] = S[:, :Ng]
    return got


@pytest.mark.parametrize('name', ['exact', 'gauss', 'gauss2'])
def test_sparse_rerank_scores_end_to_end(flavor, name):
    from prcv2025reid_amd.rerank import RerankParams
    X, r64, gate = reference(name)
    _, _, _, Nq, k1, k2 = fixture(name)
    assert_lists_are_settled(name, r64, k1)
    order, far = settled_positions(r64['s'], gate)
    assert far[:, :10].all() and far.mean() > 0.9               # the precondition: every top-10 and most of the rest are settled in the reference
    Xd, Ng = dev(X), X.shape[0] - Nq
    sparse = scores_of(Xd, Nq, Ng, RerankParams(k1, k2, LAMBDA, sparse=True), 7)
    dense = scores_of(Xd, Nq, Ng, RerankParams(k1, k2, LAMBDA), 20)
    got = sparse.cpu().numpy().astype(np.float64)
    err, err_dense = float(np.abs(got - r64['s']).max()), float((sparse - dense).abs().max())
    print(f'  sparse rerank_scores {name} {flavor}: |s* - ref| = {err:.3e}, |s* - dense| = {err_dense:.3e}, gate {gate:.3e}')
    assert err <= gate and err_dense <= gate
    idx = torch.sort(sparse, dim=1, descending=True, stable=True)[1].cpu().numpy()
    assert np.array_equal(idx[far], order[far])
    assert torch.equal(bits(scores_of(Xd, Nq, Ng, RerankParams(k1, k2, LAMBDA, sparse=True), 1024)), bits(sparse))


# ------------------------------------------------------------------------------------------------------------- 5. evaluator, CSV
def test_evaluator_and_csv_equal_the_dense_form(tmp_path, flavor):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams, SparseReranker
    X, qp, gp, Nq, k1, k2, r64, gate, g_img, q_img = eval_case()
    ev = ProtocolEvaluator(dev(X[Nq:]), torch.as_tensor(gp), g_img, normalized=True)
    Q, qpt = dev(X[:Nq]), torch.as_tensor(qp)
    assert isinstance(ev._reranker(Q, RerankParams(k1, k2, LAMBDA, sparse=True), True), SparseReranker)
    for masked in (True, False):
        got, want = (ev.rank_and_metrics(Q, qpt, q_img, ignore_same_img=masked, rerank=RerankParams(k1, k2, LAMBDA, sparse=s), chunk=8)
                     for s in (True, False))
        assert got['num_queries'] == want['num_queries'] > 0
        assert all(abs(got[k] - want[k]) <= 1e-6 for k in ('mAP', 'R@1', 'R@5', 'R@10')), (got, want)
    assert got != ev.rank_and_metrics(Q, qpt, q_img, ignore_same_img=False)                      # not the cosine ranking's
    keys = [f'q{i}' for i in range(Nq)]
    for s in (True, False):
        ev.export_submission_csv(Q, keys, g_img, str(tmp_path / f'{s}.csv'), top_k=10, rerank=RerankParams(k1, k2, LAMBDA, sparse=s), chunk=8)
    rows = (tmp_path / 'True.csv').read_text().strip().split('\n')
    assert len(rows) == Nq + 1 and rows == (tmp_path / 'False.csv').read_text().strip().split('\n')


# ------------------------------------------------------------------------------------------------------------- 6. N > 65 536
BIG = dict(seed=25, Nq=16, Ng=65536, D=64, nid=8192, noise=1.2, k1=6, k2=3)       # seed picked on the CPU for the asserted preconditions


@functools.lru_cache(maxsize=None)
def big_fixture():
    X = R.gaussian_fixture(BIG['seed'], BIG['Nq'], BIG['Ng'], BIG['D'], BIG['nid'], BIG['noise'])[0]
    sample = np.concatenate([np.arange(BIG['Nq']), BIG['Nq'] + (np.arange(256) * 257 + 11) % BIG['Ng']])
    S = X[sample].astype(np.float64) @ X.astype(np.float64).T                                   # brute force, the sampled rows only
    return X, sample, S


def test_pooled_rows_beyond_the_dense_limit():
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.rerank import RerankParams, SparseReranker, rerank_scores
    Nq, Ng, k1, k2 = BIG['Nq'], BIG['Ng'], BIG['k1'], BIG['k2']
    X, sample, S = big_fixture()
    assert R.min_gap_in_top(S, k1 + 3) >= 1e-5                  # the sampled lists are settled: fp32 cannot order them otherwise
    Xd = dev(X)
    with pytest.raises(_lib.ReidHipError, match='exceeds 65536 rows'):
        rerank_scores(Xd[:Nq], Xd[Nq:], RerankParams(k1, k2, LAMBDA), normalized=True)
    rr = SparseReranker(Xd[:Nq], Xd[Nq:], RerankParams(k1, k2, LAMBDA, sparse=True))
    nbr = rr.nbr.cpu().numpy()
    assert nbr.shape == (Nq + Ng, k1 + 1) and nbr.min() >= 0 and nbr.max() < Nq + Ng
    assert np.array_equal(nbr[sample], R.ranking(S)[:, :k1 + 1])
    r64 = RS.sparse_ref(X, nbr, Nq, k1, k2, LAMBDA)
    r32 = RS.sparse_ref(X, nbr, Nq, k1, k2, LAMBDA, np.float32)
    gate = RS.gate(r64, r32)
    assert 4 * EPS32 <= gate < 1e-5, gate
    assert int(((r64['m'] > 0).sum(1)).max()) >= 8              # a query shares columns with at least 8 gallery rows
    assert sum(len(a) > len(b) for a, b in zip(r64['Rstar'], r64['R'])) >= 100                  # the expansion does add members
    assert (rr.rowptr[1:] - rr.rowptr[:-1]).cpu().tolist() == [len(v) for v in r64['V2']]
    got = rr.rows(0, Nq)[:, :Ng].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - r64['s']).max())
    print(f'  N = {Nq + Ng}: max |s* - ref| = {err:.3e}, gate {gate:.3e}, nnz(V2) / N = {int(rr.rowptr[-1]) / (Nq + Ng):.1f}')
    assert err <= gate


# ------------------------------------------------------------------------------------------------------------- 7. errors
def test_sparse_argument_errors_launch_nothing():
    from prcv2025reid_amd import _lib, ops
    N, D, W = 256, 64, 9 * 6                                    # k1 = 8: W = 54
    X = torch.zeros(N, D, device='cuda')
    nbr = torch.zeros(N, 80, dtype=torch.int32, device='cuda')
    ints = torch.full((N, 2300), MARK, dtype=torch.int32, device='cuda')
    flts = sentinel_buffer(N, 2300, torch.float32)
    vcnt = torch.full((N,), MARK, dtype=torch.int32, device='cuda')
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device='cuda')
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_weights_sparse: k1=65 outside 1\.\.64'):
        ops.rerank_weights_sparse(nbr, X, ints, flts, vcnt, 65)
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_weights_sparse: .*ldw=53 \(ldw >= W = 54\)'):
        ops.rerank_weights_sparse(nbr, X, ints[:, :W - 1], flts[:, :W - 1].contiguous(), vcnt, 8)
    with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rerank_weights_sparse: null pointer'):
        _lib.check(_lib.lib().reid_rerank_weights_sparse(nbr.data_ptr(), 80, X.data_ptr(), D, None, flts.data_ptr(), vcnt.data_ptr(), 2300, N, D, 8, None))
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_expand_count: k1=64 k2=4 merge .* = 8840 entries per row, at most 8192'):
        ops.rerank_expand_count(ints, flts, vcnt, nbr, vcnt, 64, 4)
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_expand_sparse: k1=64 k2=65 merge'):
        ops.rerank_expand_sparse(ints, flts, vcnt, nbr, rowptr, ints, flts, 64, 65)
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_expand_sparse: k1=8 k2=10'):
        ops.rerank_expand_sparse(ints, flts, vcnt, nbr, rowptr, ints, flts, 8, 10)
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_expand_count: .*ldw=53'):
        _lib.check(_lib.lib().reid_rerank_expand_count(ints.data_ptr(), flts.data_ptr(), vcnt.data_ptr(), W - 1, nbr.data_ptr(), 80, vcnt.data_ptr(),
                                                       N, 8, 3, None))
    with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rerank_jaccard_sparse: null pointer'):
        _lib.check(_lib.lib().reid_rerank_jaccard_sparse(rowptr.data_ptr(), ints.data_ptr(), flts.data_ptr(), 10, rowptr.data_ptr(), ints.data_ptr(),
                                                         flts.data_ptr(), 10, None, 224, flts.data_ptr(), 2300, 32, 224, N, 0.3, None))
    with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rerank_jaccard_sparse: ldc=64 ldo=2300'):
        ops.rerank_jaccard_sparse(rowptr[:33], ints[0], flts[0], rowptr, ints[1], flts[1], X[:32], flts[:32], 2400, 0.3)
    torch.cuda.synchronize()
    assert bool((ints == MARK).all()) and bool(is_sentinel(flts).all()) and bool((vcnt == MARK).all())
