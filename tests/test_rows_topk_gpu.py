"""reid_rows_topk (csrc/select.hip) and the layers on top of it, on the GPU.  Every comparison is exact: indices equal, score bits
equal; the reference is rows_topk_ref.py (checked against torch's stable sort in test_rows_topk_cpu.py) or that sort itself.

The kernel changes path with the data, so the shapes are chosen by what they reach (SEL_CAP = 2048 candidates, digits 12 + 12 + 8):
one digit when everything from the crossing bin upward fits the buffer; two or three digits when a bin holds more; the column-ordered
walk when more than 2048 - above entries EQUAL the k-th key (families b, c, d at n >= 4099, g below never: it stops one step before)."""

import numpy as np
import pytest
import torch

import rows_topk_ref as T
from helpers import is_sentinel, sentinel_buffer
from test_rerank_gpu import LAMBDA, dev, eval_case, fixture, flavor  # noqa: F401

pytestmark = pytest.mark.gpu
MARK = -7777                                                      # sentinel of the int32 outputs
KS = (1, 2, 10, 100, 1024)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 20003)


def roundup4(n):
    return (n + 3) // 4 * 4


# ---- value families: one float32 row of n entries each -----------------------------------------------------------------------------
def fam_normals(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def fam_quarters(rng, n):                                          # 9 values: long tie runs cross every cut
    return (rng.integers(-4, 5, n) * 0.25).astype(np.float32)


def fam_zeros(rng, n):
    return np.zeros(n, np.float32)


def fam_lambda0(rng, n):                                           # exact zeros but 37 positive entries, some equal
    row = np.zeros(n, np.float32)
    at = rng.choice(n, min(37, n), replace=False)
    row[at] = rng.integers(1, 12, len(at)).astype(np.float32) / 32
    return row


def fam_adjacent(rng, n):                                          # 1 + j 2^-23, permuted: the top 12 key bits never separate them
    return (np.uint32(0x3f800000) + rng.permutation(n).astype(np.uint32)).view(np.float32)


def fam_specials(rng, n):
    row = rng.standard_normal(n).astype(np.float32)
    specials = np.array([0x80000000, 0, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x00000001, 0x80000001, 0x007fffff,
                         0xc0000000, 0xbf800000], np.uint32).view(np.float32)
    where = rng.random(n) < 0.3
    row[where] = specials[rng.integers(0, len(specials), int(where.sum()))]
    return row


def fam_adjacent_ties(rng, n):                                     # 300 neighbouring floats, each many times: all three digits, no walk
    return (np.uint32(0x3f800000) + rng.integers(0, 300, n).astype(np.uint32)).view(np.float32)


FAMILIES = (fam_normals, fam_quarters, fam_zeros, fam_lambda0, fam_adjacent, fam_specials, fam_adjacent_ties)
PAD = np.array([0x7f800000, 0x7fc00000, 0x7149f2ca], np.uint32).view(np.float32)      # +inf, NaN, 1e30: row q's padding columns


def padded(rows, extra=4):
    """[nq, roundup4(n) + extra] with PAD[q % 3] in the columns >= n."""
    nq, n = rows.shape
    S = np.empty((nq, roundup4(n) + extra), np.float32)
    S[:] = PAD[np.arange(nq) % 3][:, None]
    S[:, :n] = rows
    return S


def assert_lists(got, want, what):
    (gi, gs), (wi, ws) = got, want
    gi, gs = gi.cpu().numpy(), gs.cpu().numpy()
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5])
    assert np.array_equal(T.bits(gs), T.bits(ws)), what


# ---- 1. shape sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_shape_sweep(n):
    from prcv2025reid_amd import ops
    rng = np.random.default_rng(1000 + n)
    for fam in FAMILIES:
        S = padded(np.stack([fam(rng, n) for _ in range(3)]))
        assert S.shape[1] == roundup4(n) + 4
        wi, ws = T.rows_topk_ref(S, n, max(KS))                  # a shorter list is a prefix of the longest
        Sd = dev(S)
        for k in KS:
            assert_lists(ops.rows_topk(Sd, n, k), (wi[:, :k], ws[:, :k]), (fam.__name__, n, k))
        if fam is fam_zeros:
            assert np.array_equal(wi[0, :min(n, 1024)], np.arange(min(n, 1024)))


# ---- 2. exclusion -----------------------------------------------------------------------------------------------------------------------
def test_exclusion():
    from prcv2025reid_amd import ops
    n, rng = 1025, np.random.default_rng(7)
    rows = np.stack([fam_normals(rng, n), fam_quarters(rng, n), fam_lambda0(rng, n), fam_specials(rng, n), fam_normals(rng, n),
                     fam_zeros(rng, n)])
    g_img = rng.integers(-1, 40, n).astype(np.int32)
    top = int(np.argmax(rows[4]))
    g_img[top] = 11
    q_excl = np.array([[-1, -1, -1, -1], [3, -1, -1, -1], [-1, 5, -1, 7], [1, 2, 3, 4], [11, -1, -1, -1], [-1, -1, -1, 39]], np.int32)
    assert (g_img == -1).any() and all((g_img == i).any() for i in (3, 4, 5, 7, 11, 39))
    S = padded(rows)
    Sd, gd, ed = dev(S), dev(g_img), dev(q_excl)
    for k in (10, 100, 1024):
        want = T.rows_topk_ref(S, n, k, g_img, q_excl)
        assert top not in want[0][4] and np.array_equal(want[0][0], T.rows_topk_ref(S, n, k)[0][0])
        assert_lists(ops.rows_topk(Sd, n, k, gd, ed), want, k)
        if k == 1024:                                             # image id -1 is never dropped
            assert np.isin(np.flatnonzero(g_img == -1), want[0][0]).all()
        plain = T.rows_topk_ref(S, n, k)
        assert_lists(ops.rows_topk(Sd, n, k, gd, None), plain, k)         # one of the two alone masks nothing
        assert_lists(ops.rows_topk(Sd, n, k, None, ed), plain, k)
    # three eligible columns at k = 10: seven -1 / -inf entries
    g2 = rng.integers(0, 4, n).astype(np.int32)
    g2[[17, 600, 1024]] = [-1, 9, -1]
    e2 = np.tile(np.array([[0, 1, 2, 3]], np.int32), (6, 1))
    want = T.rows_topk_ref(S, n, 10, g2, e2)
    assert (np.sort(want[0][:, :3], 1) == [17, 600, 1024]).all() and (want[0][:, 3:] == -1).all() and np.isneginf(want[1][:, 3:]).all()
    assert_lists(ops.rows_topk(Sd, n, 10, dev(g2), dev(e2)), want, 'three left')
    with pytest.raises(ValueError, match='n=1025 columns asked of'):                # a narrowed view does not reach past itself
        ops.rows_topk(Sd[:, :1000], n, 10)


def test_exclusion_inside_the_tie_walk():
    """Masking where the cut lies in a tie block beyond the buffer: all three digits, then the column-ordered walk (n = 4099 zeros)."""
    from prcv2025reid_amd import ops
    n, rng = 4099, np.random.default_rng(17)
    rows = np.stack([fam_zeros(rng, n), fam_lambda0(rng, n), fam_quarters(rng, n), fam_lambda0(rng, n)])
    g_img = rng.integers(-1, 6, n).astype(np.int32)               # every id masks about a seventh of the columns
    g_img[:8] = [0, 1, 2, 3, 4, 5, -1, 0]                         # the first columns of the zero block: some dropped, some kept
    q_excl = np.array([[0, 2, -1, 4], [5, -1, -1, -1], [-1, -1, 1, 3], [-1, -1, -1, -1]], np.int32)
    S = padded(rows)
    Sd, gd, ed = dev(S), dev(g_img), dev(q_excl)
    for k in (100, 1024):
        want = T.rows_topk_ref(S, n, k, g_img, q_excl)
        assert want[0][0, :4].tolist() == [1, 3, 5, 6] and (want[0] >= 0).all()
        assert not np.array_equal(want[0][:3], T.rows_topk_ref(S, n, k)[0][:3])
        assert_lists(ops.rows_topk(Sd, n, k, gd, ed), want, k)


# ---- 3. more rows than compute units --------------------------------------------------------------------------------------------------------
def test_rows_are_independent():
    from prcv2025reid_amd import ops
    nq, n, k, rng = 300, 4099, 100, np.random.default_rng(3)
    S = padded(np.stack([FAMILIES[q % len(FAMILIES)](rng, n) for q in range(nq)]))
    assert_lists(ops.rows_topk(dev(S), n, k), T.rows_topk_ref(S, n, k), 'rows')


# ---- 4. the protocol's row length -------------------------------------------------------------------------------------------------------------
def test_protocol_size_rows():
    from prcv2025reid_amd import ops
    nq, n, rng = 8, 200000, np.random.default_rng(5)
    fams = (fam_normals, fam_zeros, fam_lambda0)
    Sd = dev(np.stack([fams[q % 3](rng, n) for q in range(nq)]))
    assert Sd.stride(0) == n
    rows = Sd.cpu()                                               # the CPU sort of the copied rows
    order = torch.sort(rows, dim=1, descending=True, stable=True)[1]
    for k in (100, 1024):
        want = (order[:, :k].numpy().astype(np.int32), torch.gather(rows, 1, order[:, :k]).numpy())
        assert_lists(ops.rows_topk(Sd, n, k), want, k)
    assert np.array_equal(order[1, :1024].numpy(), np.arange(1024))


# ---- 5. outputs inside sentinel buffers ---------------------------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_buffers():
    from prcv2025reid_amd import _lib, ops
    nq, n, k, pad, rng = 5, 4099, 100, 64, np.random.default_rng(9)
    S = padded(np.stack([FAMILIES[q](rng, n) for q in range(nq)]))
    Sd = dev(S)
    want = T.rows_topk_ref(S, n, k)

    def buffers():
        ints = torch.full((nq * k + 2 * pad,), MARK, dtype=torch.int32, device='cuda')
        flts = sentinel_buffer(1, nq * k + 2 * pad, torch.float32)[0]
        return ints, flts, (ints[pad:pad + nq * k].view(nq, k), flts[pad:pad + nq * k].view(nq, k))

    def untouched(ints, flts):
        return (bool((ints[:pad] == MARK).all()) and bool((ints[-pad:] == MARK).all()) and bool(is_sentinel(flts[:pad]).all())
                and bool(is_sentinel(flts[-pad:]).all()))
    ints, flts, out = buffers()
    got = ops.rows_topk(Sd, n, k, out=out)
    assert got[0].data_ptr() == out[0].data_ptr()
    assert_lists(got, want, 'first call')
    assert untouched(ints, flts)
    ints2, flts2, out2 = buffers()
    ops.rows_topk(Sd, n, k, out=out2)
    assert torch.equal(ints, ints2) and torch.equal(flts.view(torch.int32), flts2.view(torch.int32))
    # refused calls write nothing
    ints3, flts3, out3 = buffers()
    ld = Sd.stride(0)
    for args, msg in (((Sd.data_ptr(), ld, nq, n, 1025), r'k=1025 outside 1\.\.1024'), ((Sd.data_ptr(), ld, nq, n, 0), 'k=0 outside'),
                      ((Sd.data_ptr(), n - 3, nq, n, k), 'ld='), ((Sd.data_ptr(), ld - 2, nq, n, k), 'ld='),
                      ((Sd.data_ptr() + 4, ld, nq, n, k), '16-byte aligned')):
        with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rows_topk: .*' + msg):
            _lib.check(_lib.lib().reid_rows_topk(*args, None, None, out3[0].data_ptr(), out3[1].data_ptr(), _lib.stream_ptr()))
    with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rows_topk: null pointer'):
        _lib.check(_lib.lib().reid_rows_topk(Sd.data_ptr(), ld, nq, n, k, None, None, None, out3[1].data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((ints3 == MARK).all()) and bool(is_sentinel(flts3).all())


# ---- 6. re-ranking lists --------------------------------------------------------------------------------------------------------------------------
def cpu_lists(S, Ng, k):
    """The first k of the CPU's stable descending sort of S[:, :Ng] (a float32 device tensor), filled to k with -1 / -inf."""
    rows = S[:, :Ng].cpu()
    order = torch.sort(rows, dim=1, descending=True, stable=True)[1][:, :k]
    idx = np.full((rows.shape[0], k), -1, np.int32)
    score = np.full((rows.shape[0], k), -np.inf, np.float32)
    idx[:, :order.shape[1]] = order.numpy()
    score[:, :order.shape[1]] = torch.gather(rows, 1, order).numpy()
    return idx, score


@pytest.mark.parametrize('lam', [LAMBDA, 0.0, 1.0])
@pytest.mark.parametrize('name', ['gauss', 'gauss2'])
def test_rerank_lists_are_the_sorted_rows(flavor, name, lam):
    from prcv2025reid_amd.rerank import Reranker, RerankParams, SparseReranker, rerank_scores, rerank_topk
    X, _, _, Nq, k1, k2 = fixture(name)
    Ng = X.shape[0] - Nq
    Xd = dev(X)
    k = 200 if (name == 'gauss' and lam == 0.0) else 100
    for sparse in (False, True):
        params = RerankParams(k1, k2, lam, sparse=sparse)
        S = torch.cat([s for _, s in rerank_scores(Xd[:Nq], Xd[Nq:], params, normalized=True, chunk=20)], 0)
        if lam == 0.0 and name == 'gauss':                        # the cut lies inside the block of exact zeros
            positive = (S[:, :Ng] > 0).sum(1)
            assert int(positive.max()) < k < Ng and bool((S[:, :Ng] >= 0).all()), (int(positive.min()), int(positive.max()))
        want = cpu_lists(S, Ng, k)
        rr = (SparseReranker if sparse else Reranker)(Xd[:Nq], Xd[Nq:], params)
        assert_lists(rr.topk(0, Nq, k), want, (name, lam, sparse, 'topk'))
        part = rr.topk(5, 17, k)
        assert_lists(part, (want[0][5:17], want[1][5:17]), (name, lam, sparse, 'topk of a slice'))
        got = rerank_topk(Xd[:Nq], Xd[Nq:], params, k=k, normalized=True, chunk=20)
        assert got[0].shape == (Nq, k) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
        assert_lists(got, want, (name, lam, sparse, 'rerank_topk'))


# ---- 7. ranked_lists against the metrics kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_ids', [True, False])
@pytest.mark.parametrize('reranked', [True, False])
def test_ranked_lists_agree_with_rank_metrics(flavor, reranked, with_ids):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams
    X, qp, gp, Nq, k1, k2, _, _, g_img, q_img = eval_case()
    Ng = len(gp)
    ev = ProtocolEvaluator(dev(X[Nq:]), torch.as_tensor(gp), g_img, normalized=True)
    Q, qpt = dev(X[:Nq]), torch.as_tensor(qp)
    kw = dict(q_img_ids=q_img if with_ids else None, chunk=8, normalized=True, rerank=RerankParams(k1, k2, LAMBDA) if reranked else None)
    ap, rank1, npos = (t.cpu().numpy() for t in ev.per_query(Q, qpt, **kw))
    masked = [set(int(n[1:]) for n in q_img[i]) if with_ids else set() for i in range(Nq)]
    assert not with_ids or any(gp[j] == qp[i] for i in range(Nq) for j in masked[i])       # the mask does remove positives
    for k in (10, Ng):
        idx, score = (t.cpu().numpy() for t in ev.ranked_lists(Q, k=k, **kw))
        assert idx.shape == score.shape == (Nq, k)
        for i in range(Nq):
            live = idx[i][idx[i] >= 0]
            assert not masked[i] & set(live.tolist())                                  # no excluded image in a list
            hits = np.flatnonzero(gp[live] == qp[i])
            if npos[i] > 0 and rank1[i] <= k:
                assert hits[0] == rank1[i] - 1, (i, k)
            elif npos[i] > 0:
                assert hits.size == 0
            if k == Ng:
                assert sorted(live.tolist()) == sorted(set(range(Ng)) - masked[i]) and (idx[i, len(live):] == -1).all()
                assert len(hits) == npos[i]
                if npos[i] > 0:                                   # the same double terms, summed in another order
                    want = float(np.mean((np.arange(len(hits)) + 1.0) / (hits + 1.0)))
                    assert abs(want - ap[i]) <= npos[i] * 2.0 ** -52 * want, (i, want, ap[i])
        # scores are the rows' own bits, in ranking order
        assert (T.order_key(score)[:, :-1].astype(np.int64) >= T.order_key(score)[:, 1:].astype(np.int64)).all()


# ---- 8. CSV -------------------------------------------------------------------------------------------------------------------------------------------
def csv_rows(path, Nq):
    rows = path.read_text().strip().split('\n')
    assert rows[0] == 'query_key,ranked_gallery_ids' and len(rows) == Nq + 1
    return rows[1:]


@pytest.mark.parametrize('sparse', [False, True])
def test_csv_lists_the_whole_gallery_when_top_k_exceeds_it(tmp_path, flavor, sparse):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams
    X, _, gp, Nq, k1, k2 = fixture('gauss2')
    Ng = X.shape[0] - Nq
    assert Ng == 337
    names = [f'g{j}' for j in range(Ng)]
    ev = ProtocolEvaluator(dev(X[Nq:]), torch.as_tensor(gp), names, normalized=True)
    params = RerankParams(k1, k2, LAMBDA, sparse=sparse)
    keys = [f'q{i}' for i in range(Nq)]
    ev.export_submission_csv(dev(X[:Nq]), keys, names, str(tmp_path / 'rr.csv'), top_k=400, rerank=params, chunk=20)
    want = cpu_lists(ev._reranker(dev(X[:Nq]), params).rows(0, Nq), Ng, Ng)[0]
    for i, row in enumerate(csv_rows(tmp_path / 'rr.csv', Nq)):
        assert row == f'q{i},' + ' '.join(f'g{j}' for j in want[i]), i


def test_csv_takes_host_features_and_an_empty_top_k(tmp_path):
    """``export_submission_csv(..., rerank=...)`` moves host-resident query features to the device itself, as its other branches do,
    and top_k = 0 still writes empty lists."""
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams
    X, _, gp, Nq, k1, k2 = fixture('gauss')
    Ng = X.shape[0] - Nq
    names = [f'g{j}' for j in range(Ng)]
    ev = ProtocolEvaluator(dev(X[Nq:]), torch.as_tensor(gp), names, normalized=True)
    params = RerankParams(k1, k2, LAMBDA)
    keys = [f'q{i}' for i in range(Nq)]
    Q = torch.as_tensor(X[:Nq])
    assert not Q.is_cuda
    ev.export_submission_csv(Q, keys, names, str(tmp_path / 'host.csv'), top_k=10, rerank=params)
    ev.export_submission_csv(Q.cuda(), keys, names, str(tmp_path / 'dev.csv'), top_k=10, rerank=params)
    assert (tmp_path / 'host.csv').read_bytes() == (tmp_path / 'dev.csv').read_bytes()
    assert all(len(row.split(',')[1].split(' ')) == 10 for row in csv_rows(tmp_path / 'host.csv', Nq))
    ev.export_submission_csv(Q, keys, names, str(tmp_path / 'none.csv'), top_k=0, rerank=params)
    assert csv_rows(tmp_path / 'none.csv', Nq) == [f'q{i},' for i in range(Nq)]


def test_csv_beyond_the_list_limit_keeps_the_sort(tmp_path):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams
    g = torch.Generator().manual_seed(31)
    Nq, Ng, top_k = 24, 1100, 1030
    X = torch.nn.functional.normalize(torch.randn(Nq + Ng, 64, generator=g), dim=1).cuda()
    names = [f'g{j}' for j in range(Ng)]
    ev = ProtocolEvaluator(X[Nq:], torch.arange(Ng) // 4, names, normalized=True)
    params = RerankParams(8, 3, LAMBDA)
    keys = [f'q{i}' for i in range(Nq)]
    ev.export_submission_csv(X[:Nq], keys, names, str(tmp_path / 'rr.csv'), top_k=top_k, rerank=params, chunk=16)
    want = cpu_lists(ev._reranker(X[:Nq], params).rows(0, Nq), Ng, top_k)[0]
    for i, row in enumerate(csv_rows(tmp_path / 'rr.csv', Nq)):
        assert row == f'q{i},' + ' '.join(f'g{j}' for j in want[i]), i
