"""GPU: the three re-ranking kernels, ``rerank_scores`` and the evaluator / CSV hooks against the fp64 restatement of the definition
(tests/rerank_ref.py).  Discrete outputs (sets, lists) must be identical; continuous ones lie within a gate measured on the
reference alone: 8 x max |fp64 - fp32 numpy| of the same fixture, at least 4 fp32 ulps of 1.

Sizes are the smallest at which the logic can break: N = 251 / 256 / 385 pooled rows (no multiple of the 128-row tile or of the
16-column k-step, more than one tile), lists of k1 + 1 = 2 .. 21, exact ties in every list of the exact fixture."""
import functools

import numpy as np
import pytest
import torch

import rerank_ref as R
from helpers import is_sentinel, sentinel_buffer

pytestmark = pytest.mark.gpu

# name -> (rows, query pids, gallery pids, Nq, k1, k2): seeds picked on the CPU for the preconditions the tests assert
FIXTURES = {
    'exact': lambda: R.exact_fixture(0) + (32, 20, 6),
    'gauss': lambda: R.gaussian_fixture(422, 32, 219, 64, 24, 2.2) + (32, 8, 3),
    'gauss2': lambda: R.gaussian_fixture(2541, 48, 337, 128, 32, 1.2) + (48, 20, 6),
    'eval': lambda: R.gaussian_fixture(2908, 12, 117, 64, 24, 2.2) + (12, 8, 3),
}
LAMBDA = 0.3
EPS32 = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def fixture(name):
    X, qp, gp, Nq, k1, k2 = FIXTURES[name]()
    return np.ascontiguousarray(X, dtype=np.float32), qp, gp, Nq, k1, k2


def far_from(X):
    """A unit row whose largest cosine to any row of X is as low as a perceptron pass gets it (low enough on the fixtures that no row lists it)."""
    X64 = X.astype(np.float64)
    far = np.linalg.lstsq(X64, -np.ones(X.shape[0]), rcond=None)[0]
    for _ in range(4000):
        far /= np.linalg.norm(far)
        far -= 0.02 * X64[int(np.argmax(X64 @ far))]
    return (far / np.linalg.norm(far)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, k1=None, k2=None, far_row=False):
    """(rows, fp64 reference, gate) of a fixture, computed once and shared; ``far_row`` appends a row nobody lists."""
    X, _, _, Nq, k1_, k2_ = fixture(name)
    k1, k2 = k1 or k1_, k2 or k2_
    if far_row:
        X = np.concatenate([X, far_from(X)[None]], 0)
    r64 = R.rerank_ref(X, Nq, k1, k2, LAMBDA)
    r32 = R.rerank_ref(X, Nq, k1, k2, LAMBDA, np.float32, nbr=r64['nbr'])
    gate = R.gate(r64, r32)
    assert 4 * EPS32 <= gate < 1e-5, gate
    return X, r64, gate


@pytest.fixture(params=['bf16', 'f16'])
def flavor(request):
    from prcv2025reid_amd import _lib
    _lib.set_flavor(request.param)
    yield request.param
    _lib.set_flavor('bf16')


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def assert_lists_are_settled(name, r64, k1):
    """The fp64 similarities inside the first k1 + 3 of every pooled row are >= 1e-5 apart (Gaussian fixtures), or every product is
    exact in fp32 (exact fixture): no legitimate fp32 ranking can then differ from the reference's inside the lists that are read."""
    if name == 'exact':
        X = fixture(name)[0]
        assert np.array_equal((X @ X.T).astype(np.float64), r64['cos'])
    else:
        assert R.min_gap_in_top(r64['cos'], k1 + 3) >= 1e-5


# ------------------------------------------------------------------------------------------------------------- 1. weights
@pytest.mark.parametrize('k1', [1, 6, 8, 20])
@pytest.mark.parametrize('name', ['exact', 'gauss'])
def test_weights_match_the_reference_sets_and_values(name, k1):
    from prcv2025reid_amd import ops
    X, r64, gate = reference(name, k1, 1, far_row=True)
    N = X.shape[0]
    assert r64['Rstar'][N - 1] == [N - 1]                       # the appended row: in nobody's list, so alone in its own R*
    if k1 >= 6:
        assert sum(len(a) > len(b) for a, b in zip(r64['Rstar'], r64['R'])) > 10      # the expansion does add members
    nbr = dev(r64['nbr'][:, :k1 + 1], torch.int32)              # the kernel reads the lists it is given: the sets must be identical
    ld = (N + 3) // 4 * 4 + 4
    V = sentinel_buffer(N, ld, torch.float32)
    ops.rerank_weights(nbr, dev(X), V, k1)
    torch.cuda.synchronize()
    assert bool(is_sentinel(V[:, N:]).all())                    # columns >= N are not the call's
    got = V[:, :N].cpu().numpy().astype(np.float64)
    assert np.array_equal(got != 0, r64['V'] != 0)
    err = float(np.abs(got - r64['V']).max())
    print(f'  weights {name} k1={k1}: max |V - ref| = {err:.3e}, gate {gate:.3e}')
    assert err <= gate
    assert got[N - 1, N - 1] == 1.0
    V2 = torch.empty_like(V)
    ops.rerank_weights(nbr, dev(X), V2, k1)
    assert torch.equal(V[:, :N], V2[:, :N])                     # deterministic


# ------------------------------------------------------------------------------------------------------------- 2. expand
@pytest.mark.parametrize('name', ['exact', 'gauss'])
def test_expand_is_the_mean_of_the_first_k2_rows(name):
    from prcv2025reid_amd import ops
    X, r64, gate = reference(name)
    _, _, _, _, k1, _ = fixture(name)
    N = X.shape[0]
    V32 = r64['V'].astype(np.float32)
    ld = (N + 3) // 4 * 4
    V = torch.zeros(N, ld, device='cuda'); V[:, :N] = dev(V32)
    V[:, N:] = 7.0                                              # padding columns are never read
    nbr = dev(r64['nbr'][:, :k1 + 1], torch.int32)
    for k2 in (1, 3, 6):
        out = sentinel_buffer(N, ld + 4, torch.float32)
        ops.rerank_expand(V, nbr, out, k1, k2)
        torch.cuda.synchronize()
        assert bool(is_sentinel(out[:, N:]).all())
        got = out[:, :N].cpu().numpy()
        if k2 == 1:
            assert np.array_equal(got.view(np.int32), V32[r64['nbr'][:, 0]].view(np.int32))     # bit for bit
            assert np.array_equal(r64['nbr'][:, 0], np.arange(N)) or name == 'exact'
        want = V32.astype(np.float64)[r64['nbr'][:, :k2]].mean(1)
        err = float(np.abs(got - want).max())
        print(f'  expand {name} k2={k2}: max |V2 - ref| = {err:.3e}, gate {gate:.3e}')
        assert err <= gate


def test_kernels_at_the_row_limit():
    # N = 65 536, the most the package accepts: the last rows' elements lie past 2^32 bytes and past 2^31 floats
    from prcv2025reid_amd import ops
    N = 65536
    rows = torch.arange(N, device='cuda')
    V = torch.zeros(N, N, device='cuda')
    V[rows, (rows * 7919 + 13) % N] = 0.75
    V[rows, (rows * 104729 + 5) % N] += 0.25
    nbr = torch.stack([rows, (rows + 1) % N], 1).to(torch.int32).contiguous()
    out = torch.empty(N, N, device='cuda')
    ops.rerank_expand(V, nbr, out, 20, 1)
    assert torch.equal(out, V)
    ops.rerank_expand(V, nbr, out, 20, 2)
    pick = torch.cat([rows[:32], rows[32767:32800], rows[-32:]])
    assert torch.equal(out[pick], (V[pick] + V[(pick + 1) % N]) / 2)
    assert float(out[N - 1].sum()) == 1.0 and float(out.sum(1).min()) == 1.0
    # weights and Jaccard at the same size, on lists whose answer is known: rows 2t and 2t + 1 are equal basis vectors that list
    # each other (k1 = 1, kh = 0), so R* = {2t, 2t + 1} and both weights are exactly 1/2
    del V
    X = torch.zeros(N, 64, device='cuda')
    X[rows, (rows // 2) % 64] = 1.0
    nbr = torch.stack([rows, rows ^ 1], 1).to(torch.int32).contiguous()
    out.fill_(float('nan'))
    ops.rerank_weights(nbr, X, out, 1)
    assert float(out.sum()) == N and bool((out[rows, rows] == 0.5).all()) and bool((out[rows, rows ^ 1] == 0.5).all())
    Nq, Ng = 15, N - 15                                         # query 14 and gallery row 0 (pooled row 15) are such a pair
    cos = torch.zeros(Nq, Ng + 3, device='cuda')
    s = torch.full((Nq, Ng + 3), 7.0, device='cuda')
    ops.rerank_jaccard(out[:Nq], out[Nq:], cos, s, Ng, N, 0.25)
    want = torch.zeros(Nq, Ng, device='cuda'); want[14, 0] = 0.75
    assert torch.equal(s[:, :Ng], want) and bool((s[:, Ng:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------- 3. jaccard
@pytest.mark.parametrize('Ng', [3, 219, 257])
@pytest.mark.parametrize('nq', [1, 5, 64, 70])
def test_jaccard_rows_against_fp64(nq, Ng):
    from prcv2025reid_amd import ops
    for N in (251, 320):
        rng = np.random.default_rng(1000 * nq + Ng + N)
        A, B = R.sparse_rows(rng, nq, N, 12), R.sparse_rows(rng, Ng, N, 12)
        B[Ng // 2] = A[0]                                       # one pair of equal rows: m = 1, J = 1
        cos = rng.uniform(-1, 1, (nq, Ng)).astype(np.float32)
        lda = (N + 3) // 4 * 4
        At = torch.full((nq, lda), 7.0, device='cuda'); At[:, :N] = dev(A)     # padding columns would change every sum if read
        Bt = torch.full((Ng, lda + 4), 7.0, device='cuda'); Bt[:, :N] = dev(B)
        ldo = (Ng + 3) // 4 * 4 + 8                             # ldo > Ng
        for lam in (0.0, 0.3, 1.0):
            want = R.jaccard_ref(A, B, cos, lam)
            gate = max(8 * float(np.abs(want - R.jaccard_ref(A, B, cos, lam, np.float32)).max()), 4 * EPS32)
            out = sentinel_buffer(nq, ldo, torch.float32)
            ops.rerank_jaccard(At, Bt, dev(cos), out, Ng, N, lam)
            torch.cuda.synchronize()
            assert bool(is_sentinel(out[:, Ng:]).all())         # columns >= Ng are not written
            got = out[:, :Ng].cpu().numpy().astype(np.float64)
            err = float(np.abs(got - want).max())
            assert err <= gate, (N, lam, err, gate)
            if lam == 1.0:
                assert np.array_equal(got, cos.astype(np.float64))
            if lam == 0.0:
                assert abs(got[0, Ng // 2] - 1.0) <= gate


# ------------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize('name', ['exact', 'gauss', 'gauss2'])
def test_rerank_scores_end_to_end(flavor, name):
    from prcv2025reid_amd.rerank import Reranker, RerankParams, rerank_scores
    X, r64, gate = reference(name)
    _, _, _, Nq, k1, k2 = fixture(name)
    assert_lists_are_settled(name, r64, k1)
    params = RerankParams(k1, k2, LAMBDA)
    Xd = dev(X)
    rr = Reranker(Xd[:Nq], Xd[Nq:], params)
    assert np.array_equal(rr.nbr.cpu().numpy(), r64['nbr'][:, :k1 + 1])
    N, Ng = X.shape[0], X.shape[0] - Nq
    err2 = float(np.abs(rr.V2[:, :N].cpu().numpy() - r64['V2']).max())
    assert np.array_equal(rr.V2[:, :N].cpu().numpy() != 0, r64['V2'] != 0) and err2 <= gate, err2
    got = np.zeros((Nq, Ng))
    starts = []
    for a, S in rerank_scores(Xd[:Nq], Xd[Nq:], params, normalized=True, chunk=20):
        assert S.shape[1] % 4 == 0 and S.shape[1] >= Ng and S.shape[0] <= 20
        got[a:a + S.shape[0]] = S[:, :Ng].cpu().numpy()
        starts.append(a)
    assert starts == list(range(0, Nq, 20))
    err = float(np.abs(got - r64['s']).max())
    print(f'  rerank_scores {name} {flavor}: max |s* - ref| = {err:.3e}, |V2 - ref| = {err2:.3e}, gate {gate:.3e}')
    assert err <= gate
    # the ranking of the returned rows is a valid ranking under the reference
    idx = torch.sort(torch.as_tensor(got, dtype=torch.float32), dim=1, descending=True, stable=True)[1].numpy()
    along = np.take_along_axis(r64['s'], idx, 1)
    assert (along[:, :-1] >= along[:, 1:] - 2 * gate).all()
    base = R.ranking(r64['cos'][:Nq, Nq:])[:, :10]
    assert (idx[:, :10] != base).any(1).mean() > 0.5            # re-ranking does change the top-10 of most queries


# ------------------------------------------------------------------------------------------------------------- 5. evaluator
def eval_case():
    X, qp, gp, Nq, k1, k2 = fixture('eval')
    _, r64, gate = reference('eval')
    Ng = X.shape[0] - Nq
    g_img = [f'g{j}' for j in range(Ng)]
    # every query carries two image ids: one of its positives (when it has one) and one other gallery row
    q_img = []
    for i in range(Nq):
        pos = np.flatnonzero(gp == qp[i])
        q_img.append([g_img[(7 * i + 3) % Ng]] + ([g_img[int(pos[i % len(pos)])]] if len(pos) else []))
    return X, qp, gp, Nq, k1, k2, r64, gate, g_img, q_img


def want_metrics(s, qp, gp, q_img, g_img, masked):
    rows = []
    for i in range(len(qp)):
        keep = np.array([not (masked and n in q_img[i]) for n in g_img])
        rows.append(R.ap_cmc(s[i], gp, qp[i], keep))
    valid = [r for r in rows if r[2] > 0]
    return {'mAP': float(np.mean([r[0] for r in valid])), 'num_queries': len(valid),
            **{f'R@{k}': float(np.mean([r[1] <= k for r in valid])) for k in (1, 5, 10)}}


def test_evaluator_metrics_with_rerank(flavor):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams
    X, qp, gp, Nq, k1, k2, r64, gate, g_img, q_img = eval_case()
    assert_lists_are_settled('eval', r64, k1)
    s = r64['s']
    for i in range(Nq):                                         # every positive-negative pair of a row is more than 4 gates apart
        pos, neg = s[i][gp == qp[i]], s[i][gp != qp[i]]
        assert pos.size == 0 or np.abs(pos[:, None] - neg[None, :]).min() > 4 * gate
    ev = ProtocolEvaluator(dev(X[Nq:]), torch.as_tensor(gp), g_img, normalized=True)
    Q, qpt = dev(X[:Nq]), torch.as_tensor(qp)
    results = {}
    for masked in (True, False):
        got = ev.rank_and_metrics(Q, qpt, q_img, ignore_same_img=masked, rerank=RerankParams(k1, k2, LAMBDA), chunk=8)
        want = want_metrics(s, qp, gp, q_img, g_img, masked)
        print(f'  evaluator {flavor} masked={masked}: {got}')
        assert got['num_queries'] == want['num_queries'] and abs(got['mAP'] - want['mAP']) < 1e-9, (got, want)
        # (the same hit counts: the evaluator's mean of 0/1 flags may round the quotient one ulp away from numpy's)
        assert all(abs(got[k] - want[k]) < 1e-12 for k in ('R@1', 'R@5', 'R@10')), (got, want)
        results[masked] = got
    assert results[True] != results[False]                      # the mask did remove positives
    # rerank=None is the existing path: the same dictionary, and not the re-ranked one
    plain = ev.rank_and_metrics(Q, qpt, q_img)
    assert plain == ev.rank_and_metrics(Q, qpt, q_img, rerank=None) and plain != results[True]
    S = ev.scores(Q)[:, :len(gp)].cpu().numpy().astype(np.float64)
    want = want_metrics(S, qp, gp, q_img, g_img, True)
    assert plain['num_queries'] == want['num_queries'] and all(abs(plain[k] - want[k]) < 1e-12 for k in ('mAP', 'R@1', 'R@5', 'R@10'))


# ------------------------------------------------------------------------------------------------------------- 6. CSV
def test_csv_export_with_and_without_rerank(tmp_path, flavor):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams
    from prcv2025reid_amd.retrieval import GalleryIndex
    X, qp, gp, Nq, k1, k2, r64, gate, g_img, _ = eval_case()
    top_k = 10
    assert R.min_gap_in_top(r64['s'], top_k + 1) > 4 * gate     # the first top_k of every reference row are settled
    ev = ProtocolEvaluator(dev(X[Nq:]), torch.as_tensor(gp), g_img, normalized=True)
    keys = [f'q{i}' for i in range(Nq)]
    ev.export_submission_csv(dev(X[:Nq]), keys, g_img, str(tmp_path / 'rr.csv'), top_k=top_k, rerank=RerankParams(k1, k2, LAMBDA), chunk=8)
    rows = (tmp_path / 'rr.csv').read_text().strip().split('\n')
    assert rows[0] == 'query_key,ranked_gallery_ids' and len(rows) == Nq + 1
    want = R.ranking(r64['s'])[:, :top_k]
    for i in range(Nq):
        assert rows[1 + i] == f'q{i},' + ' '.join(f'g{j}' for j in want[i]), i
    # without rerank: the file of the existing path, byte for byte
    ev.export_submission_csv(dev(X[:Nq]), keys, g_img, str(tmp_path / 'a.csv'), top_k=top_k)
    ev.export_submission_csv(dev(X[:Nq]), keys, g_img, str(tmp_path / 'b.csv'), top_k=top_k, rerank=None)
    idx, _ = GalleryIndex(dev(X[Nq:]), normalized=True).topk(dev(X[:Nq]), k=top_k)
    today = 'query_key,ranked_gallery_ids\r\n' + ''.join(f'q{i},' + ' '.join(f'g{j}' for j in row) + '\r\n'
                                                         for i, row in enumerate(idx.cpu().tolist()))
    assert (tmp_path / 'a.csv').read_bytes() == (tmp_path / 'b.csv').read_bytes() == today.encode()
    assert (tmp_path / 'a.csv').read_bytes() != (tmp_path / 'rr.csv').read_bytes()


# ------------------------------------------------------------------------------------------------------------- 7. errors
def test_argument_errors_launch_nothing():
    from prcv2025reid_amd import _lib, ops
    N, D = 256, 64
    X = torch.zeros(N, D, device='cuda')
    nbr = torch.zeros(N, 80, dtype=torch.int32, device='cuda')
    V = sentinel_buffer(N, N, torch.float32)
    V2 = sentinel_buffer(N, N, torch.float32)
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_weights: k1=65 outside 1\.\.64'):
        ops.rerank_weights(nbr, X, V, 65)
    with pytest.raises(_lib.ReidHipError, match=r'rc=-1: reid_rerank_expand: k1=8 k2=10'):
        ops.rerank_expand(V, nbr, V2, 8, 10)
    with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rerank_jaccard: null pointer'):
        _lib.check(_lib.lib().reid_rerank_jaccard(V.data_ptr(), N, V.data_ptr(), N, None, 224, V2.data_ptr(), N, 32, 224, N, 0.3, None))
    with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_rerank_weights: null pointer'):
        _lib.check(_lib.lib().reid_rerank_weights(None, 80, X.data_ptr(), D, V.data_ptr(), N, N, D, 8, None))
    torch.cuda.synchronize()
    assert bool(is_sentinel(V).all()) and bool(is_sentinel(V2).all())
