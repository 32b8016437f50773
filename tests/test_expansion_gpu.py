"""reid_expand_rows (csrc/expand.hip) and the layers on top of it, on the GPU.  The raw sum is compared bit for bit with the float32
loop of expansion_ref.py (itself checked against float64 and against hand cases in test_expansion_cpu.py); the normalised output with
rowops_refs.l2norm_ref's allowance on the kernel's own raw sum; every layer above with the same call made by hand, bit for bit.

Shapes are the smallest at which the kernel's paths differ: D = 4 (one lane), 252 / 256 / 260 (around one float4 per lane), 512 and
1024 (the two- and four-vector instantiations); rows 1..5 around the four rows of a workgroup and 257 (more than one workgroup, a
partial last one); lists of 1, 2, 10, 11 and 64 entries (below, at and above the four-entry unroll; every lane of the wave)."""
import numpy as np
import pytest
import torch

import expansion_ref as E
from helpers import is_sentinel, sentinel_buffer
from rowops_refs import assert_within, f32, l2norm_ref

pytestmark = pytest.mark.gpu

DS = (4, 252, 256, 260, 512, 1024)
ROWS = (1, 3, 4, 5, 257)
MS = (1, 5, 1000)
K_KL = ((1, 1), (1, 2), (10, 10), (10, 11), (64, 64))
ALPHAS = (0, 1, 3)
SELF_BASES = (-1, 0, 7)
EPS = 1e-12


@pytest.fixture(params=['bf16', 'f16'])
def flavor(request):
    from prcv2025reid_amd import _lib
    _lib.set_flavor(request.param)
    yield request.param
    _lib.set_flavor('bf16')


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def unit_rows(rng, n, D):
    v = rng.standard_normal((n, D))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def in_wider(a, extra, fill):
    """``a`` [r, c] as the [:r, :c] view of a device buffer with ``extra`` more columns holding ``fill`` (a leading dimension > c)."""
    r, c = a.shape
    buf = torch.full((r, c + extra), fill, dtype=torch.as_tensor(a[:0]).dtype, device='cuda')
    buf[:, :c] = dev(a)
    return buf[:, :c]


def sweep(D, k, kl):
    """Yields (x, table, nbr, score as numpy; their device views with padded leading dimensions; alpha, self_base) over the rows, table
    sizes, weights and self bases of the grid, for one D and one (k, kl).  Row 0 of x is all zero from three rows on."""
    rng = np.random.default_rng(100000 + 100 * D + 7 * k + kl)
    table = unit_rows(rng, max(MS), D)
    table_d = in_wider(table, 4, float('nan'))
    for M in MS:
        for rows in ROWS:
            x = unit_rows(rng, rows, D)
            if rows >= 3:
                x[0] = 0.0
            x_d = in_wider(x, 8, float('nan'))
            for self_base in SELF_BASES:
                nbr, score = E.random_lists(rng, rows, kl, M, self_base)
                nbr_d, score_d = in_wider(nbr, 3, 0), in_wider(score, 3, 1.0)      # entries past kl are valid ones: never to be used
                for alpha in ALPHAS:
                    yield (x, table[:M], nbr, score), (x_d, table_d[:M], nbr_d, score_d), alpha, self_base


def launch(dv, k, alpha, self_base, normalize):
    """The kernel's output [rows, D] inside a sentinel buffer with 12 padding columns and 2 rows past the end; checks that only
    out[:rows, :D] was written."""
    from prcv2025reid_amd import ops
    x_d = dv[0]
    rows, D = x_d.shape
    buf = sentinel_buffer(rows + 2, D + 12, torch.float32)
    out = ops.expand_rows(*dv, k, alpha, self_base=self_base, normalize=normalize, eps=EPS, out=buf[:rows, :D])
    assert out.data_ptr() == buf.data_ptr()
    assert bool(is_sentinel(buf[:, D:]).all()) and bool(is_sentinel(buf[rows:]).all())
    assert not bool(is_sentinel(out).any())
    return out


# ---- 4. the raw sum, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,kl', K_KL)
@pytest.mark.parametrize('D', DS)
def test_raw_output_is_bit_equal_to_the_float32_loop(D, k, kl):
    cases = added = 0
    for host, dv, alpha, self_base in sweep(D, k, kl):
        assert dv[0].stride(0) > D and dv[1].stride(0) > D and dv[2].stride(0) > kl
        want = E.expand_rows_ref(*host, k, alpha, self_base)
        got = launch(dv, k, alpha, self_base, normalize=False).cpu().numpy()
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), (dict(D=D, k=k, kl=kl, alpha=alpha, self_base=self_base, rows=host[0].shape[0], M=host[1].shape[0]),
                            np.argwhere(~same)[:5].tolist())
        cases += 1
        added += int((want != host[0]).any())
    assert cases == len(MS) * len(ROWS) * len(SELF_BASES) * len(ALPHAS) and added > cases // 2       # (most cases do add rows)


# ---- 5. the normalised output --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,kl', K_KL)
@pytest.mark.parametrize('D', DS)
def test_normalised_output_is_within_l2norms_allowance_of_the_raw_sum(D, k, kl):
    worst = 0.0
    for _, dv, alpha, self_base in sweep(D, k, kl):
        raw = launch(dv, k, alpha, self_base, normalize=False)
        got = launch(dv, k, alpha, self_base, normalize=True)
        ref, allow = l2norm_ref(raw.double(), f32(EPS), 1.0)
        worst = max(worst, assert_within(got, ref, allow, dict(D=D, k=k, kl=kl, alpha=alpha, self_base=self_base, rows=raw.shape[0])))
    print(f'D={D} k={k} kl={kl}: worst |d| / allowance = {worst:.3f}')


def test_zero_row_without_neighbours_normalises_to_zeros():
    from prcv2025reid_amd import ops
    x = torch.zeros(5, 64, device='cuda')
    x[3] = 1.0
    table = dev(unit_rows(np.random.default_rng(1), 9, 64))
    nbr = torch.full((5, 4), -1, dtype=torch.int32, device='cuda')
    score = torch.ones(5, 4, device='cuda')
    out = ops.expand_rows(x, table, nbr, score, 3, 1)
    assert bool((bits(out[[0, 1, 2, 4]]) == 0).all())                         # +0, not NaN
    assert torch.equal(out[3], torch.full((64,), 0.125, device='cuda'))       # 1 / sqrt(64)
    assert torch.equal(ops.expand_rows(x, table, nbr, score, 3, 1, normalize=False), x)


# ---- 6. expand_queries -----------------------------------------------------------------------------------------------------------------------
def clustered(seed, Nq, Ng, D, per_id=6):
    """(Q [Nq, D], q_pid, G [Ng, D], g_pid) float32 numpy: gallery rows around one centre per identity, queries around the same centres
    with a common shift (the other modality)."""
    rng = np.random.default_rng(seed)
    g_pid = np.arange(Ng) // per_id
    centres = rng.standard_normal((g_pid.max() + 1, D))
    G = centres[g_pid] + 0.7 * rng.standard_normal((Ng, D))
    q_pid = rng.integers(0, g_pid.max() + 1, Nq)
    Q = centres[q_pid] + 0.7 * rng.standard_normal((Nq, D)) + 0.5 * rng.standard_normal(D)
    return Q.astype(np.float32), q_pid, G.astype(np.float32), g_pid


def expansion_f64(x, table, nbr, score, alpha):
    """Normalised float64 x + sum max(s, 0)^alpha table[nbr] over the valid entries of given lists (all of them are used)."""
    x, table, nbr, score = (t.cpu().numpy() for t in (x, table, nbr, score))
    w = np.where(nbr >= 0, np.maximum(score.astype(np.float64), 0.0) ** alpha, 0.0)
    raw = x.astype(np.float64) + np.einsum('rt,rtd->rd', w, table.astype(np.float64)[np.clip(nbr, 0, None)])
    return raw / np.linalg.norm(raw, axis=1, keepdims=True)


@pytest.mark.parametrize('alpha', [0, 3])
def test_expand_queries_is_expand_rows_on_the_index_lists(alpha):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.expansion import ExpansionParams, expand_queries
    from prcv2025reid_amd.retrieval import GalleryIndex, l2_normalize
    Q, _, G, _ = clustered(5, 33, 500, 64)
    g_img = torch.arange(500, dtype=torch.int32) // 2
    q_img = torch.arange(33, dtype=torch.int32) * 3
    index = GalleryIndex(dev(G), img_ids=g_img)
    p = ExpansionParams(10, alpha)
    Qn = l2_normalize(dev(Q))
    for ids in (None, q_img):
        nbr, score = index.topk(Qn, k=10, normalized=True, query_img_ids=ids)
        want = ops.expand_rows(Qn, index.Gf, nbr, score, 10, alpha)
        got = expand_queries(dev(Q), index, p, query_img_ids=ids)
        assert torch.equal(bits(got), bits(want))
        assert torch.equal(bits(expand_queries(Qn, index, p, normalized=True, query_img_ids=ids)), bits(want))
        assert np.abs(got.cpu().numpy() - expansion_f64(Qn, index.Gf, nbr, score, alpha)).max() < 1e-6
        assert float((got - Qn).abs().max()) > 0.01                              # the queries do move
    excluded = g_img.cuda()[nbr.long()] == q_img.cuda()[:, None]
    assert not bool(excluded.any())


# ---- 7. augment_gallery ----------------------------------------------------------------------------------------------------------------------
def test_augment_gallery_does_not_depend_on_the_chunk():
    from prcv2025reid_amd.expansion import ExpansionParams, augment_gallery
    from prcv2025reid_amd.retrieval import GalleryIndex, l2_normalize
    _, _, G, _ = clustered(6, 1, 300, 64)
    G[5] = G[2]                                                   # an exact duplicate: row 5's list starts with row 2, then itself
    p = ExpansionParams(10, 3)
    Gd = dev(G)
    whole = augment_gallery(Gd, p, chunk=300)
    assert whole.shape == (300, 64) and whole.data_ptr() != Gd.data_ptr()
    for chunk in (7, 64):
        assert torch.equal(bits(augment_gallery(Gd, p, chunk=chunk)), bits(whole)), chunk
    Gn = l2_normalize(Gd)
    assert torch.equal(bits(augment_gallery(Gn, p, normalized=True)), bits(whole))
    nbr, score = GalleryIndex(Gn, normalized=True).topk(Gn, k=11, normalized=True)
    assert nbr[5, :2].tolist() == [2, 5] and nbr[2, :2].tolist() == [2, 5]
    assert torch.equal(bits(whole[5]), bits(whole[2]))            # each uses the other: dropped by index, not by position
    own = nbr == torch.arange(300, device='cuda', dtype=torch.int32)[:, None]
    assert bool((own.sum(1) == 1).all())
    others = torch.argsort((~own).long(), dim=1, descending=True, stable=True)[:, :10]          # the ten other entries, in list order
    want = expansion_f64(Gn, Gn, torch.gather(nbr, 1, others), torch.gather(score, 1, others), 3)
    assert np.abs(whole.cpu().numpy() - want).max() < 1e-6
    assert float((whole - Gn).abs().max()) > 0.01


def test_augment_gallery_of_three_rows_with_k_ten():
    from prcv2025reid_amd.expansion import ExpansionParams, augment_gallery
    from prcv2025reid_amd.retrieval import l2_normalize
    rng = np.random.default_rng(8)
    G = (rng.standard_normal((3, 64)) + 2.0).astype(np.float32)            # positive cosines
    out = augment_gallery(dev(G), ExpansionParams(10, 1))
    Gn = l2_normalize(dev(G)).cpu().numpy().astype(np.float64)
    want = np.stack([Gn[i] + sum((Gn[i] @ Gn[j]) * Gn[j] for j in range(3) if j != i) for i in range(3)])
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert out.shape == (3, 64) and np.abs(out.cpu().numpy() - want).max() < 1e-6


# ---- 8. - 10. the evaluator ---------------------------------------------------------------------------------------------------------------------
def evaluator_case(D):
    Nq, Ng = 40, 600
    Q, q_pid, G, g_pid = clustered(40 + D, Nq, Ng, D)
    names = [f'g{j}' for j in range(Ng)]
    cos = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float64) @ (G / np.linalg.norm(G, axis=1, keepdims=True)).astype(np.float64).T
    order = np.argsort(-cos, 1)
    q_img = []
    for i in range(Nq):                                           # queries 0..19: one to four excluded images, the top gallery row first
        n = (i % 4) + 1 if i < 20 else 0
        q_img.append([names[j] for j in order[i, [0, 3, 17, 150][:n]]])
    return dev(Q), torch.as_tensor(q_pid), dev(G), torch.as_tensor(g_pid), names, q_img, order


def by_hand(ev, Q, p, **lists_kw):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.retrieval import l2_normalize
    nbr, score = ev.ranked_lists(Q, k=p.k, **lists_kw)
    return ops.expand_rows(l2_normalize(Q), ev.Gf, nbr, score, p.k, p.alpha), nbr, score


def same_tuple(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize('D', [64, 512])
def test_evaluator_expand_is_the_call_on_features_expanded_by_hand(tmp_path, flavor, D):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.expansion import ExpansionParams
    from prcv2025reid_amd.rerank import RerankParams
    Q, qp, G, gp, names, q_img, _ = evaluator_case(D)
    ev = ProtocolEvaluator(G, gp, names)
    p = ExpansionParams(10, 3)
    Qe, nbr, _ = by_hand(ev, Q, p, q_img_ids=q_img, chunk=16)
    assert float((Qe - torch.nn.functional.normalize(Q, dim=1)).abs().max()) > 0.01
    keys = [f'q{i}' for i in range(Q.shape[0])]
    for rerank in (None, RerankParams(8, 3, 0.3), RerankParams(8, 3, 0.3, sparse=True)):
        kw = dict(q_img_ids=q_img, chunk=16, rerank=rerank)
        assert same_tuple(ev.per_query(Q, qp, expand=p, **kw), ev.per_query(Qe, qp, normalized=True, **kw)), rerank
        assert same_tuple(ev.ranked_lists(Q, k=20, expand=p, **kw), ev.ranked_lists(Qe, k=20, normalized=True, **kw)), rerank
        ap, rank1, npos = ev.per_query(Qe, qp, normalized=True, **kw)
        m = ev.rank_and_metrics(Q, qp, q_img, chunk=16, rerank=rerank, expand=p)
        assert m['num_queries'] == int((npos > 0).sum()) > 0 and m['mAP'] == float(ap[npos > 0].mean())
        assert m['R@1'] == float((rank1[npos > 0] <= 1).double().mean())
        # the export ranks without exclusion, and so does its expansion
        Qu, _, _ = by_hand(ev, Q, p, chunk=16)
        ev.export_submission_csv(Q, keys, names, str(tmp_path / 'a.csv'), top_k=15, rerank=rerank, chunk=16, expand=p)
        ev.export_submission_csv(Qu, keys, names, str(tmp_path / 'b.csv'), top_k=15, rerank=rerank, chunk=16)
        text = (tmp_path / 'a.csv').read_text()
        assert text == (tmp_path / 'b.csv').read_text() and len(text.strip().split('\n')) == Q.shape[0] + 1
    # expansion changes the evaluation: it is not the plain call
    assert not same_tuple(ev.ranked_lists(Q, k=20, q_img_ids=q_img, expand=p)[1:], ev.ranked_lists(Q, k=20, q_img_ids=q_img)[1:])


@pytest.mark.parametrize('D', [64, 512])
def test_evaluator_augment_is_the_evaluator_of_the_augmented_gallery(flavor, D):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.expansion import ExpansionParams, augment_gallery
    Q, qp, G, gp, names, q_img, _ = evaluator_case(D)
    p = ExpansionParams(10, 3)
    a = ProtocolEvaluator(G, gp, names, augment=p)
    b = ProtocolEvaluator(augment_gallery(G, p), gp, names, normalized=True)
    assert torch.equal(bits(a.Gf), bits(b.Gf)) and torch.equal(a._Gcat.view(torch.int16), b._Gcat.view(torch.int16))
    for expand in (None, p):
        kw = dict(q_img_ids=q_img, chunk=16, expand=expand)
        assert same_tuple(a.per_query(Q, qp, **kw), b.per_query(Q, qp, **kw))
        assert same_tuple(a.ranked_lists(Q, k=20, **kw), b.ranked_lists(Q, k=20, **kw))
    assert not torch.equal(bits(a.Gf), bits(ProtocolEvaluator(G, gp, names).Gf))


def test_excluded_image_is_never_averaged_into_its_query():
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.expansion import ExpansionParams
    from prcv2025reid_amd.retrieval import l2_normalize
    Q, qp, G, gp, names, q_img, order = evaluator_case(64)
    ev = ProtocolEvaluator(G, gp, names)
    p = ExpansionParams(10, 3)
    got = ev._expanded(Q, p, q_img, True, 16, False)
    plain_idx, plain_score = (t.cpu().numpy() for t in ev.ranked_lists(Q, k=p.k + 4))          # no exclusion: up to four rows to drop
    Qn = l2_normalize(Q)
    for i in (0, 1, 3, 30):                                       # one, two and four excluded images; none
        drop = {int(n[1:]) for n in q_img[i]}
        assert (int(plain_idx[i, 0]) in drop) == (i < 20) and (i >= 20 or int(order[i, 0]) == int(plain_idx[i, 0]))
        keep = [t for t in range(p.k + 4) if int(plain_idx[i, t]) not in drop][:p.k]
        nbr, score = plain_idx[i:i + 1, keep], plain_score[i:i + 1, keep]
        raw = E.expand_rows_ref(Qn[i:i + 1].cpu().numpy(), ev.Gf.cpu().numpy(), nbr, score, p.k, p.alpha)
        ref, allow = l2norm_ref(torch.as_tensor(raw).double(), f32(EPS), 1.0)
        assert_within(got[i:i + 1].cpu(), ref, allow, f'query {i}')
        assert torch.equal(bits(got[i:i + 1]), bits(ops.expand_rows(Qn[i:i + 1], ev.Gf, dev(nbr), dev(score), p.k, p.alpha)))
    # with the exclusion switched off the top row is averaged in: another feature
    assert not torch.equal(bits(ev._expanded(Q, p, q_img, False, 16, False)[:20]), bits(got[:20]))


def test_defaults_leave_the_plain_calls_bit_for_bit():
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    Q, qp, G, gp, names, q_img, _ = evaluator_case(64)
    ev = ProtocolEvaluator(G, gp, names)
    ev_none = ProtocolEvaluator(G, gp, names, augment=None)
    assert torch.equal(bits(ev.Gf), bits(ev_none.Gf))
    assert same_tuple(ev.per_query(Q, qp, q_img, chunk=16), ev_none.per_query(Q, qp, q_img, chunk=16, expand=None))
    assert same_tuple(ev.ranked_lists(Q, k=20, q_img_ids=q_img), ev_none.ranked_lists(Q, k=20, q_img_ids=q_img, expand=None))
    assert ev.rank_and_metrics(Q, qp, q_img) == ev_none.rank_and_metrics(Q, qp, q_img, expand=None)
