"""GPU: reid_rank_metrics_at (csrc/metrics.hip) per query against the numpy fp64 walk (tests/metrics_at_k_ref.py) of the evaluator's
OWN fp32 score rows -- the contract of test_evaluate_gpu.py::test_metrics_vs_oracle.

Exact: hits, rank1, rank_last, npos; ap / rank1 / npos equal to reid_rank_metrics' bits on the same rows; two runs give the same bits;
32 guard words around every output stay untouched and every element inside is written.  sum_at: within (hits + 1) * 2^-52 * sum_at,
twice the standard bound gamma_n of a sum of `hits` rounded quotients (metrics_at_k_ref.sum_bound: derived, not measured; below the
1e-12 of the existing test for K <= 1024).

Shapes, the smallest that reach each branch of the kernel: (16, 4100, 2) more than 256 positives per query, i.e. more than one per
thread in the last loop; (40, 3001, 7) Ng % 4 != 0, the scalar tail, ld = 3004; (8, 9000, 1) more than 8192 positives, npos = -1 and
zeros.  Every shape: duplicated gallery rows (exact score ties), exclusion lists of 0..4 image ids, query pids absent from the
gallery, cutoffs (1, 5, 100, Ng + 7)."""
import numpy as np
import pytest
import torch

import metrics_at_k_ref as M
from metrics_at_k_ref import check_guarded, guarded, make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(params=['bf16', 'f16'])
def flavor(request):
    from prcv2025reid_amd import _lib
    _lib.set_flavor(request.param)
    yield request.param
    _lib.set_flavor('bf16')


def reference(S, gp, qp, q_img, ks):
    ids = np.arange(S.shape[1])
    return [M.rows_ref(S[i], gp.numpy(), int(qp[i]), ks, ids, [int(x[2:]) for x in q_img[i]]) for i in range(S.shape[0])]


def compare(got, want, ks):
    """got: dict of numpy arrays (per_query_at's keys); want: list of rows_ref dictionaries."""
    for i, w in enumerate(want):
        assert (int(got['npos'][i]), int(got['rank1'][i]), int(got['rank_last'][i])) == (w['npos'], w['rank1'], w['rank_last']), (i, w)
        assert got['hits'][i].tolist() == w['hits'].tolist(), (i, got['hits'][i], w['hits'])
        err = np.abs(got['sum_at'][i] - w['sum_at'])
        assert np.all(err <= M.sum_bound(w['hits'], w['sum_at'])), (i, got['sum_at'][i], w['sum_at'], err)


@pytest.mark.parametrize('Nq,Ng,npid', [(16, 4100, 2), (40, 3001, 7), (8, 9000, 1)])
def test_rank_metrics_at_vs_numpy_walk(flavor, Nq, Ng, npid):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    ks = (1, 5, 100, Ng + 7)
    Q, G, qp, gp, q_img, g_img = make_case(Nq, Ng, npid)
    ev = ProtocolEvaluator(G.cuda(), gp, g_img)
    S = ev.scores(Q.cuda())
    assert S.stride(0) == (Ng + 3) // 4 * 4
    qp32, slot = ev._query_ids(qp)
    excl = ev._exclusions(q_img, True)
    assert bool((slot < 0).any()) and sorted({int(n) for n in (excl >= 0).sum(1)}) == [0, 1, 2, 3, 4]

    def run():
        bufs = {'ap': guarded((Nq,), torch.float64), 'rank1': guarded((Nq,), torch.int32), 'npos': guarded((Nq,), torch.int32),
                'rank_last': guarded((Nq,), torch.int32), 'hits': guarded((Nq, len(ks)), torch.int32),
                'sum_at': guarded((Nq, len(ks)), torch.float64)}
        ops.rank_metrics_at(S, ev.g_pid, ev.g_img, qp32, slot, excl, ev.csr_off, ev.csr_idx, Ng, ev.max_pos, ks,
                            *(bufs[n][1] for n in ('ap', 'rank1', 'npos', 'rank_last', 'hits', 'sum_at')))
        check_guarded(bufs)
        return {n: v[1].clone() for n, v in bufs.items()}
    first, second = run(), run()
    for n in first:                                                     # two runs: the same bits
        assert torch.equal(first[n].view(torch.int32), second[n].view(torch.int32)), n
    # ap, rank1, npos: reid_rank_metrics' bits on the same rows
    old = {'ap': guarded((Nq,), torch.float64), 'rank1': guarded((Nq,), torch.int32), 'npos': guarded((Nq,), torch.int32)}
    ops.rank_metrics(S, ev.g_pid, ev.g_img, qp32, slot, excl, ev.csr_off, ev.csr_idx, Ng, ev.max_pos, *(old[n][1] for n in ('ap', 'rank1', 'npos')))
    check_guarded(old)
    for n in old:
        assert torch.equal(old[n][1].view(torch.int32), first[n].view(torch.int32)), n
    # per_query_at is this call ...
    at = ev.per_query_at(Q.cuda(), qp, ks, q_img)
    for n in first:
        assert torch.equal(at[n].view(torch.int32), first[n].view(torch.int32)), n
    # ... per chunk of queries (chunk = 7: several launches, the last one short; the rows of a chunk are scored on their own, so only
    # what does not depend on the last bit of a score is compared with the unchunked call: per_query's bits on the same chunks, and
    # the cutoff beyond the gallery, which counts every positive)
    at7 = ev.per_query_at(Q.cuda(), qp, ks, q_img, chunk=7)
    for n, t in zip(('ap', 'rank1', 'npos'), ev.per_query(Q.cuda(), qp, q_img, chunk=7)):
        assert torch.equal(at7[n].view(torch.int32), t.view(torch.int32)), n
    assert torch.equal(at7['hits'][:, -1], at7['npos'].clamp(min=0)) and bool((at7['rank_last'] >= at7['rank1']).all())
    got = {n: v.cpu().numpy() for n, v in first.items()}
    Sn = S[:, :Ng].cpu().numpy()
    want = reference(Sn, gp, qp, q_img, ks)
    compare(got, want, ks)
    if npid == 1:                                                       # nothing is evaluated: more than 8192 positives, or none
        assert sorted(set(got['npos'].tolist())) == [-1, 0]
        for n in ('rank_last', 'hits', 'sum_at', 'ap', 'rank1'):
            assert not got[n].any(), n
        return
    assert (got['npos'] > 256).any() or Ng != 4100                      # more than one positive per thread in the last loop
    # a positive and a non-positive of EQUAL score on either side of a cutoff: only the tie rule decides hits there
    ties = 0
    gpn, qpn = gp.numpy(), qp.numpy()
    for i in range(Nq):
        excl_i = [int(x[2:]) for x in q_img[i]]
        order = np.argsort(-Sn[i].astype(np.float64), kind='stable')
        walk = order[~np.isin(order, excl_i)]
        for K in ks:
            if K < len(walk) and Sn[i, walk[K - 1]] == Sn[i, walk[K]]:
                ties += int((gpn[walk[K - 1]] == qpn[i]) != (gpn[walk[K]] == qpn[i]))
    assert ties >= 2, ties
    assert sum(Ng - len(np.unique(Sn[i])) for i in range(Nq)) > 4        # the duplicated rows did produce equal scores
    # the summary on the device tensors against the numpy arithmetic on the reference's per-query values
    from prcv2025reid_amd.evaluate import cutoff_summary
    for norm in ('hits', 'min'):
        s = cutoff_summary(first['sum_at'], first['hits'], first['rank1'], first['rank_last'], first['npos'], ks, norm)
        w = M.summary_ref(want, ks, norm)
        assert set(s) == set(w)
        for k in w:
            assert abs(s[k] - w[k]) <= 1e-12, (norm, k, s[k], w[k])
    # rank_and_metrics: ks=None is today's dictionary, a tuple adds the summary's keys to exactly that
    base = ev.rank_and_metrics(Q.cuda(), qp, q_img)
    full = ev.rank_and_metrics(Q.cuda(), qp, q_img, ks=ks)
    assert set(base) == {'mAP', 'R@1', 'R@5', 'R@10', 'num_queries'}
    assert {k: full[k] for k in base} == base
    assert {k: v for k, v in full.items() if k not in ('mAP', 'R@10', 'num_queries')} == \
        cutoff_summary(first['sum_at'], first['hits'], first['rank1'], first['rank_last'], first['npos'], ks, 'hits')
    assert full[f'mAP@{Ng + 7}'] == pytest.approx(full['mAP'], abs=1e-12)        # a cutoff beyond the gallery: the untruncated AP
    mAP, top1 = ev.reid_map(Q.cuda(), qp)
    mAP5, top1_5 = ev.reid_map(Q.cuda(), qp, k=5)
    t5 = ev.per_query_at(Q.cuda(), qp, (5,), None, False)
    assert top1_5 == top1 and mAP5 == cutoff_summary(t5['sum_at'], t5['hits'], t5['rank1'], None, t5['npos'], (5,))['mAP@5']


def test_per_query_at_on_reranked_and_expanded_rows(flavor):
    """With rerank= / expand=, per_query_at scores the rows per_query scores: the reference walks those rows."""
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.expansion import ExpansionParams
    from prcv2025reid_amd.rerank import RerankParams
    Nq, Ng, ks = 12, 301, (1, 5, 100)
    Q, G, qp, gp, q_img, g_img = make_case(Nq, Ng, 7)
    ev = ProtocolEvaluator(G.cuda(), gp, g_img)
    # re-ranked: s* rows of the pooled re-ranker
    rp = RerankParams(k1=8, k2=3, lambda_value=0.3)
    rows = ev._reranker(Q.cuda(), rp).rows(0, Nq)[:, :Ng].cpu().numpy()
    got = {n: v.cpu().numpy() for n, v in ev.per_query_at(Q.cuda(), qp, ks, q_img, rerank=rp).items()}
    compare(got, reference(rows, gp, qp, q_img, ks), ks)
    old = ev.per_query(Q.cuda(), qp, q_img, rerank=rp)
    for n, t in zip(('ap', 'rank1', 'npos'), old):
        assert np.array_equal(got[n].view(np.int32), t.cpu().numpy().view(np.int32)), n
    # expanded: cosine rows of the expanded queries
    xp = ExpansionParams(k=5, alpha=3)
    Qe = ev._expanded(Q.cuda(), xp, q_img, True, 1024, False)
    rows = ev.scores(Qe, normalized=True)[:, :Ng].cpu().numpy()
    got = {n: v.cpu().numpy() for n, v in ev.per_query_at(Q.cuda(), qp, ks, q_img, expand=xp).items()}
    compare(got, reference(rows, gp, qp, q_img, ks), ks)
    assert (got['npos'] > 0).any() and (got['hits'][:, 0] != got['hits'][:, 2]).any()


def test_rank_metrics_at_refuses_bad_arguments(flavor):
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    Q, G, qp, gp, q_img, g_img = make_case(8, 64, 3)
    ev = ProtocolEvaluator(G.cuda(), gp, g_img)
    for bad in ((5, 1), (0,), (), tuple(range(1, 10)), (3, 3)):
        with pytest.raises(ValueError, match='cutoffs'):
            ev.per_query_at(Q.cuda(), qp, bad)
    with pytest.raises(ValueError, match='norm'):
        ev.rank_and_metrics(Q.cuda(), qp, ks=(5,), norm='max')
