"""GPU: reid_list_metrics (csrc/list_metrics.hip) and the evaluator's list side -- score_lists, per_query_lists, score_submission_csv.

Lists of ranked_lists(k) for k in {1, 63, 64, 65, 100, 1024} (either side of the kernel's 64-position chunks, the longest list)
against galleries of 50 rows (k > Ng: trailing -1 entries) and 3001 rows: the integers equal those of per_query_at on the rows the
lists were cut from and those of the numpy list reference (tests/metrics_at_k_ref.py) exactly, the sums within
(hits + 1) * 2^-52 * sum_at (metrics_at_k_ref.sum_bound).  Hand-made lists, malformed lists, and the reference's own compute_map /
compute_cmc values (tests/golden/map_at_k.npz) through both paths, rows and lists."""
import os

import numpy as np
import pytest
import torch

import metrics_at_k_ref as M
from helpers import GOLDEN
from metrics_at_k_ref import check_guarded, guarded, make_case

pytestmark = pytest.mark.gpu
NQ = 16


@pytest.fixture(params=['bf16', 'f16'])
def flavor(request):
    from prcv2025reid_amd import _lib
    _lib.set_flavor(request.param)
    yield request.param
    _lib.set_flavor('bf16')


_cases = {}


def evaluator(flavor, Ng):
    """(evaluator, case) per (flavor, Ng), built once."""
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    if (flavor, Ng) not in _cases:
        case = make_case(NQ, Ng, 7)
        _cases[flavor, Ng] = ProtocolEvaluator(case[1].cuda(), case[3], case[5]), case
    return _cases[flavor, Ng]


def list_reference(idx, gp, qp, q_img, ks):
    ids = np.arange(len(gp))
    return [M.list_ref(idx[i], gp.numpy(), int(qp[i]), ks, ids, [int(x[2:]) for x in q_img[i]]) for i in range(idx.shape[0])]


def compare_lists(got, want):
    for i, w in enumerate(want):
        assert (int(got['npos'][i]), int(got['rank1'][i])) == (w['npos'], w['rank1']), (i, got['npos'][i], got['rank1'][i], w)
        assert got['hits'][i].tolist() == w['hits'].tolist(), (i, got['hits'][i], w['hits'])
        err = np.abs(got['sum_at'][i] - w['sum_at'])
        assert np.all(err <= M.sum_bound(w['hits'], w['sum_at'])), (i, got['sum_at'][i], w['sum_at'], err)


@pytest.mark.parametrize('Ng', [50, 3001])
@pytest.mark.parametrize('k', [1, 63, 64, 65, 100, 1024])
def test_lists_of_ranked_lists_vs_rows_and_numpy(flavor, k, Ng):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.evaluate import cutoff_summary
    ev, (Q, G, qp, gp, q_img, g_img) = evaluator(flavor, Ng)
    ks = tuple(sorted({K for K in (1, 5, 63, 64, 65, 100, k) if K <= k}))
    idx, _ = ev.ranked_lists(Q.cuda(), k=k, q_img_ids=q_img)
    assert bool((idx[:, -1] == -1).all()) == (k > Ng)                     # lists longer than the gallery trail with -1
    # the kernel itself, between guard words, twice
    qp32, slot = ev._query_ids(qp)
    excl = ev._exclusions(q_img, True)

    def run():
        bufs = {'npos': guarded((NQ,), torch.int32), 'rank1': guarded((NQ,), torch.int32), 'hits': guarded((NQ, len(ks)), torch.int32),
                'sum_at': guarded((NQ, len(ks)), torch.float64), 'status': guarded((NQ,), torch.int32)}
        ops.list_metrics(idx, ev.g_pid, ev.g_img, qp32, slot, excl, ev.csr_off, ev.csr_idx, Ng, ks,
                         out=tuple(bufs[n][1] for n in ('npos', 'rank1', 'hits', 'sum_at', 'status')))
        check_guarded(bufs)
        return {n: v[1].clone() for n, v in bufs.items()}
    first, second = run(), run()
    for n in first:
        assert torch.equal(first[n].view(torch.int32), second[n].view(torch.int32)), n
    assert not bool(first['status'].any())
    lists = ev.per_query_lists(idx, qp, ks, q_img)
    for n in lists:
        assert torch.equal(lists[n].view(torch.int32), first[n].view(torch.int32)), n
    got = {n: v.cpu().numpy() for n, v in lists.items()}
    # against the numpy walk of the same lists
    want = list_reference(idx.cpu().numpy(), gp, qp, q_img, ks)
    compare_lists(got, want)
    assert any(w['hits'][-1] > 0 for w in want) and any(w['npos'] == 0 for w in want)
    # against the row kernel on the rows the lists were cut from
    rows = {n: v.cpu().numpy() for n, v in ev.per_query_at(Q.cuda(), qp, ks, q_img).items()}
    assert np.array_equal(got['hits'], rows['hits']) and np.array_equal(got['npos'], rows['npos'])
    assert np.array_equal(got['rank1'], np.where(rows['rank1'] <= k, rows['rank1'], 0))
    assert np.all(np.abs(got['sum_at'] - rows['sum_at']) <= M.sum_bound(rows['hits'], rows['sum_at']))
    for norm in ('hits', 'min'):
        a = ev.score_lists(idx, qp, ks, q_img, norm=norm)
        b = cutoff_summary(*(torch.from_numpy(rows[n]) for n in ('sum_at', 'hits', 'rank1')), None, torch.from_numpy(rows['npos']), ks, norm)
        assert set(a) == set(b) and 'mINP' not in a
        for key in a:
            assert abs(a[key] - b[key]) <= 1e-12, (norm, key, a[key], b[key])


def test_hand_made_lists(flavor):
    """Hits on both sides of position 64, a list without a hit, a query pid absent from the gallery, and a foreign list that holds a
    gallery row its query excludes: the row is skipped and what follows moves up."""
    ev, (Q, G, qp, gp, q_img, g_img) = evaluator(flavor, 3001)
    k, ks = 100, (1, 5, 64, 65, 100)
    idx = torch.full((NQ, k), -1, dtype=torch.int32)
    gpn = gp.numpy()
    for i in range(NQ):                                                  # no hit, nothing excluded: every query but 0 and 3 keeps this list
        ex = [int(x[2:]) for x in q_img[i]]
        neg = [j for j in np.nonzero(gpn != int(qp[i]))[0].tolist() if j not in ex][:k]
        idx[i] = torch.tensor(neg, dtype=torch.int32)
    pos = np.nonzero(gpn == 0)[0]
    assert int(qp[0]) == int(qp[3]) == 0 and not q_img[0] and len(q_img[3]) == 4
    for t, j in zip((2, 63, 64, 69), pos[:4]):                           # query 0: hits at positions 3, 64, 65, 70
        idx[0, t] = int(j)
    # query 3 excludes four gallery images: its list holds two of them in front of the same four hits, which move up by two
    excluded = sorted({int(x[2:]) for x in q_img[3]})
    assert len(excluded) >= 2
    keep = [int(j) for j in pos if int(j) not in excluded][:4]
    idx[3, 0], idx[3, 1] = excluded[0], excluded[-1]
    for t, j in zip((4, 65, 66, 71), keep):
        idx[3, t] = j
    got = {n: v.cpu().numpy() for n, v in ev.per_query_lists(idx, qp, ks, q_img).items()}
    compare_lists(got, list_reference(idx.numpy(), gp, qp, q_img, ks))
    for q in (0, 3):
        assert got['rank1'][q] == 3 and got['hits'][q].tolist() == [0, 1, 2, 3, 4]
        assert abs(got['sum_at'][q, 4] - (1 / 3 + 2 / 64 + 3 / 65 + 4 / 70)) <= 5 * 2.0 ** -52
    assert got['npos'][0] == len(pos) and got['npos'][3] == len(set(pos.tolist()) - set(excluded)) < len(pos)   # (make_case: query 3 excludes a positive)
    assert got['npos'][1] == got['npos'][7] == 0 and not got['hits'][[1, 2, 7]].any() and not got['rank1'][[1, 2, 7]].any()
    r = ev.score_lists(idx, qp, ks, q_img)
    assert r['num_queries@1'] == 0 and r['mAP@1'] == 0.0 and r['num_queries@100'] == 2
    assert abs(r['mAP@100'] - (1 / 3 + 2 / 64 + 3 / 65 + 4 / 70) / 4) <= 1e-15


def test_malformed_lists(flavor):
    from prcv2025reid_amd import ops
    ev, (Q, G, qp, gp, q_img, g_img) = evaluator(flavor, 50)
    k, ks = 70, (1, 5, 64, 65)
    good, _ = ev.ranked_lists(Q.cuda(), k=k, q_img_ids=q_img)
    clean = ev.per_query_lists(good, qp, ks, q_img)
    qp32, slot = ev._query_ids(qp)
    excl = ev._exclusions(q_img, True)
    bad = good.clone()
    bad[2, 66] = -2                                                       # a negative index other than -1 (second chunk)
    bad[5, 3] = 50                                                        # an index >= Ng
    bad[6, 10] = -1                                                       # an entry behind a -1 ...
    bad[9, 69] = 7                                                        # ... also when the -1 sits in an earlier chunk
    npos, rank1, hits, sum_at, status = ops.list_metrics(bad, ev.g_pid, ev.g_img, qp32, slot, excl, ev.csr_off, ev.csr_idx, 50, ks)
    want = torch.zeros(NQ, dtype=torch.int32)
    want[2], want[5], want[6], want[9] = ops.LIST_BAD_NEGATIVE, ops.LIST_BAD_RANGE, ops.LIST_BAD_ORDER, ops.LIST_BAD_ORDER
    assert torch.equal(status.cpu(), want)
    flagged = want != 0
    for t, c in ((npos, clean['npos']), (rank1, clean['rank1']), (hits, clean['hits']), (sum_at, clean['sum_at'])):
        assert not bool(t.cpu()[flagged].any())                           # a flagged query: every output zero
        assert torch.equal(t.cpu()[~flagged], c.cpu()[~flagged])          # the others: untouched by their neighbours' lists
    for q, t, v in ((2, 66, -2), (5, 3, 50), (6, 10, -1)):
        one = good.clone(); one[q, t] = v
        with pytest.raises(ValueError, match=rf'query {q} holds an index outside -1 \.\. 49 or an entry behind a -1'):
            ev.score_lists(one, qp, ks, q_img)
    twice = good.clone(); twice[4, 30] = twice[4, 2]
    with pytest.raises(ValueError, match='a gallery row occurs twice in the list of query 4'):
        ev.score_lists(twice, qp, ks, q_img)
    assert set(ev.score_lists(twice, qp, ks, q_img, check_duplicates=False)) == set(ev.score_lists(good, qp, ks, q_img))
    # a cutoff above k: refused before any launch (the outputs are never allocated: the status of a launch could not be read here)
    for call in (lambda: ev.score_lists(good, qp, (5, 71), q_img),
                 lambda: ops.list_metrics(good, ev.g_pid, ev.g_img, qp32, slot, excl, ev.csr_off, ev.csr_idx, 50, (5, 71))):
        with pytest.raises(ValueError, match='cutoffs: 71 is beyond the list length 70'):
            call()
    with pytest.raises(ValueError, match='cutoffs'):
        ev.score_lists(good, qp, (5, 5), q_img)
    with pytest.raises(ValueError, match='16 lists for 3 query pids'):
        ev.score_lists(good, qp[:3], ks)


def test_reference_fixture_through_rows_and_lists(flavor):
    """compute_map(k) / compute_cmc(k) of the reference (train.py:101-138) on tests/golden/map_at_k.npz: 'hits' form, no exclusion."""
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    z = np.load(os.path.join(GOLDEN, 'map_at_k.npz'))
    Q, G = torch.tensor(z['Q']).cuda(), torch.tensor(z['G']).cuda()
    qp, gp = torch.tensor(z['q_pid']), torch.tensor(z['g_pid'])
    Nq, Ng = Q.shape[0], G.shape[0]
    ev = ProtocolEvaluator(G, gp)
    map_ks, cmc_ks = tuple(int(k) for k in z['map_ks']), tuple(int(k) for k in z['cmc_ks'])
    rows = ev.rank_and_metrics(Q, qp, ignore_same_img=False, ks=map_ks)
    idx, _ = ev.ranked_lists(Q, k=100)
    assert Ng < 100 and bool((idx[:, Ng:] == -1).all()) and bool((idx[:, :Ng] >= 0).all())
    lists = ev.score_lists(idx, qp, map_ks)
    for k, want in zip(map_ks, z['map_at']):
        assert abs(rows[f'mAP@{k}'] - float(want)) < 1e-6, (k, rows[f'mAP@{k}'], want)
        assert abs(lists[f'mAP@{k}'] - float(want)) < 1e-6, (k, lists[f'mAP@{k}'], want)
    assert ev.reid_map(Q, qp, k=100)[0] == rows['mAP@100']
    r_rows = ev.per_query_at(Q, qp, cmc_ks)['rank1'].cpu().numpy()
    r_lists = ev.per_query_lists(idx, qp, cmc_ks)['rank1'].cpu().numpy()
    for k, want in zip(cmc_ks, z['cmc_at']):                              # compute_cmc divides by ALL queries: compare counts
        n = int(round(float(want) * Nq))
        assert int(((r_rows >= 1) & (r_rows <= k)).sum()) == n and int(((r_lists >= 1) & (r_lists <= k)).sum()) == n, k


@pytest.mark.parametrize('Ng', [50, 500])
def test_submission_csv_scores_like_its_lists(tmp_path, flavor, Ng):
    """export_submission_csv -> score_submission_csv reproduces score_lists of the export's own unmasked lists (Ng = 50: lists of 50
    names under a cutoff of 100)."""
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    Q, G, qp, gp, q_img, g_img = make_case(NQ, Ng, 7)
    names = [f'{x}.jpg' for x in g_img]
    ev = ProtocolEvaluator(G.cuda(), gp, g_img)
    keys = [f'q{i:02d}' for i in range(NQ)]
    path = str(tmp_path / 'sub.csv')
    ev.export_submission_csv(Q.cuda(), keys, names, path, top_k=100)
    ks = (1, 10, 100)
    idx, _ = ev.index.topk(Q.cuda(), k=min(100, Ng))                       # the lists the export wrote
    idx = torch.cat([idx, torch.full((NQ, 100 - idx.shape[1]), -1, dtype=torch.int32, device=idx.device)], 1)
    for norm in ('hits', 'min'):
        got = ev.score_submission_csv(path, {key: int(p) for key, p in zip(keys, qp)}, names, ks, norm)
        assert got == ev.score_lists(idx, qp, ks, None, False, norm)
    assert got['num_queries@100'] > 0 and 0.0 < got['mAP@100'] <= 1.0
    with open(path, 'a') as f:
        f.write('q99,im1.jpg\n')
    with pytest.raises(ValueError, match=r"sub\.csv:18: unknown query key 'q99'"):
        ev.score_submission_csv(path, {key: int(p) for key, p in zip(keys, qp)}, names, ks)
