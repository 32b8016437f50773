"""CPU: the cutoff metrics' host side -- the numpy references against the reference's own compute_map / compute_cmc values
(tests/golden/map_at_k.npz), evaluate.cutoff_summary on hand-computed cases, the submission CSV parser and the two new entry points'
declarations.  No kernel runs here (tests/test_metrics_at_k_gpu.py, tests/test_list_metrics_gpu.py)."""
import csv
import importlib.util
import os

import numpy as np
import pytest
import torch

import metrics_at_k_ref as M
from helpers import GOLDEN


@pytest.fixture(scope='module')
def fixture():
    return dict(np.load(os.path.join(GOLDEN, 'map_at_k.npz')))


def _scores(z):
    """fp32 cosine rows of the fixture, as the reference forms them (normalise, plain fp32 product)."""
    Q = z['Q'] / np.linalg.norm(z['Q'], axis=1, keepdims=True)
    G = z['G'] / np.linalg.norm(z['G'], axis=1, keepdims=True)
    return (Q.astype(np.float64) @ G.astype(np.float64).T).astype(np.float32)


def test_numpy_reference_reproduces_compute_map_and_compute_cmc(fixture):
    z = fixture
    S = _scores(z)
    srt = -np.sort(-S.astype(np.float64), axis=1)
    assert float((srt[:, :-1] - srt[:, 1:]).min()) >= 1e-5 - 4e-7        # the generator's gap: no tie, no rounding decides a rank
    Nq, Ng = S.shape
    ks = [int(k) for k in z['map_ks']]
    assert ks == [1, 5, 20, 100] and ks[-1] > Ng > ks[-2]
    assert len(set(z['q_pid'].tolist()) - set(z['g_pid'].tolist())) == 3
    rows = [M.rows_ref(S[i], z['g_pid'], int(z['q_pid'][i]), ks) for i in range(Nq)]
    got = M.summary_ref(rows, ks, 'hits')
    for k, want in zip(ks, z['map_at']):
        assert abs(got[f'mAP@{k}'] - float(want)) <= 1e-6, (k, got[f'mAP@{k}'], want)
    assert got['num_queries@1'] < got['num_queries@5'] <= got['num_queries@100'] == Nq - 3     # hits_K == 0 does occur
    for k, want in zip(z['cmc_ks'], z['cmc_at']):
        assert sum(1 <= d['rank1'] <= int(k) for d in rows) == int(round(float(want) * Nq)), k
    # the list form of the same ranking, cut at the list length
    order = np.argsort(-S.astype(np.float64), axis=1, kind='stable')
    for K in (5, 20, Ng):
        cut = [k for k in ks if k <= K]
        for i in range(Nq):
            a, b = M.list_ref(order[i, :K], z['g_pid'], int(z['q_pid'][i]), cut), rows[i]
            assert a['hits'].tolist() == b['hits'][:len(cut)].tolist() and a['npos'] == b['npos']
            assert np.array_equal(a['sum_at'], b['sum_at'][:len(cut)])
            assert a['rank1'] == (b['rank1'] if b['rank1'] <= K else 0)


@pytest.mark.container
def test_fixture_equals_what_the_reference_computes_now(fixture):
    if not os.path.exists('/root/reference/train.py'):
        pytest.skip('reference not mounted')
    spec = importlib.util.spec_from_file_location('make_map_at_k_golden', os.path.join(GOLDEN, 'make_map_at_k_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = gen.generate()
    assert sorted(fresh) == sorted(fixture)
    for k, v in fresh.items():
        assert np.asarray(v).shape == fixture[k].shape, k
        assert float(np.abs(np.asarray(v, dtype=np.float64) - fixture[k].astype(np.float64)).max()) == 0.0, k


# ---- cutoff_summary ----------------------------------------------------------------------------------------------------------
def _hand_case():
    """Four queries, cutoffs (2, 5).  Ranks of the positives: q0: 1, 3, 9 (npos 3); q1: 4 (npos 1: no hit at K = 2); q2: none
    (npos 0); q3: 7, 8 (npos 2: no hit at either cutoff)."""
    ks = (2, 5)
    sum_at = torch.tensor([[1.0, 1.0 + 2.0 / 3.0], [0.0, 0.25], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    hits = torch.tensor([[1, 2], [0, 1], [0, 0], [0, 0]], dtype=torch.int32)
    rank1 = torch.tensor([1, 4, 0, 7], dtype=torch.int32)
    rank_last = torch.tensor([9, 4, 0, 8], dtype=torch.int32)
    npos = torch.tensor([3, 1, 0, 2], dtype=torch.int32)
    return sum_at, hits, rank1, rank_last, npos, ks


def test_cutoff_summary_hand_computed():
    from prcv2025reid_amd.evaluate import cutoff_summary
    sum_at, hits, rank1, rank_last, npos, ks = _hand_case()
    h = cutoff_summary(sum_at, hits, rank1, rank_last, npos, ks)                        # norm='hits' is the default
    assert h == cutoff_summary(sum_at, hits, rank1, rank_last, npos, ks, norm='hits')
    # 'hits': K = 2 -> only q0 (1 / 1); K = 5 -> q0 (5/3 / 2), q1 (0.25 / 1); q3 has hits_K = 0 at both and is left out
    assert h['num_queries@2'] == 1 and abs(h['mAP@2'] - 1.0) < 1e-15
    assert h['num_queries@5'] == 2 and abs(h['mAP@5'] - ((5.0 / 3.0) / 2.0 + 0.25) / 2.0) < 1e-15
    # 'min': every query with npos > 0 (q0, q1, q3); K = 2 -> 1 / min(2, 3), 0 / 1, 0 / 2; K = 5 -> (5/3) / 3, 0.25 / 1, 0 / 2
    m = cutoff_summary(sum_at, hits, rank1, rank_last, npos, ks, norm='min')
    assert m['num_queries@2'] == m['num_queries@5'] == 3
    assert abs(m['mAP@2'] - (0.5 + 0.0 + 0.0) / 3.0) < 1e-15
    assert abs(m['mAP@5'] - ((5.0 / 3.0) / 3.0 + 0.25 + 0.0) / 3.0) < 1e-15
    for r in (h, m):                                                                    # CMC and mINP do not depend on the norm
        assert abs(r['R@2'] - 1.0 / 3.0) < 1e-15 and abs(r['R@5'] - 2.0 / 3.0) < 1e-15
        assert abs(r['mINP'] - (3.0 / 9.0 + 1.0 / 4.0 + 2.0 / 8.0) / 3.0) < 1e-15
    assert set(h) == {'mAP@2', 'R@2', 'num_queries@2', 'mAP@5', 'R@5', 'num_queries@5', 'mINP'}
    assert 'mINP' not in cutoff_summary(sum_at, hits, rank1, None, npos, ks)            # lists: no last positive
    # the numpy summary used by the GPU tests is the same arithmetic
    per_query = [dict(sum_at=sum_at[i].numpy(), hits=hits[i].numpy(), rank1=int(rank1[i]), rank_last=int(rank_last[i]), npos=int(npos[i]))
                 for i in range(4)]
    for norm, got in (('hits', h), ('min', m)):
        want = M.summary_ref(per_query, ks, norm)
        assert set(want) == set(got) and all(abs(want[k] - got[k]) < 1e-15 for k in want), norm


def test_cutoff_summary_empty_means_and_refusals():
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.evaluate import cutoff_summary
    sum_at, hits, rank1, rank_last, npos, ks = _hand_case()
    none = cutoff_summary(sum_at[2:3], hits[2:3], rank1[2:3], rank_last[2:3], npos[2:3], ks, 'min')      # only the npos = 0 query
    assert none == {'mAP@2': 0.0, 'R@2': 0.0, 'num_queries@2': 0, 'mAP@5': 0.0, 'R@5': 0.0, 'num_queries@5': 0, 'mINP': 0.0}
    for bad in ((5, 2), (2, 2), (0, 5), (), tuple(range(1, 10))):
        with pytest.raises(ValueError, match='cutoffs'):
            cutoff_summary(sum_at, hits, rank1, rank_last, npos, bad)
    with pytest.raises(ValueError, match='norm'):
        cutoff_summary(sum_at, hits, rank1, rank_last, npos, ks, norm='max')
    with pytest.raises(ValueError, match='sum_at, hits'):
        cutoff_summary(sum_at, hits, rank1, rank_last, npos, (2, 5, 9))
    over = npos.clone(); over[0] = -1
    with pytest.raises(_lib.ReidHipError, match='8192'):
        cutoff_summary(sum_at, hits, rank1, rank_last, over, ks)


def test_competition_metrics_key():
    from prcv2025reid_amd.evaluate import competition_metrics
    m = {'single/nir': {'mAP': 0.2, 'mAP@100': 0.1}, 'single/sk': {'mAP': 0.4, 'mAP@100': 0.3}, 'single/cp': {'map': 0.6, 'mAP@100': 0.5},
         'single/text': {'mAP': 0.8, 'mAP@100': 0.7}, 'quad/nir+sk+cp+text': {'mAP': 0.9, 'mAP@100': 0.6}}
    d = competition_metrics(m)
    assert abs(d['map_single'] - 0.5) < 1e-12 and abs(d['map_quad'] - 0.9) < 1e-12 and abs(d['map_avg2'] - 0.7) < 1e-12
    k = competition_metrics(m, key='mAP@100')
    assert abs(k['map_single'] - 0.4) < 1e-12 and abs(k['map_quad'] - 0.6) < 1e-12 and abs(k['map_avg2'] - 0.5) < 1e-12


# ---- submission CSV -----------------------------------------------------------------------------------------------------------
def _write(path, rows):
    with open(path, 'w', newline='') as f:                     # the writer of ProtocolEvaluator.export_submission_csv
        w = csv.writer(f)
        w.writerow(['query_key', 'ranked_gallery_ids'])
        for key, names in rows:
            w.writerow([key, ' '.join(names)])


def test_submission_csv_round_trip_and_error_lines(tmp_path):
    from prcv2025reid_amd.evaluate import parse_submission_csv
    names = [f'img_{i:03d}.jpg' for i in range(6)] + [None, 7]              # a row without a name, a name that is not a string
    pids = {'q,1': 11, 'q2': 12, 'q3': 13}                                  # (a key the csv module has to quote)
    p = str(tmp_path / 'sub.csv')
    _write(p, [('q2', [names[3], names[0], '7']), ('q,1', [names[5]]), ('q3', [])])
    rows, got = parse_submission_csv(p, pids, names)
    assert rows == [[3, 0, 7], [5], []] and got == [12, 11, 13]
    _write(p, [('q2', [names[1]]), ('q9', [names[2]])])
    with pytest.raises(ValueError, match=r"sub\.csv:3: unknown query key 'q9'"):
        parse_submission_csv(p, pids, names)
    _write(p, [('q2', [names[1]]), ('q3', [names[2]]), ('q,1', [names[4], 'img_999.jpg'])])
    with pytest.raises(ValueError, match=r"sub\.csv:4: unknown gallery image 'img_999\.jpg'"):
        parse_submission_csv(p, pids, names)
    with open(p, 'w') as f:
        f.write('key,ids\nq2,img_000.jpg\n')
    with pytest.raises(ValueError, match=r'sub\.csv:1: expected the header'):
        parse_submission_csv(p, pids, names)
    _write(p, [])
    with pytest.raises(ValueError, match='no query rows'):
        parse_submission_csv(p, pids, names)


# ---- declarations --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_python_binds_the_two_entry_points():
    import ctypes
    from prcv2025reid_amd import _lib, ops
    from test_cabi_cpu import ctype_of, header_macro, header_prototypes
    protos = header_prototypes()
    for name, n_args in (('reid_rank_metrics_at', 21), ('reid_list_metrics', 19)):
        assert name in protos and name in _lib.SIGNATURES, name
        ret, params = protos[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(params) == len(argtypes) == n_args, name
        assert (restype, list(argtypes)) == (ctype_of(ret), [ctype_of(p) for p in params]), name
    # the old entry point keeps its signature: the new one is that signature plus (cutoffs, n_cut) and three outputs
    old, new = ([' '.join(p.split()) for p in protos[n][1]] for n in ('reid_rank_metrics', 'reid_rank_metrics_at'))
    assert len(old) == 16 and new[:12] == old[:12] and new[14:17] == old[12:15] and new[-1] == old[-1]
    assert header_macro('REID_METRICS_MAX_CUTOFFS') == ops.METRICS_MAX_CUTOFFS == 8
    assert header_macro('REID_ROWS_TOPK_MAX_K') == ops.ROWS_TOPK_MAX_K
    assert (header_macro('REID_LIST_BAD_NEGATIVE'), header_macro('REID_LIST_BAD_RANGE'), header_macro('REID_LIST_BAD_ORDER')) == \
        (ops.LIST_BAD_NEGATIVE, ops.LIST_BAD_RANGE, ops.LIST_BAD_ORDER)
    assert header_macro('REID_ABI_VERSION') == _lib.ABI_VERSION == 201
    cut = ops.check_cutoffs((1, 5, 100))
    assert isinstance(cut, ctypes.Array) and list(cut) == [1, 5, 100] and ctypes.sizeof(cut) == 12
    with pytest.raises(ValueError, match='beyond the list length 64'):
        ops.check_cutoffs((1, 100), limit=64)


def test_entry_points_refuse_bad_cutoffs_before_any_launch():
    # host-side argument checks of the library itself: no device is touched (null stream, never reached)
    import ctypes
    from prcv2025reid_amd import _lib, build
    build.build(verbose=False)
    h = _lib.bind(ctypes.CDLL(_lib.LIB_PATHS['bf16']))
    buf = (ctypes.c_int32 * 64)()
    a = ctypes.addressof(buf)
    def at(cut):
        c = (ctypes.c_int32 * len(cut))(*cut)
        return h.reid_rank_metrics_at(a, 64, a, None, a, a, None, a, a, 1, 64, 1, ctypes.addressof(c), len(cut), a, a, a, a, a, a, None)
    def lst(cut, k=8):
        c = (ctypes.c_int32 * len(cut))(*cut)
        return h.reid_list_metrics(a, 1, k, a, None, a, a, None, a, a, 64, ctypes.addressof(c), len(cut), a, a, a, a, a, None)
    for cut, msg in (((5, 1), b'strictly ascending'), ((0, 1), b'strictly ascending'), ((3, 3), b'strictly ascending'),
                     (tuple(range(1, 10)), b'n_cut=9')):
        assert at(cut) == -1 and msg in h.reid_last_error(), cut
        assert lst(cut, k=16) == -1 and msg in h.reid_last_error(), cut
    assert lst((1, 9), k=8) == -1 and b'beyond the list length k=8' in h.reid_last_error()
    assert lst((1,), k=1025) == -1 and b'k=1025 outside 1..1024' in h.reid_last_error()
    assert h.reid_list_metrics(None, 1, 8, a, None, a, a, None, a, a, 64, a, 1, a, a, a, a, a, None) == -1 and b'null pointer' in h.reid_last_error()
