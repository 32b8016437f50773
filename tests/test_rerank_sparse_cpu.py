"""CPU: the list / dictionary restatement of re-ranking (tests/rerank_sparse_ref.py) equals the dense fp64 one, and the sparse
form's parameter checks refuse what cannot run before anything touches a device."""
import os
import re
import time

import numpy as np
import pytest
import torch

import rerank_ref as R
import rerank_sparse_ref as RS


def dense_rows(rows, N):
    M = np.zeros((len(rows), N))
    for i, r in enumerate(rows):
        M[i, list(r)] = [float(v) for v in r.values()]
    return M


@pytest.mark.parametrize('name', ['exact', 'gauss'])
def test_list_reference_equals_the_dense_reference(name):
    X, Nq, k1, k2 = (R.exact_fixture(0)[0], 32, 20, 6) if name == 'exact' else (R.gaussian_fixture(422, 32, 219, 64, 24, 2.2)[0], 32, 8, 3)
    want = R.rerank_ref(X, Nq, k1, k2, 0.3)
    got = RS.sparse_ref(X, want['nbr'], Nq, k1, k2, 0.3)
    assert got['R'] == want['R'] and got['Rh'] == want['Rh'] and got['Rstar'] == want['Rstar']
    N = X.shape[0]
    assert [list(v) for v in got['V']] == want['Rstar']                       # V rows in R* order
    V, V2 = dense_rows(got['V'], N), dense_rows(got['V2'], N)
    assert np.array_equal(V != 0, want['V'] != 0) and np.array_equal(V2 != 0, want['V2'] != 0)
    assert np.abs(V - want['V']).max() < 1e-12 and np.abs(V2 - want['V2']).max() < 1e-12
    assert np.abs(got['s'] - want['s']).max() < 1e-12
    # the fp32 run: same sets, values at fp32 distance
    got32 = RS.sparse_ref(X, want['nbr'], Nq, k1, k2, 0.3, np.float32)
    assert got32['Rstar'] == want['Rstar'] and got32['s'].dtype == np.float32
    assert 0 < RS.gate(got, got32) < 1e-5


def test_list_reference_is_quick_beyond_the_dense_limit():
    # N = 65 552, k1 = 6: lists that are reciprocal by construction (blocks of 8 consecutive rows), seconds on the CPU
    N, D = 65552, 8
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, D)); X /= np.linalg.norm(X, axis=1, keepdims=True)
    blk = np.arange(N) // 8 * 8
    nbr = np.stack([np.arange(N)] + [blk + (np.arange(N) % 8 + t) % 8 for t in range(1, 7)], 1)
    t0 = time.perf_counter()
    r = RS.sparse_ref(X, nbr, 16, 6, 3, 0.3)
    took = time.perf_counter() - t0
    print(f'  sparse_ref at N = {N}: {took:.1f} s')
    assert took < 60 and len(r['V2']) == N and r['s'].shape == (16, N - 16)
    assert all(abs(sum(v.values()) - 1) < 1e-12 for v in r['V2'][:64])


def test_sparse_parameter_checks_run_before_a_device_is_touched():
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.rerank import SPARSE_MERGE_MAX, RerankParams, list_width, rerank_scores
    assert RerankParams() == RerankParams(k1=20, k2=6, lambda_value=0.3) and RerankParams().sparse is False
    assert RerankParams(20, 6, 0.3, True).sparse is True               # placed last
    assert SPARSE_MERGE_MAX >= 4096 and SPARSE_MERGE_MAX >= 21 * list_width(20)      # k2 = k1 + 1 at the default k1 fits
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'reid_hip.h')).read()
    assert int(re.search(r'#define\s+REID_RERANK_MERGE_MAX\s+(\d+)', header).group(1)) == SPARSE_MERGE_MAX      # the kernels' constant
    assert [list_width(k) for k in (1, 6, 8, 20, 30, 64)] == [(k + 1) * (R.kh_of(k) + 2) for k in (1, 6, 8, 20, 30, 64)]
    assert 6 * list_width(20) == 1512 and 6 * list_width(30) == 3162
    sp = lambda **kw: RerankParams(sparse=True, **kw)
    with pytest.raises(_lib.ReidHipError, match='exceeds 65536 rows'):
        rerank_scores(torch.zeros(1537, 64), torch.zeros(64000, 64), RerankParams(sparse=False))
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):       # the row limit is gone
        rerank_scores(torch.zeros(1537, 64), torch.zeros(64000, 64), sp())
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), sp(k1=30, k2=6))
    with pytest.raises(_lib.ReidHipError, match=r'k1 \+ 1 = 21 neighbours asked of N = 20'):
        rerank_scores(torch.zeros(4, 64), torch.zeros(16, 64), sp())
    with pytest.raises(_lib.ReidHipError, match='k1=65'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), sp(k1=65))
    with pytest.raises(_lib.ReidHipError, match='k2=10'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), sp(k1=8, k2=10))
    with pytest.raises(_lib.ReidHipError, match='lambda=1.5'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), sp(lambda_value=1.5))
    with pytest.raises(_lib.ReidHipError, match=rf'k1=64 k2=65 merge .* = {65 * 2210} entries per row, more than SPARSE_MERGE_MAX = {SPARSE_MERGE_MAX}'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), sp(k1=64, k2=65))
    # the dense form takes the same parameters
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), RerankParams(k1=64, k2=65))


def test_sparse_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    h = _lib.bind(ctypes.CDLL(_lib.LIB_PATHS['bf16']))
    assert list(_lib.SIGNATURES)[-7:-3] == ['reid_rerank_weights_sparse', 'reid_rerank_expand_count', 'reid_rerank_expand_sparse',
                                           'reid_rerank_jaccard_sparse']
    p = 4096                                                      # a non-null stand-in: nothing is launched
    W = 21 * 12
    assert h.reid_rerank_weights_sparse(p, 80, p, 64, p, p, p, W, 100000, 64, 65, None) == -1 and b'reid_rerank_weights_sparse: k1=65' in h.reid_last_error()
    assert h.reid_rerank_weights_sparse(p, 80, p, 64, p, p, p, W - 1, 100000, 64, 20, None) == -1 and b'ldw >= W = 252' in h.reid_last_error()
    assert h.reid_rerank_weights_sparse(p, 80, p, 64, p, None, p, W, 100000, 64, 20, None) == -1 and b'null pointer' in h.reid_last_error()
    assert h.reid_rerank_expand_count(p, p, p, 2210, p, 80, p, 256, 64, 65, None) == -1 and b'reid_rerank_expand_count: k1=64 k2=65 merge' in h.reid_last_error()
    assert b'at most 8192' in h.reid_last_error()
    assert h.reid_rerank_expand_sparse(p, p, p, 2210, p, 80, p, p, p, 256, 64, 4, None) == -1 and b'= 8840 entries per row, at most 8192' in h.reid_last_error()
    assert h.reid_rerank_expand_sparse(p, p, p, W, p, 80, None, p, p, 256, 20, 6, None) == -1 and b'reid_rerank_expand_sparse: null pointer' in h.reid_last_error()
    assert h.reid_rerank_expand_count(p, p, p, W, p, 80, p, 256, 20, 22, None) == -1 and b'k2=22' in h.reid_last_error()
    assert h.reid_rerank_jaccard_sparse(p, p, p, 10, p, p, p, 10, None, 224, p, 224, 32, 224, 256, 0.3, None) == -1 and b'null pointer' in h.reid_last_error()
    assert h.reid_rerank_jaccard_sparse(p, p, p, 10, p, p, p, 10, p, 224, p, 226, 32, 224, 256, 0.3, None) == -1 and b'ldo' in h.reid_last_error()
