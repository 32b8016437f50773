"""CPU: the fp64 restatement of k-reciprocal re-ranking checks itself, the three entry points are bound and exported, and
``rerank_scores`` refuses what cannot run before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

import rerank_ref as R

NEW = ['reid_rerank_weights', 'reid_rerank_expand', 'reid_rerank_jaccard']


@pytest.fixture(scope='module')
def gauss():
    X, qp, gp = R.gaussian_fixture(422, 32, 219, 64, 24, 2.2)
    return X, qp, gp, R.rerank_ref(X, 32, k1=8, k2=3, lam=0.3)


def test_rows_of_v_and_v2_sum_to_one(gauss):
    _, _, _, r = gauss
    assert np.abs(r['V'].sum(1) - 1).max() < 1e-14 and np.abs(r['V2'].sum(1) - 1).max() < 1e-14
    assert (r['V'] >= 0).all() and all((r['V'][i] > 0).sum() == len(m) == len(set(m)) for i, m in enumerate(r['Rstar']))
    # the expansion is exercised, and the sets stay inside the bound the kernel sizes its list by
    assert sum(len(a) > len(b) for a, b in zip(r['Rstar'], r['R'])) > 10
    assert max(len(m) for m in r['Rstar']) <= (8 + 1) * (R.kh_of(8) + 2)


def test_k2_one_leaves_v(gauss):
    X = gauss[0]
    r = R.rerank_ref(X, 32, k1=8, k2=1)
    # nbr[i, 0] is i itself unless an equal row with a lower index exists, which then has the same V row
    assert np.array_equal(r['V2'], r['V'])


def test_lambda_one_is_the_cosine_order(gauss):
    X = gauss[0]
    r = R.rerank_ref(X, 32, k1=8, k2=3, lam=1.0)
    assert np.array_equal(r['s'], r['cos'][:32, 32:])
    assert np.array_equal(R.ranking(r['s']), R.ranking(r['cos'][:32, 32:]))


def test_kh_rounds_half_to_even():
    assert [R.kh_of(k) for k in (1, 2, 3, 5, 6, 7, 8, 20, 63, 64)] == [0, 1, 2, 2, 3, 4, 4, 10, 32, 32]


def test_six_points_on_a_circle():
    # angles 0, 10, 25 | 100, 112 | 180 degrees, k1 = 2 (kh = 1): every list is the point and its two nearest
    ang = np.deg2rad([0, 10, 25, 100, 112, 180])
    X = np.stack([np.cos(ang), np.sin(ang)], 1)
    r = R.rerank_ref(X, 2, k1=2, k2=1)
    assert r['nbr'][:, :3].tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 4, 2], [4, 3, 5], [5, 4, 3]]
    # 2 is in 3's list but 3 is not in 2's; 3 is in 5's list but 5 is not in 3's
    assert r['R'] == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 4], [4, 3, 5], [5, 4]]
    # kh = 1: 1 is 2's nearest but 0 is 1's; 4 is 5's nearest but 3 is 4's
    assert r['Rh'] == [[0, 1], [1, 0], [2], [3, 4], [4, 3], [5]]
    # every accepted R(j, 1) lies inside R(i, 2) already; for i = 5, R(4, 1) = {4, 3} meets {5, 4} in one of two: refused
    assert r['Rstar'] == r['R']
    assert abs(r['V'][5, 4] - np.exp(np.cos(ang[5] - ang[4]) - 1) / (1 + np.exp(np.cos(ang[5] - ang[4]) - 1))) < 1e-15


def test_expansion_adds_a_set_that_overlaps_by_more_than_two_thirds():
    # hand-made lists (no geometry): k1 = 6, kh = 3.  R(0, 6) = {0..5}; R(1, 3) = {1, 2, 3, 7} has 3 of 4 inside: 9 > 8, so 7 joins;
    # R(2, 3) = {2, 8, 9, 1} has 2 of 4 inside: 6 > 8 fails, so 8 and 9 stay out
    N = 10
    nbr = np.zeros((N, N), dtype=np.int64)
    lists = {0: [0, 1, 2, 3, 4, 5, 6], 1: [1, 2, 3, 7, 0, 4, 5], 2: [2, 8, 9, 1, 0, 3, 4], 3: [3, 1, 0, 2, 4, 5, 6],
             4: [4, 0, 5, 6, 1, 2, 3], 5: [5, 0, 4, 6, 1, 2, 3], 6: [6, 7, 8, 9, 4, 5, 3], 7: [7, 1, 6, 8, 9, 2, 3],
             8: [8, 2, 9, 6, 7, 0, 1], 9: [9, 2, 8, 6, 7, 0, 1]}
    for i, head in lists.items():
        nbr[i] = head + [j for j in range(N) if j not in head]
    X = np.eye(N)
    r = R.rerank_ref(X, 2, k1=6, k2=1, nbr=nbr)
    assert r['R'][0] == [0, 1, 2, 3, 4, 5]                      # 6's list does not hold 0
    assert r['Rh'][1] == [1, 2, 3, 7] and r['Rh'][2] == [2, 8, 9, 1]
    assert r['Rstar'][0] == [0, 1, 2, 3, 4, 5, 7]


def test_exact_fixture_has_ties_in_every_list():
    X, _, _ = R.exact_fixture()
    assert np.array_equal(np.abs(X), np.full_like(X, 0.125))
    c64 = X @ X.T
    c32 = X.astype(np.float32) @ X.astype(np.float32).T
    assert np.array_equal(c64, c32.astype(np.float64)) and np.array_equal(np.diag(c64), np.ones(256))
    top = -np.sort(-c64, axis=1)[:, :21]
    assert ((top[:, :-1] == top[:, 1:]).any(1)).all()            # an exact tie inside the first k1 + 1 = 21 of every row


def test_new_entry_points_are_bound_and_exported():
    from prcv2025reid_amd import build, _lib
    assert list(_lib.SIGNATURES)[-3:] == NEW
    build.build(verbose=False)
    for flavor, path in _lib.LIB_PATHS.items():
        h = _lib.bind(ctypes.CDLL(path))
        assert all(hasattr(h, n) for n in NEW), flavor
        assert h.reid_version() == 201


def test_argument_errors_need_no_gpu():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    h = _lib.bind(ctypes.CDLL(_lib.LIB_PATHS['bf16']))
    p = 4096                                                      # a non-null, 16-byte aligned stand-in: nothing is launched
    assert h.reid_rerank_weights(p, 80, p, 64, p, 256, 256, 64, 65, None) == -1 and b'k1=65' in h.reid_last_error()
    assert h.reid_rerank_weights(p, 80, p, 64, p, 8, 8, 64, 8, None) == -1 and b'k1 + 1 = 9' in h.reid_last_error()
    assert h.reid_rerank_weights(None, 80, p, 64, p, 256, 256, 64, 8, None) == -1 and b'null pointer' in h.reid_last_error()
    assert h.reid_rerank_expand(p, 256, p, 80, p, 256, 256, 8, 10, None) == -1 and b'k2=10' in h.reid_last_error()
    assert h.reid_rerank_expand(p, 256, None, 80, p, 256, 256, 8, 3, None) == -1 and b'null pointer' in h.reid_last_error()
    assert h.reid_rerank_jaccard(p, 256, p, 256, None, 224, p, 224, 32, 224, 256, 0.3, None) == -1 and b'null pointer' in h.reid_last_error()
    assert h.reid_rerank_jaccard(p, 256, p, 256, p, 224, p, 226, 32, 224, 256, 0.3, None) == -1 and b'ldo' in h.reid_last_error()


def test_rerank_scores_refuses_before_touching_a_device():
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.rerank import RerankParams, rerank_scores
    assert RerankParams() == RerankParams(k1=20, k2=6, lambda_value=0.3)
    with pytest.raises(_lib.ReidHipError, match='exceeds 65536 rows'):
        rerank_scores(torch.zeros(1537, 64), torch.zeros(64000, 64))
    with pytest.raises(_lib.ReidHipError, match=r'k1 \+ 1 = 21 neighbours asked of N = 20'):
        rerank_scores(torch.zeros(4, 64), torch.zeros(16, 64))
    with pytest.raises(_lib.ReidHipError, match='k1=65'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), RerankParams(k1=65))
    with pytest.raises(_lib.ReidHipError, match='k2=10'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64), RerankParams(k1=8, k2=10))
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        rerank_scores(torch.zeros(40, 64), torch.zeros(160, 64))
