"""CPU: the fixtures of test_retrieval_exact_gpu.py hold what they claim (retrieval_ref.py) -- the bit budget, tie groups that straddle
rank k across tiles, chunks and the end of the sample, group sizes relative to cap_for and SELECT_SV, the exclusion cases, the gaps and
the scrambled 16-bit order of the rounded fixture -- and ``ranking`` is the stable descending sort."""
import numpy as np
import pytest
import torch

import retrieval_ref as R
from helpers import assert_bit_budget, round16

CASES = R.all_cases(256) + R.scan_cases(304)[-4:]                      # two compute-unit counts: the scan galleries follow the device
ROUNDED = sorted(R.ROUNDED_SEEDS)


def test_cap_for_and_workspace_match_the_library():
    assert [R.cap_for(*a) for a in ((100, 1), (8192, 10), (8193, 10), (200000, 10), (200000, 100), (40000, 1024))] == \
        [256, 256, 256, 6 * 10 * 25 + 64, 8192, 8192]
    try:
        from prcv2025reid_amd import _lib
        fn = _lib.lib().reid_topk_ws_bytes
    except Exception:                                             # no built library here: the restatement stands alone
        return
    for Nq, Ng, k in ((1, 6144, 1), (5, 8193, 10), (128, 200000, 10), (2100, 32000, 10), (3, 1500, 1024), (7, 57400, 10)):
        assert int(fn(Nq, Ng, k)) == R.topk_ws_bytes(Nq, Ng, k)


def test_ranking_is_the_stable_descending_sort():
    rng = np.random.default_rng(1)
    Q = rng.integers(-2, 3, (7, 16)).astype(np.float64)
    G = rng.integers(-2, 3, (300, 16)).astype(np.float64)
    G[250:] = G[:50]                                              # exact ties
    exq = np.array([-1, 3, 4, -1, 5, 3, 9], np.int32)
    exg = rng.integers(-1, 6, 300).astype(np.int32)
    exg[:] = np.where(np.arange(300) % 3 == 0, exg, 3)            # id 3 leaves 100 rows at most; id 9 matches nothing
    for k in (1, 10, 150, 300):
        for ids in ((exq, exg), (None, None)):
            idx, sc = R.ranking(Q, G, ids[0], ids[1], k)
            sim = torch.from_numpy(Q @ G.T)
            if ids[0] is not None:
                sim = sim.masked_fill(torch.from_numpy((exq[:, None] >= 0) & (exq[:, None] == exg[None, :])), -1e9)
            want_s, want_i = torch.sort(sim, dim=1, descending=True, stable=True)
            assert np.array_equal(idx, want_i[:, :k].numpy()) and np.array_equal(sc, want_s[:, :k].numpy()), k
    idx, sc = R.ranking(Q, G, exq, exg, 300)
    n3 = int((exg == 3).sum())
    assert (sc[1, 300 - n3:] == R.EXCLUDED).all() and (np.diff(idx[1, 300 - n3:]) > 0).all()      # excluded rows last, in index order
    assert np.array_equal(R.bits(np.float32(-1e9)), R.bits(R.EXCLUDED)) and float(np.float32(-1e9)) == -1e9


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_exact_fixture(case):
    fx = case.fixture()
    Q, G, k, Ng = fx.Q, fx.G, fx.k, fx.Ng
    # representable in both 16-bit formats, and every partial sum exact in fp32
    for x in (Q, G):
        xt = torch.from_numpy(np.array(x))
        assert torch.equal(round16(xt, 'bf16'), xt) and torch.equal(round16(xt, 'f16'), xt)
    assert_bit_budget(torch.from_numpy(np.abs(Q) @ np.abs(G).max(0)), fx.quantum())          # (bounds sum_i |Q[q, i] G[g, i]| of every pair)
    norms = np.linalg.norm(G, axis=1)
    assert 0.4 < np.median(norms) < 1.5
    assert np.array_equal(fx.score, fx.score.astype(np.float32).astype(np.float64))
    # expectations in the contract's order
    assert ((fx.score[:, :-1] > fx.score[:, 1:]) | ((fx.score[:, :-1] == fx.score[:, 1:]) & (fx.idx[:, :-1] < fx.idx[:, 1:]))).all()
    cap = R.cap_for(Ng, k)
    ties = [q for q, kd in enumerate(fx.kind) if kd in R.TIE_KINDS]
    if Ng >= 2 * k + 128:
        assert ties and ties[0] == 0
    spread = last = False
    for q in ties:
        tied = fx.tied_with_kth(q)
        if len(tied) == 0:                                        # (a two-row group displaced by a later plant, or k == Ng)
            assert fx.kind[q] == 'tie2' or k == Ng, (q, fx.kind[q])
            continue
        # the k-th and (k+1)-th rows tie exactly; the group lies in several 32-row tiles, 64-row chunks (= workgroups: consecutive
        # chunks go to consecutive workgroups) and on both sides of the sample's end
        sides = Ng <= R.SAMPLE or (tied.min() < R.SAMPLE <= tied.max())
        spread |= len(set(tied // 32)) > 1 and len(set(tied // 64)) > 1 and bool(sides)
        last |= (Ng - 1) in tied
        if fx.kind[q] == 'tie513':
            assert len(tied) > R.SELECT_SV
        if fx.kind[q] == 'tieCap':
            assert len(tied) > cap
    if any(R.tie_size(fx.kind[q], Ng, k) > k for q in ties):     # (a group of more than k copies of the best row cannot be displaced)
        assert spread and last, (spread, last)
    for q, kd in enumerate(fx.kind):
        row = R.similarity(Q[q:q + 1], G, None if fx.exq is None else fx.exq[q:q + 1], fx.exg)[0]
        plain = Q[q] @ G.T
        if kd == 'zero':
            assert not Q[q].any() and np.array_equal(fx.idx[q], np.arange(k)) and not fx.score[q].any()
        elif kd == 'neg':
            assert (G >= 0).all() and (Q[q] <= 0).all() and (plain < 0).all() and (fx.score[q] < 0).all()
        elif kd == 'ex3':
            best3 = np.argsort(-plain, kind='stable')[:3]
            assert (row[best3] == R.EXCLUDED).all() and (fx.exg == 7).sum() == 3
            assert not np.isin(best3, fx.idx[q]).any() or k > Ng - 3
        elif kd == 'exPart':
            assert Ng < 100 or (0 < (row == R.EXCLUDED).sum() < Ng - k and (fx.score[q] > R.EXCLUDED).all())
        elif kd == 'exAlone':
            assert fx.exq[q] >= 0 and not (fx.exg == fx.exq[q]).any() and np.array_equal(row, plain)
        elif kd == 'exFew':
            usable = int((row > R.EXCLUDED).sum())
            assert usable < k and usable == min(k - 1, 5)
            assert (fx.score[q, usable:] == R.EXCLUDED).all() and np.array_equal(fx.idx[q, usable:], np.flatnonzero(row == R.EXCLUDED)[:k - usable])
        elif kd == 'exAll':
            assert (row == R.EXCLUDED).all() and np.array_equal(fx.idx[q], np.arange(k))
        elif kd == 'far':
            assert fx.idx[q].min() >= R.SAMPLE
        elif kd == 'near':
            assert fx.idx[q].max() < R.SAMPLE
        elif fx.exq is not None and fx.exq[q] < 0:
            assert (fx.exg == -1).any() or fx.excl == 'all'
            assert np.array_equal(row, plain)                      # -1 on both sides excludes nothing
    if Ng >= R.SAMPLE + 2 * k + 16 and not fx.neg and fx.Nq >= 12:
        assert 'far' in fx.kind and 'near' in fx.kind
    for kd in case.complete:                                      # fits the candidate list in both flavors, whatever the threshold kernel popped
        q = fx.kind.index(kd)
        assert max(R.tiled_candidates(fx, q, f) for f in ('bf16', 'f16')) <= cap, (R.tiled_candidates(fx, q, 'bf16'), cap)
    assert set(fx.must_flag(True)) >= set(fx.must_flag(False))


def test_the_gpu_checker_rejects_wrong_lists():
    """check_lists of test_retrieval_exact_gpu.py accepts the expected lists and nothing near them."""
    from test_retrieval_exact_gpu import MARK, check_lists
    fx = R.exact_fixture(6, 1024, 512, 4, 2, 'main')
    good_i, good_s = fx.idx.copy(), fx.score.astype(np.float32)
    assert check_lists(fx, good_i, good_s, may_flag=False)[1] == 0.0
    q, r = np.argwhere(fx.score[:, :-1] == fx.score[:, 1:])[0]

    def rejected(idx, sc, fixture=fx, **kw):
        with pytest.raises(AssertionError):
            check_lists(fixture, idx, sc, **kw)
    swapped = good_i.copy(); swapped[q, [r, r + 1]] = swapped[q, [r + 1, r]]
    rejected(swapped, good_s)                                     # a tie in the wrong index order
    ulp = good_s.copy(); ulp[3, 1] = np.nextafter(ulp[3, 1], np.float32(2))
    rejected(good_i, ulp)                                         # one unit in the last place
    minus = good_s.copy(); minus[fx.kind.index('zero'), 0] = -0.0
    rejected(good_i, minus)                                       # the sign of a zero score
    flagged_i, flagged_s = good_i.copy(), good_s.copy()
    flagged_i[2] = MARK; flagged_i[2, 0] = -2; flagged_s[2, 0] = 0
    check_lists(fx, flagged_i, flagged_s)
    rejected(flagged_i, flagged_s, may_flag=False)
    rejected(flagged_i, flagged_s, complete=[2])
    rejected(good_i, good_s, must_flag=[2])
    half = flagged_i.copy(); half[2, 1] = good_i[2, 1]
    rejected(half, flagged_s)                                     # a flagged row with more than its marker written
    fr = R.rounded_fixture(*ROUNDED[0])
    ri, rs = fr.idx.copy(), fr.score.astype(np.float32)
    assert 0 < check_lists(fr, ri, rs, may_flag=False)[1] <= 1.0   # (the rounding of the reference to fp32 is within b)
    off = rs.copy(); off[0, 4] += np.float32(4e-6)
    rejected(ri, off, fixture=fr)                                 # beyond the bound (and out of its own order)
    twin = ri.copy(); twin[2, [0, 1]] = twin[2, [1, 0]]
    rejected(twin, rs, fixture=fr)                                # the bit-identical pair in the wrong order


def test_every_planted_kind_meets_every_path():
    for path in ('scan', 'tiled', 'stream'):
        kinds = set()
        for c in R.all_cases(256):
            if c.path == path:
                kinds |= set(c.fixture().kind)
        want = set(R.TIE_KINDS) | {'zero', 'neg', 'ex3', 'exPart', 'exAlone', 'exFew', 'exAll'}
        if path != 'stream':
            want |= {'far', 'near'}
        assert kinds >= want, (path, want - kinds)


@pytest.mark.parametrize('key', ROUNDED, ids=[str(k) for k in ROUNDED])
def test_rounded_fixture(key):
    Nq, Ng, D, k = key
    fx = R.rounded_fixture(*key)
    assert R.find_rounded_seed(*key) == R.ROUNDED_SEEDS[key] and R.gaps_ok(fx.Q, fx.G, k)
    for x in (fx.Q, fx.G):                                        # fp32 values, unit rows
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
        assert np.abs(np.linalg.norm(x, axis=1) - 1).max() < 1e-6
    sim = R.similarity(fx.Q, fx.G)
    assert fx.bound.max() < 2e-6 and fx.bound.min() > 0
    assert fx.idx[2, 0] < fx.idx[2, 1] == Ng - 1 and fx.score[2, 0] == fx.score[2, 1]         # the bit-identical pair, tied exactly
    for q, n in enumerate(R.CLUSTERS):
        # the narrower band of the two flavors under the k-th score holds most of the cluster: hundreds of rows the 16-bit scores
        # cannot order, a few 1e-4 apart
        band = int((sim[q] >= fx.score[q, k - 1] - 2 * R.EPS16['f16']).sum())
        assert 0.6 * n <= band <= n + k and fx.score[q, 0] - fx.score[q, k - 1] < 1e-3
        d = -np.diff(fx.score[q])
        assert d.min() > 2e-6 and d.max() < 1e-3
        assert int((sim[q] >= fx.score[q, k - 1] - 2 * R.EPS16['bf16']).sum()) <= n + k
        for fmt in ('bf16', 'f16'):                               # ranking by the 16-bit operands gets these queries wrong
            Qr = round16(torch.from_numpy(np.array(fx.Q)), fmt).numpy()
            Gr = round16(torch.from_numpy(np.array(fx.G)), fmt).numpy()
            assert not np.array_equal(R.ranking(Qr[q:q + 1], Gr, None, None, k)[0][0], fx.idx[q]), (q, fmt)
    assert band <= R.cap_for(Ng, k) < R.CLUSTERS[0]                # the second cluster fits the candidate list, the first cannot
