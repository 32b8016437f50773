"""reid_expand_rows without a GPU: the float32 restatement of its definition (expansion_ref.py) against an independent float64 formula
and against cases worked by hand, the host-side refusals of the bound library, and the argument checks of the Python layers."""
import ctypes

import numpy as np
import pytest
import torch

import expansion_ref as E

F32 = np.float32
NAN = F32(np.nan)


@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import _lib, build
    build.build(verbose=False)
    return {f: _lib.bind(ctypes.CDLL(p)) for f, p in _lib.LIB_PATHS.items()}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def unit_rows(rng, n, D):
    v = rng.standard_normal((n, D))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


@pytest.mark.parametrize('alpha', [0, 1, 3, 16])
@pytest.mark.parametrize('k,kl,self_base', [(1, 1, -1), (10, 11, 0), (10, 11, 7), (64, 64, -1), (5, 20, -1)])
def test_float32_loop_is_within_its_derived_allowance_of_the_float64_formula(alpha, k, kl, self_base):
    rng = np.random.default_rng(1000 * alpha + 10 * k + kl)
    rows, M, D = 37, 90, 24
    x, table = unit_rows(rng, rows, D), unit_rows(rng, M, D)
    nbr, score = E.random_lists(rng, rows, kl, M, self_base)
    raw = E.expand_rows_ref(x, table, nbr, score, k, alpha, self_base)
    ref, allow = E.expand_rows_f64(x, table, nbr, score, k, alpha, self_base)
    assert raw.dtype == F32 and not np.isnan(raw).any()
    ratio = np.abs(raw.astype(np.float64) - ref) / allow
    print(f'alpha={alpha} k={k} kl={kl} self_base={self_base}: worst error / allowance = {ratio.max():.3f}')
    assert ratio.max() <= 1.0, f'worst error / allowance = {ratio.max():.3f}'
    assert np.abs(ref - x).max() > 0.01 or k == 1          # (the lists do add rows: the comparison is not x against x)


# ---- cases by hand: table rows and x of small integers, weights that are powers of two or 1 + m 2^-23: every expected value is exact
TABLE = np.array([[j + 1, 2 * (j + 1), -(j + 1), 0.25] for j in range(6)], F32)        # M = 6
X1 = np.array([[1, 2, 3, 4]], F32)


def run(nbr, score, k, alpha, self_base=-1, x=X1):
    return E.expand_rows_ref(x, TABLE, np.array(nbr, np.int32), np.array(score, F32), k, alpha, self_base)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(np.asarray(want, F32)))


def test_entries_outside_the_table_are_skipped_and_do_not_count():
    got = run([[-1, 7, 6, 2, 0, 1]], [[.9, .8, .7, .6, .5, .4]], k=2, alpha=0)
    assert same_bits(got, X1 + TABLE[2] + TABLE[0])                           # -1, 7 and 6 (= M) skipped; rows 2 and 0 are the first two
    got = run([[-1, 7, 6, 2, 0, 1]], [[.5, .5, .5, .5, .25, .125]], k=3, alpha=1)
    assert same_bits(got, X1 + 0.5 * TABLE[2] + 0.25 * TABLE[0] + 0.125 * TABLE[1])


@pytest.mark.parametrize('pos', [0, 1, 2])
def test_self_entry_is_dropped_by_index_at_any_position(pos):
    others = [1, 2]
    row = others[:pos] + [3] + others[pos:]                                   # self_base = 3, row 0: index 3 is the row itself
    got = run([row], [[.5, .5, .5]], k=2, alpha=1, self_base=3)
    assert same_bits(got, X1 + 0.5 * TABLE[1] + 0.5 * TABLE[2])
    assert same_bits(run([row], [[.5, .5, .5]], k=3, alpha=1, self_base=3), got)        # fewer than k eligible entries: the same two
    # without a self index, or for another row of the chunk, index 3 is an ordinary neighbour (k = 2: whichever two come first)
    first2 = row[:2]
    assert same_bits(run([row], [[.5, .5, .5]], k=2, alpha=1), X1 + 0.5 * TABLE[first2[0]] + 0.5 * TABLE[first2[1]])
    x2 = np.array([[0, 0, 0, 0], [1, 2, 3, 4]], F32)
    got2 = run([[5, 5, 5], row], [[0, 0, 0], [.5, .5, .5]], k=2, alpha=1, self_base=2, x=x2)   # row 1 of a chunk at 2: self = 3
    assert same_bits(got2[1], (X1 + 0.5 * TABLE[1] + 0.5 * TABLE[2])[0]) and same_bits(got2[0], x2[0])


def test_score_classes():
    # NaN: not eligible, does not count.  Negative and zero (either sign): eligible, count towards k, weight 0 for alpha >= 1: not added
    nbr = [[0, 1, 2, 3, 4]]
    score = [[NAN, -0.25, 0.0, -0.0, 0.5]]
    assert same_bits(run(nbr, score, k=3, alpha=1), X1)                        # the three used entries all weigh 0
    assert same_bits(run(nbr, score, k=4, alpha=1), X1 + 0.5 * TABLE[4])
    assert same_bits(run(nbr, score, k=3, alpha=0), X1 + TABLE[1] + TABLE[2] + TABLE[3])   # AQE: w = 1 whatever the score, NaN still out
    # subnormal score: alpha = 1 adds the (subnormal, exact) products to a zero row; alpha = 3 underflows the weight to 0: not added
    s = F32(2.0 ** -140)
    x0 = np.zeros((1, 4), F32)
    assert same_bits(run([[1]], [[s]], 1, 1, x=x0), [[2.0 ** -139, 2.0 ** -138, -2.0 ** -139, 2.0 ** -142]])
    got = run([[1, 2]], [[s, s]], 2, 3, x=x0)
    assert same_bits(got, x0) and not np.signbit(got).any()
    # 1 + 2^-23 by repeated fp32 products: every step rounds 1 + a e + (a - 1) e^2 to 1 + a e, so alpha = 3 gives 1 + 3 e (also what
    # a correctly rounded power gives) and alpha = 16 gives exactly 1 + 16 e = 1 + 2^-19
    e = 2.0 ** -23
    s = F32(1 + e)
    assert float(E.weight_ref(s, 1)) == 1 + e and float(E.weight_ref(s, 3)) == 1 + 3 * e and float(E.weight_ref(s, 16)) == 1 + 16 * e
    assert same_bits(run([[3]], [[s]], 1, 16), X1.astype(np.float64) + (1 + 16 * e) * TABLE[3].astype(np.float64))   # exact in fp32
    assert float(E.weight_ref(F32(0.5), 16)) == 2.0 ** -16 and float(E.weight_ref(F32(-3.0), 16)) == 0.0
    assert float(E.weight_ref(NAN, 0)) == 1.0


def test_no_eligible_entry_returns_x_and_k_stops_the_walk():
    assert same_bits(run([[-1, -1, 6]], [[.5, .5, .5]], 3, 1), X1)
    assert same_bits(run([[0]], [[NAN]], 1, 0), X1)
    assert same_bits(run([[0, 0]], [[.5, .5]], 2, 1, self_base=0), X1)
    got = run([[0, 1, 2, 3]], [[1, 1, 1, 1]], k=2, alpha=3)
    assert same_bits(got, X1 + TABLE[0] + TABLE[1])
    got = run([[4, 4]], [[1, .5]], k=2, alpha=1)                               # a repeated index is two entries
    assert same_bits(got, X1 + TABLE[4] + 0.5 * TABLE[4])


def test_order_of_the_sum_is_list_order():
    # 2^24 + 1 - 2^24 in fp32: (x + a) + b differs from (x + b) + a
    table = np.array([[2.0 ** 24], [-2.0 ** 24]], F32).repeat(4, 1)
    x = np.ones((1, 4), F32)
    a = E.expand_rows_ref(x, table, np.array([[0, 1]], np.int32), np.ones((1, 2), F32), 2, 0)
    b = E.expand_rows_ref(x, table, np.array([[1, 0]], np.int32), np.ones((1, 2), F32), 2, 0)
    assert a.tolist() == [[0.0] * 4] and b.tolist() == [[1.0] * 4]


# ---- the bound library, no GPU
def test_bound_library_refuses_bad_arguments_without_a_gpu(libs):
    # fake non-null, 16-byte aligned pointers: every call is refused on the host before anything is read or launched
    X, T, N, S, O = (1 << 20), (2 << 20), (3 << 20), (4 << 20), (5 << 20)
    for h in libs.values():
        def refused(x=X, ldx=16, table=T, ldt=16, M=100, nbr=N, score=S, ldn=11, kl=11, k=10, alpha=3, self_base=-1, normalize=1,
                    eps=1e-12, out=O, ldo=16, rows=8, D=16):
            assert h.reid_expand_rows(x, ldx, table, ldt, M, nbr, score, ldn, kl, k, alpha, self_base, normalize, eps, out, ldo, rows, D,
                                      None) == -1
            return h.reid_last_error()
        for name in ('x', 'table', 'nbr', 'score', 'out'):
            assert b'null pointer' in refused(**{name: None})
        assert b'k=12 outside 1..kl=11' in refused(k=12)
        assert b'k=0 outside' in refused(k=0)
        assert b'kl=65 outside 1..64' in refused(kl=65, ldn=65)
        assert b'kl=0 outside' in refused(kl=0)
        assert b'ldn=10 < kl=11' in refused(ldn=10)
        assert b'alpha=17 outside 0..16' in refused(alpha=17)
        assert b'alpha=-1 outside 0..16' in refused(alpha=-1)
        assert b'D=18 unsupported' in refused(D=18, ldx=20, ldt=20, ldo=20)
        assert b'D=1028 unsupported' in refused(D=1028, ldx=1028, ldt=1028, ldo=1028)
        assert b'D=0 unsupported' in refused(D=0)
        for name in ('ldx', 'ldt', 'ldo'):
            assert name.encode() + b'=12' in refused(**{name: 12})            # < D
            assert name.encode() + b'=18' in refused(**{name: 18})            # not a multiple of 4
        assert b'16-byte aligned' in refused(x=X + 4)
        assert b'16-byte aligned' in refused(table=T + 8)
        assert b'16-byte aligned' in refused(out=O + 4)
        assert b'out must not be table or x' in refused(out=T)
        assert b'out must not be table or x' in refused(out=X)
        assert b'rows=0' in refused(rows=0)
        assert b'M=0' in refused(M=0)
        assert b'self_base=-2' in refused(self_base=-2)
        assert b'normalize=2' in refused(normalize=2)
        assert b'eps=' in refused(eps=-1.0)
        assert b'eps=' in refused(eps=float('nan'))


# ---- Python layers
def test_expansion_params_validate_their_ranges():
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.expansion import ExpansionParams
    p = ExpansionParams()
    assert (p.k, p.alpha) == (10, 3)
    assert ExpansionParams(64, 16).k == 64 and ExpansionParams(1, 0).alpha == 0
    for bad in (dict(k=0), dict(k=65), dict(alpha=-1), dict(alpha=17), dict(alpha=2.5), dict(k=3.0)):
        with pytest.raises(_lib.ReidHipError, match='expansion'):
            ExpansionParams(**bad)
    with pytest.raises(Exception):
        p.k = 3                                                             # frozen


def test_python_layers_refuse_cpu_tensors():
    from prcv2025reid_amd import _lib, ops
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.expansion import ExpansionParams, augment_gallery, expand_queries
    Q, G = torch.randn(4, 8), torch.randn(30, 8)
    with pytest.raises(_lib.ReidHipError, match='device tensors'):
        augment_gallery(G, ExpansionParams(3, 1))
    with pytest.raises(_lib.ReidHipError, match='k=64 needs lists of k \\+ 1 entries'):
        augment_gallery(G, ExpansionParams(64, 1))
    with pytest.raises(_lib.ReidHipError, match='device tensors'):
        expand_queries(Q, None, ExpansionParams(3, 1))                      # refused before the index is touched
    with pytest.raises(_lib.ReidHipError, match='device tensors'):
        ProtocolEvaluator.per_query(object.__new__(ProtocolEvaluator), Q, torch.zeros(4), expand=ExpansionParams(3, 1))
    with pytest.raises(_lib.ReidHipError, match='CUDA'):
        ops.expand_rows(Q, G, torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3), 3, 1)
