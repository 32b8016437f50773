"""CPU: the fp64 reference of the hetero-center triplet loss (hc_triplet_ref.py) against a plain-loop implementation, the clearing of
the fixtures the GPU test checks for index equality, the config defaults, and the argument checks of reid_hc_triplet_* through the
built library (no device)."""
import ctypes

import pytest
import torch

import hc_triplet_ref as R


def _small(seed, P=2, N=11, Mg=9, D=8, ratio=3.0):
    """Interleaved, unsorted labels with uneven counts, an identity on one side only, and some invalid rows."""
    q, g, _, _ = R.make_case(P, N, Mg, D, ratio, seed)
    ql = torch.tensor([7, 2, 7, 5, 2, 2, 9, 7, 5, 2, 7])
    gl = torch.tensor([5, 7, 2, 4, 7, 5, 2, 5, 5])
    qv = torch.ones(P, N, dtype=torch.uint8); qv[0, 0] = 0; qv[1, 6] = 0       # pair 0: the first row of identity 7; pair 1: all of 9
    gv = torch.ones(Mg, dtype=torch.uint8); gv[3] = 0                           # all of identity 4
    return q, g, ql, gl, qv, gv


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
@pytest.mark.parametrize('valid', [False, True])
def test_reference_equals_the_plain_loops(valid, margin, normalize):
    q, g, ql, gl, qv, gv = _small(1)
    if not valid:
        qv = gv = None
    a = R.reference(q, g, ql, gl, qv, gv, margin, normalize)
    b = R.loop_reference(q, g, ql, gl, qv, gv, margin, normalize)
    for k in ('q_lead', 'q_count', 'q_label', 'g_lead', 'g_count', 'g_label', 'idx_p', 'idx_n'):
        assert a[k].tolist() == b[k], k
    for k in ('d_ap', 'd_an', 'loss'):
        assert torch.allclose(a[k], torch.tensor(b[k], dtype=torch.float64), rtol=1e-13, atol=1e-15), k
    assert a['n_q'] == b['n_q'] and a['n_g'] == b['n_g'] and a['flag'] == b['flag'] == [1.0, 1.0]
    assert all(abs(x - y) <= 1e-13 * (1 + abs(y)) for x, y in zip(a['L'], b['L']))
    if valid:
        # pair 0: identity 7's leader is row 2 (row 0 is invalid): slots 2, 7, 5, 9 in leader order 1, 2, 3, 6
        assert a['q_lead'][0].tolist() == [-1, 0, 1, 2, 0, 0, 3, 1, 2, 0, 1] and a['q_count'][0].tolist()[:5] == [4, 3, 2, 1, 0]
        assert a['q_label'][0].tolist()[:4] == [2, 7, 5, 9] and a['S_q'] == [4, 3] and a['S_g'] == 3
        assert a['g_lead'].tolist() == [0, 1, 2, -1, 1, 0, 2, 0, 0] and a['g_count'].tolist()[:4] == [4, 2, 2, 0]
        # identity 9 exists on the q side of pair 0 only: an anchor without a positive
        assert int(a['idx_p'][0, 3]) == -1 and float(a['d_ap'][0, 3]) == 0.0 and a['n_q'] == [3, 3] and a['n_g'] == [3, 3]


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
def test_reference_gradient_is_that_of_the_whole_tensor_formulation(margin, normalize):
    """The autograd gradient at the reference's selection against the independent one-hot / masked-min formulation (all rows valid)."""
    q, g, ql, gl, _, _ = _small(2)
    ref = R.reference(q, g, ql, gl, None, None, margin, normalize)
    gs = [0.75, -0.5]
    dq, dg = R.gradient(q, g, margin, normalize, ref, ql, gl, None, None, gs)
    qa, ga = q.double().requires_grad_(True), g.double().requires_grad_(True)
    L = R.torch_loss(qa, ga, ql, gl, margin, normalize)
    assert all(abs(float(a) - b) <= 1e-13 * (1 + abs(b)) for a, b in zip(L.detach(), ref['L']))
    (L * torch.tensor(gs, dtype=torch.float64)).sum().backward()
    assert float(dq.abs().max()) > 0 and float(dg.abs().max()) > 0
    assert float((qa.grad - dq).abs().max()) <= 1e-12 and float((ga.grad - dg).abs().max()) <= 1e-12


def test_reference_gradient_below_eps_is_g_over_eps():
    q, g, ql, gl, _, _ = _small(3)
    q[1, 3] = 0.0                                          # |x| < eps: x / max(|x|, eps) is linear there
    ref = R.reference(q, g, ql, gl, None, None, 0.3, True)
    assert int(ref['idx_p'][1, int(ref['q_lead'][1, 3])]) >= 0
    dq, _ = R.gradient(q, g, 0.3, True, ref, ql, gl)
    assert float(dq[1, 3].abs().max()) > 1e9 and bool(torch.isfinite(dq).all())


def test_single_identity_and_empty_sides_give_nothing():
    q, g, ql, gl, _, _ = _small(4)
    one = R.reference(q, g, torch.zeros_like(ql), torch.zeros_like(gl), None, None, 0.3, True)
    assert one['L'] == [0.0, 0.0] and one['flag'] == [0.0, 0.0] and bool((one['idx_p'] == -1).all()) and one['S_q'] == [1, 1]
    dq, dg = R.gradient(q, g, 0.3, True, one, torch.zeros_like(ql), torch.zeros_like(gl))
    assert float(dq.abs().max()) == 0.0 == float(dg.abs().max())
    none = R.reference(q, g, ql, gl, None, torch.zeros(g.shape[0], dtype=torch.uint8), 0.3, True)
    assert none['flag'] == [0.0, 0.0] and none['S_g'] == 0 and bool((none['g_lead'] == -1).all())


@pytest.mark.parametrize('shape,ratio', R.EXACT_INDEX)
def test_fixtures_checked_for_index_equality_are_cleared(shape, ratio):
    """What makes the GPU test's index-equality check legitimate: on these fixtures, with unit rows and without, every anchor's fp64
    gap between the nearest and the second-nearest negative exceeds twice the bound on a kernel distance."""
    assert R.EXACT_INDEX == [(s, 0.0) for s in R.SHAPES[:4]]
    q, g, ql, gl = R.fixture(shape, ratio)
    ok, worst = R.cleared(q, g, ql, gl, factor=2.0)
    print(f'  {shape}: smallest gap / bound = {worst:.3g}')
    assert ok, (shape, worst)
    ref = R.reference(q, g, ql, gl, None, None, 0.3, True)
    assert sum(ref['n_q']) > 0 and sum(ref['n_g']) > 0


@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    return {f: _lib.bind(ctypes.CDLL(p)) for f, p in _lib.LIB_PATHS.items()}


@pytest.mark.parametrize('flavor', ['bf16', 'f16'])
def test_entry_points_check_their_arguments_without_a_device(libs, flavor):
    h = libs[flavor]
    buf = (ctypes.c_float * 64)()                         # host memory: only its (16-byte aligned) address is looked at before the refusal
    p = ctypes.addressof(buf)
    p += (-p) % 16
    nan = float('nan')

    def fwd(q=p, ldq=8, g=p, ldg=8, P=2, N=4, Mg=4, D=8, margin=0.3, normalize=1, eps=1e-12, out=p, ws=p):
        return h.reid_hc_triplet_fwd(q, ldq, g, ldg, p, p, None, None, P, N, Mg, D, margin, normalize, eps, out, p, p, p, p, ws, p, None)

    def bwd(q=p, ldq=8, g=p, ldg=8, P=2, N=4, Mg=4, D=8, margin=0.3, normalize=1, eps=1e-12, out=p, ws=p, dq=p, lddq=8, dg=p, lddg=8):
        return h.reid_hc_triplet_bwd(q, ldq, g, ldg, P, N, Mg, D, margin, normalize, eps, out, p, ws, p, p, dq, lddq, dg, lddg, None)

    def refused(rc, *words):
        msg = h.reid_last_error()
        return rc == -1 and all(w in msg for w in words)

    for call, name in ((fwd, b'reid_hc_triplet_fwd'), (bwd, b'reid_hc_triplet_bwd')):
        assert refused(call(q=None), name, b'null pointer') and refused(call(out=None), name, b'null pointer')
        for P in (0, 9):
            assert refused(call(P=P), name, b'P=%d' % P)
        for n in (0, 8193):
            assert refused(call(N=n), name, b'N=%d' % n) and refused(call(Mg=n), name, b'Mg=%d' % n)
        for D in (0, 6, 1028):
            assert refused(call(D=D, ldq=1028, ldg=1028), name, b'D=%d' % D)
        assert refused(call(ldq=4), name, b'ldq=4') and refused(call(ldq=10), name, b'ldq=10')         # < D; not a multiple of 4
        assert refused(call(ldg=4), name, b'ldg=4') and refused(call(ldg=10), name, b'ldg=10')
        assert refused(call(q=p + 4), name, b'16-byte aligned') and refused(call(g=p + 8), name, b'16-byte aligned')
        assert refused(call(ws=p + 4), name, b'16-byte aligned')
        assert refused(call(P=8, N=8192, ldq=1 << 15), name, b'ldq', b'2^31') and refused(call(Mg=8192, ldg=1 << 18), name, b'ldg', b'2^31')
        assert refused(call(margin=nan), name, b'margin', b'NaN') and refused(call(eps=-1.0), name, b'eps=')
        assert refused(call(normalize=2), name, b'normalize=2')
    assert refused(bwd(dq=None), b'null pointer') and refused(bwd(dg=None), b'null pointer')
    assert refused(bwd(lddq=4), b'lddq=4') and refused(bwd(lddg=10), b'lddg=10')
    assert refused(bwd(dq=p + 8), b'16-byte aligned') and refused(bwd(dg=p + 4), b'16-byte aligned')
    assert refused(bwd(P=8, N=8192, lddq=1 << 15), b'lddq', b'2^31')
    ws = h.reid_hc_triplet_ws_floats
    P, N, Mg, D = 4, 64, 64, 512
    R_, U_ = P * N + Mg, N + Mg                            # unit rows, centres, centre gradients; labels, distances, indices, losses
    assert ws(P, N, Mg, D) >= 2 * R_ * D + P * U_ * D + 7 * P * U_ + 3 * R_ + P + 1 and ws(P, N, Mg, D) % 4 == 0
    for args, word in (((0, 4, 4, 8), b'P=0'), ((9, 4, 4, 8), b'P=9'), ((1, 0, 4, 8), b'N=0'), ((1, 4, 8193, 8), b'Mg=8193'), ((1, 4, 4, 6), b'D=6'),
                       ((1, 4, 4, 1028), b'D=1028')):
        assert refused(ws(*args), b'reid_hc_triplet_ws_floats', word)


def test_config_and_head_expose_the_loss():
    from prcv2025reid_amd import _lib, losses
    from prcv2025reid_amd.config import TrainingConfig
    cfg = TrainingConfig()
    assert cfg.hc_triplet_weight == 0.0 and cfg.hc_triplet_margin == 0.3 and cfg.hc_triplet_normalize is True
    z = torch.zeros(4, 8)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.hetero_center_triplet(z, z, torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
