"""CPU: the fp64 reference of the cross-modal batch-hard triplet loss (cross_triplet_ref.py) against a plain-loop implementation,
against finite differences and against torch autograd of the torch-op formulation; the fixtures the GPU test checks for index equality;
and the argument checks of reid_cross_triplet_* through the built library (no device)."""
import ctypes

import pytest
import torch

import cross_triplet_ref as R


def _small(seed=0, valid=False):
    """P = 2, N = 6, Mg = 5, D = 8.  With validity: g row 0 is invalid -- the only positive of q rows 0 and 1 -- and pair 1 keeps only
    q row 5, whose label no g row has: that pair has no positive at all."""
    gen = torch.Generator().manual_seed(seed)
    ql, gl = torch.tensor([0, 0, 1, 1, 2, 3]), torch.tensor([0, 1, 1, 2, 4])
    off = torch.randn(5, 8, generator=gen, dtype=torch.float64)
    q = 0.7 * off[ql][None] + torch.randn(2, 6, 8, generator=gen, dtype=torch.float64) + 2.0
    g = 0.7 * off[gl] + torch.randn(5, 8, generator=gen, dtype=torch.float64) + 2.0
    qv = gv = None
    if valid:
        qv = torch.tensor([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1]], dtype=torch.uint8)
        gv = torch.tensor([0, 1, 1, 1, 1], dtype=torch.uint8)
    return q, g, ql, gl, qv, gv


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
@pytest.mark.parametrize('with_valid', [False, True])
def test_reference_equals_plain_loops(margin, with_valid, normalize):
    q, g, ql, gl, qv, gv = _small(1, with_valid)
    ref = R.reference(q, g, ql, gl, qv, gv, margin, normalize)
    loop = R.loop_reference(q, g, ql, gl, qv, gv, margin, normalize)
    for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
        assert ref[k].tolist() == loop[k], k
    for k in ('q_d_ap', 'q_d_an', 'q_row_loss', 'g_d_ap', 'g_d_an', 'g_row_loss'):
        assert torch.allclose(ref[k], torch.tensor(loop[k], dtype=torch.float64), rtol=1e-13, atol=0), k
    assert ref['n_qg'] == loop['n_qg'] and ref['n_gq'] == loop['n_gq'] and ref['flag'] == loop['flag']
    assert all(abs(a - b) <= 1e-13 * (1 + abs(b)) for a, b in zip(ref['L'], loop['L']))
    if with_valid:
        assert ref['q_idx_p'][0].tolist()[:2] == [-1, -1] and ref['q_idx_n'][0].tolist()[:2] == [-1, -1]     # their only positive is invalid
        assert ref['n_qg'] == [3, 0] and ref['n_gq'] == [3, 0] and ref['flag'] == [1.0, 0.0] and ref['L'][1] == 0.0 and ref['L'][0] > 0
        assert bool((ref['q_idx_p'][1] == -1).all()) and bool((ref['g_idx_p'][1] == -1).all())
        assert 0 not in ref['q_idx_n'][0].tolist()                                                            # an invalid row is never chosen
    else:
        # q row 5 (label 3) and g row 4 (label 4) have no positive; there is no self-exclusion (q row 0's positive is g row 0)
        assert ref['n_qg'] == [5, 5] and ref['n_gq'] == [4, 4] and ref['q_idx_p'][0].tolist()[0] == 0


def test_reference_ties_go_to_the_lowest_index_in_both_directions():
    q, g, ql, gl, _, _ = _small(2)
    g[1] = q[0, 2] + 100.0; g[2] = g[1]                   # g rows 1 and 2 (label 1) equal and far away: tied hardest positives of q rows 2, 3
    q[0, 1] = q[0, 0]                                     # q rows 0 and 1 (label 0) equal: tied hardest positives of g row 0
    ref = R.reference(q, g, ql, gl, None, None, 0.3, False)
    loop = R.loop_reference(q, g, ql, gl, None, None, 0.3, False)
    assert ref['q_idx_p'][0].tolist()[2:4] == [1, 1] and float(ref['q_gap_p'][0][2]) == 0.0
    assert int(ref['g_idx_p'][0][0]) == 0 and float(ref['g_gap_p'][0][0]) == 0.0
    for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
        assert ref[k].tolist() == loop[k], k
    # tied hardest NEGATIVES: q rows 0 and 1 of pair 0 sit next to g row 3 (label 2); g rows 1 and 2 next to q row 4 (label 2) of pair 1
    q[0, 0] = g[3] + 0.001; q[0, 1] = q[0, 0]
    g[1] = q[1, 4] + 0.001; g[2] = g[1]
    ref = R.reference(q, g, ql, gl, None, None, 0.3, False)
    loop = R.loop_reference(q, g, ql, gl, None, None, 0.3, False)
    assert int(ref['g_idx_n'][0][3]) == 0 and float(ref['g_gap_n'][0][3]) == 0.0
    assert int(ref['q_idx_n'][1][4]) == 1 and float(ref['q_gap_n'][1][4]) == 0.0
    for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
        assert ref[k].tolist() == loop[k], k


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
def test_reference_gradient_equals_finite_differences_and_autograd(margin, normalize):
    q, g, ql, gl, qv, gv = _small(3, valid=False)
    qv = torch.tensor([[1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 1]], dtype=torch.uint8)
    gv = torch.tensor([1, 1, 1, 1, 1], dtype=torch.uint8)
    gs = [1.7, -0.6]
    ref = R.reference(q, g, ql, gl, qv, gv, margin, normalize)
    assert min(ref['n_qg']) >= 4 and min(ref['n_gq']) >= 3 and float(ref['q_row_loss'].max()) > 0
    gaps = torch.cat([ref[k].flatten() for k in ('q_gap_p', 'q_gap_n', 'g_gap_p', 'g_gap_n')])
    assert float(gaps.min()) > 1e-4                                                       # the selection is stable under the probe
    if margin is not None:
        for s in 'qg':
            z = (ref[f'{s}_d_ap'] - ref[f'{s}_d_an'] + margin)[ref[f'{s}_idx_p'] >= 0]
            assert float(z.abs().min()) > 1e-4                                            # away from the hinge's kink
    dq, dg = R.gradient(q, g, margin, normalize, ref, gs)
    f = lambda qq, gg: sum(w * L for w, L in zip(gs, R.evaluate(qq, gg, ref, margin, normalize)['L']))
    h, worst = 1e-6, 0.0
    for x, dx, other, first in ((q, dq, g, True), (g, dg, q, False)):
        flat, dflat = x.reshape(-1), dx.reshape(-1)
        for e in range(flat.numel()):
            xp, xm = flat.clone(), flat.clone()
            xp[e] += h; xm[e] -= h
            a, b = xp.reshape(x.shape), xm.reshape(x.shape)
            fd = (f(a, other) - f(b, other)) / (2 * h) if first else (f(other, a) - f(other, b)) / (2 * h)
            worst = max(worst, abs(fd - float(dflat[e])))
    assert worst <= 1e-8, worst
    assert float(dq[0, 3].abs().max()) == 0.0 and float(dq.abs().max()) > 0 and float(dg.abs().max()) > 0     # the invalid row gets nothing
    qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    L = R.torch_loss(qa, ga, ql, gl, qv, gv, margin, normalize)
    assert all(abs(float(a) - b) <= 1e-13 * (1 + abs(b)) for a, b in zip(L.detach(), ref['L']))
    (L * torch.tensor(gs, dtype=torch.float64)).sum().backward()
    assert float((qa.grad - dq).abs().max()) <= 1e-12 and float((ga.grad - dg).abs().max()) <= 1e-12


def test_reference_gradient_below_eps_is_g_over_eps():
    # (a zero row is at distance 1 from every unit row: its own z = d_ap - d_an is 0 up to rounding, where the soft margin's torch
    # formulation has a kink of its own and mining is ill-conditioned -- hence the hinge, and autograd at the reference's selection)
    q, g, ql, gl, _, _ = _small(4)
    q[1, 2] = 0.0                                          # |x| < eps: x / max(|x|, eps) is linear there
    ref = R.reference(q, g, ql, gl, None, None, 0.3, True)
    assert int(ref['q_idx_p'][1][2]) >= 0 and 2 in ref['g_idx_p'][1].tolist()          # an anchor, and some g anchor's choice
    dq, _ = R.gradient(q, g, 0.3, True, ref)
    assert float(dq[1, 2].abs().max()) > 1e9 and bool(torch.isfinite(dq).all())
    qa = q.clone().requires_grad_(True)
    R.torch_loss_at(qa, g, ref, 0.3, True).sum().backward()
    assert float((qa.grad - dq).abs().max()) <= 1e-12 * float(dq[1, 2].abs().max())


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('shape,ratio', R.EXACT_INDEX)
def test_fixtures_checked_for_index_equality_have_clear_gaps(shape, ratio, normalize):
    """What makes the GPU test's index-equality check legitimate: on these fixtures every anchor's fp64 gap between the best and the
    runner-up distance exceeds 10 x the bound on a kernel distance."""
    q, g, ql, gl = R.fixture(shape, ratio)
    ref = R.reference(q, g, ql, gl, None, None, 0.3, normalize)
    assert (sum(ref['n_qg']) > 0 and sum(ref['n_gq']) > 0) == (shape[1] > 1)
    for s, kind, mask in R.small_gaps(ref, shape[3], normalize, 10.0):
        assert not bool(mask.any()), (s, kind, torch.nonzero(mask).tolist())


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
        return h.reid_cross_triplet_fwd(q, ldq, g, ldg, p, p, None, None, P, N, Mg, D, margin, normalize, eps, out, p, p, p, ws, p, None)

    def bwd(q=p, ldq=8, g=p, ldg=8, P=2, N=4, Mg=4, D=8, margin=0.3, normalize=1, eps=1e-12, out=p, ws=p, dq=p, lddq=8, dg=p, lddg=8):
        return h.reid_cross_triplet_bwd(q, ldq, g, ldg, None, None, P, N, Mg, D, margin, normalize, eps, out, p, p, p, ws, p, p, dq, lddq,
                                        dg, lddg, None)

    def refused(rc, *words):
        msg = h.reid_last_error()
        return rc == -1 and all(w in msg for w in words)

    for call, name in ((fwd, b'reid_cross_triplet_fwd'), (bwd, b'reid_cross_triplet_bwd')):
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
    ws = h.reid_cross_triplet_ws_floats
    assert ws(4, 64, 64, 512) >= (4 * 64 + 64) * 512 + (4 * 64 + 64) + 4 * 64 + 4 * 64
    for args, word in (((0, 4, 4, 8), b'P=0'), ((9, 4, 4, 8), b'P=9'), ((1, 0, 4, 8), b'N=0'), ((1, 4, 8193, 8), b'Mg=8193'), ((1, 4, 4, 6), b'D=6'),
                       ((1, 4, 4, 1028), b'D=1028')):
        assert refused(ws(*args), b'reid_cross_triplet_ws_floats', word)


def test_config_and_head_expose_the_loss():
    from prcv2025reid_amd import _lib, losses
    from prcv2025reid_amd.config import TrainingConfig
    cfg = TrainingConfig()
    assert cfg.cross_triplet_weight == 0.0 and cfg.cross_triplet_margin == 0.3 and cfg.cross_triplet_normalize is True
    z = torch.zeros(4, 8)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.cross_modal_triplet(z, z, torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
