"""GPU: the cross-modal Smooth-AP loss (csrc/smooth_ap.hip) against the fp64 reference of smooth_ap_ref.py within its derived bounds, in
both library flavours (the kernels are fp32: the same bits in both), in the batch and over a ring, and the loss behind the public calls,
inside the model and in the graphed step.

Every output and the ring live between 32 guard elements that hold a sentinel pattern and must keep it; padded input rows carry NaN in
their padding, padded output rows the sentinel.  Invalid rows hold NaN."""
import types

import numpy as np
import pytest
import torch

import smooth_ap_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 32
U = R.U
_CASE = {}                               # case key -> inputs on the CPU with their fp64 reference (shared by the flavours and the tests)


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


def guarded(n, dtype=torch.float32):
    """([GUARD + n + GUARD] sentinel buffer of int32, its middle n elements viewed as ``dtype``)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL32, dtype=torch.int32, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(dtype)


def untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL32).all()) and bool((buf[GUARD + n:] == SENTINEL32).all())


def strided(x, pad):
    """The rows of x [..., D] as a [rows, D] view of a [rows, D + pad] buffer whose padding columns are NaN."""
    x2 = x.reshape(-1, x.shape[-1])
    if pad == 0:
        return x2.contiguous()
    buf = torch.full((x2.shape[0], x2.shape[1] + pad), float('nan'), device=x.device)
    buf[:, :x2.shape[1]] = x2
    return buf[:, :x2.shape[1]]


def grad_rows(rows, D, pad):
    """(raw int32 buffer, [rows, D] fp32 view) between guard rows and sentinel padding columns."""
    raw = torch.full((rows + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda')
    return raw, raw.view(torch.float32)[GUARD:GUARD + rows, :D]


def grad_rows_intact(raw, rows, D, name):
    assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + rows:] == SENTINEL32).all()), f'{name}: guard rows overwritten'
    assert bool((raw[GUARD:GUARD + rows, D:] == SENTINEL32).all()), f'{name}: padding columns overwritten'
    assert not bool((raw[GUARD:GUARD + rows, :D] == SENTINEL32).any()), f'{name}: elements not written'


def bits(t):
    t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t
    return t.detach().cpu().contiguous().view(torch.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def labelled_case(P, N, Mg, D, pos, seed, invalid=0.0):
    """Random directions with a planned number of positives per q anchor: ``pos`` 1: every gallery row its own identity; 2: identities in
    pairs; 'G-1': one gallery row of another identity.  Invalid rows (a share ``invalid``) hold NaN."""
    r = np.random.default_rng(seed)
    q = (r.standard_normal((P, N, D)) * r.uniform(0.5, 2.0, (P, N, 1))).astype(np.float32)
    g = (r.standard_normal((Mg, D)) * r.uniform(0.5, 2.0, (Mg, 1))).astype(np.float32)
    if pos == 'G-1':
        gl = np.zeros(Mg, np.int64); gl[int(r.integers(0, Mg))] = 1
        ql = np.zeros(N, np.int64)
    else:
        gl = (np.arange(Mg) // pos).astype(np.int64)
        ql = r.choice(gl, N).astype(np.int64) if Mg > 1 else (np.arange(N) % 2).astype(np.int64)      # (one gallery row: a negative for g->q)
    qv = gv = None
    if invalid > 0:
        qv, gv = (r.random((P, N)) >= invalid).astype(np.uint8), (r.random(Mg) >= invalid).astype(np.uint8)
        q[qv == 0] = np.nan; g[gv == 0] = np.nan
    return q, g, ql, gl, qv, gv


class DeviceRing:
    """The tensors of a CrossBatchMemory, each between guards."""

    def __init__(self, M, sides, D):
        self.M, self.sides, self.D = M, sides, D
        self.b_rows, rows = guarded(sides * M * D); self.rows = rows.view(sides, M, D); self.rows.zero_()
        self.b_labels, lab = guarded(2 * M, torch.int32); self.labels = lab.view(torch.int64); self.labels.zero_()
        self.b_valid, val = guarded((sides * M + 3) // 4, torch.int32); self.valid = val.view(torch.uint8)[:sides * M].view(sides, M); self.valid.zero_()
        self.b_cursor, self.cursor = guarded(2, torch.int32); self.cursor.zero_()

    def mem(self):
        return (self.rows, self.labels, self.valid)

    def fill(self, rows, labels, valid):
        self.rows.copy_(dev(rows)); self.labels.copy_(dev(labels)); self.valid.copy_(dev(valid))

    def intact(self):
        return untouched(self.b_rows, self.rows.numel()) and untouched(self.b_labels, 2 * self.M) and \
            untouched(self.b_valid, (self.sides * self.M + 3) // 4) and untouched(self.b_cursor, 2)

    def host(self):
        return self.rows.cpu().numpy().copy(), self.labels.cpu().numpy().copy(), self.valid.cpu().numpy().copy()


def run(ops, q, g, ql, gl, qv, gv, tau, normalize=True, ring=None, with_grad=True, gscale=None, pad=4, enqueue=False):
    """Forward (and backward) of q [P, N, D], g [Mg, D] (numpy) through ops.*; every output between guards."""
    P, N, D = q.shape
    Mg = g.shape[0]
    o = dict(P=P, N=N, Mg=Mg, D=D, q2=strided(dev(q), pad), g2=strided(dev(g), pad), ql=dev(ql), gl=dev(gl),
             qv=None if qv is None else dev(qv).reshape(-1).contiguous(), gv=dev(gv))
    mem = None if ring is None else ring.mem()
    if enqueue:
        ops.xbm_enqueue(o['q2'], o['g2'], o['ql'], o['qv'], o['gv'], normalize, R.EPS, *mem, ring.cursor, P=P)
    G = (Mg, N) if ring is None else (ring.M, ring.M)
    o['b_ws'], o['ws'] = guarded(ops.smooth_ap_ws_floats(P, N, Mg, D, *G, with_grad))
    o['b_q_ap'], o['q_ap'] = guarded(P * N); o['b_g_ap'], o['g_ap'] = guarded(P * Mg)
    o['b_q_npos'], o['q_npos'] = guarded(P * N, torch.int32); o['b_g_npos'], o['g_npos'] = guarded(P * Mg, torch.int32)
    o['b_result'], o['result'] = guarded(4 * P)
    ops.smooth_ap_fwd(o['q2'], o['g2'], o['ql'], o['gl'], o['qv'], o['gv'], tau, normalize, R.EPS, with_grad, o['q_ap'], o['q_npos'], o['g_ap'],
                      o['g_npos'], o['ws'], o['result'], P=P, ring=mem)
    torch.cuda.synchronize()
    for k in ('ws', 'q_ap', 'g_ap', 'q_npos', 'g_npos', 'result'):
        assert untouched(o['b_' + k], o[k].numel()), f'{k}: guard elements overwritten'
        if k != 'ws':                    # (ws holds pieces only some anchors or only the gradient pass write)
            assert not bool((o[k].view(torch.int32) == SENTINEL32).any()), f'{k}: elements not written'
    assert ring is None or ring.intact()
    if with_grad:
        gs = np.ones(P, np.float32) if gscale is None else np.asarray(gscale, np.float32)
        raw_q, o['dq'] = grad_rows(P * N, D, pad); raw_g, o['dg'] = grad_rows(Mg, D, pad)
        ops.smooth_ap_bwd(o['qv'], o['gv'], o['ws'], dev(gs), o['dq'], o['dg'], P=P)
        torch.cuda.synchronize()
        grad_rows_intact(raw_q, P * N, D, 'dq'); grad_rows_intact(raw_g, Mg, D, 'dg')
        assert untouched(o['b_ws'], o['ws'].numel())
    return o


def check(o, f, need_margin=False):
    """The outputs of ``run`` against the reference dict ``f`` within its bounds; prints the measured maxima beside the bounds."""
    P, N, Mg, D = o['P'], o['N'], o['Mg'], o['D']
    res = o['result'].cpu().numpy().reshape(P, 4).astype(np.float64)
    assert np.array_equal(res[:, 1], f['flag']) and np.array_equal(res[:, 2:], f['n_active'])
    e_loss = np.abs(res[:, 0] - f['loss'])
    worst = {}
    for side, n in (('q', N), ('g', Mg)):
        ap = o[side + '_ap'].cpu().numpy().reshape(P, n).astype(np.float64)
        assert np.array_equal(o[side + '_npos'].cpu().numpy().reshape(P, n), f[side + '_npos']), side
        act = f[side + '_ap'] >= 0
        assert np.array_equal(ap >= 0, act) and (ap[~act] == -1).all(), side
        err, bound = np.abs(ap - f[side + '_ap'])[act], f['e_' + side + '_ap'][act]
        if act.any():
            worst[side + '_ap'] = (err.max(), bound[err.argmax()], (err / bound).max())
        assert (err <= bound).all(), (side, float((err / bound).max()))
        if need_margin and act.any():
            assert ((1 - f[side + '_ap'][act]) >= 20 * bound).all(), (side, float(((1 - f[side + '_ap'][act]) / bound).min()))
    assert (e_loss <= f['e_loss']).all(), (e_loss, f['e_loss'])
    assert (res[f['flag'] == 0, 0] == 0).all()
    worst['loss'] = (e_loss.max(), f['e_loss'][e_loss.argmax()], (e_loss / np.maximum(f['e_loss'], 1e-300)).max())
    if 'dq' in o:
        for name, got, want, bound in (('dq', o['dq'].cpu().numpy().reshape(P, N, D), f['dq'], f['e_dq']), ('dg', o['dg'].cpu().numpy(), f['dg'], f['e_dg'])):
            assert np.isfinite(got).all(), name
            err = np.abs(got.astype(np.float64) - want)
            ok = err <= bound
            worst[name] = (err.max(), bound.flat[err.argmax()], (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
            assert ok.all(), (name, float((err[~ok] / bound[~ok]).max()) if (bound[~ok] > 0).all() else 'non-zero where the reference is exactly 0')
            if need_margin:
                assert np.abs(want).max() >= 20 * bound.max(), (name, np.abs(want).max() / bound.max())
    print(' '.join(f'{k}: err {v[0]:.3e} bound {v[1]:.3e} worst ratio {v[2]:.3f};' for k, v in worst.items()))
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. the batch form
# (P, N, Mg, D, positives per q anchor, share of invalid rows): the gallery of q->g has Mg rows, that of g->q N rows -- 1, 2, 63, 64, 65
# and 257 rows each appear; N = 1, 3, 64, 65; D = 32, 96, 512; P = 1, 3; 1, 2 and G - 1 positives
BATCH_CASES = [(1, 1, 257, 32, 1, 0.0), (3, 3, 2, 512, 1, 0.0), (1, 64, 63, 32, 2, 0.0), (1, 65, 64, 96, 1, 0.1), (3, 64, 65, 512, 2, 0.1),
               (1, 3, 257, 32, 'G-1', 0.0), (1, 65, 257, 96, 2, 0.0), (1, 2, 1, 32, 1, 0.0), (1, 3, 64, 512, 'G-1', 0.0)]


def margins_hold(f):
    """True when the REFERENCE's 1 - AP of every active anchor and its largest |dq| and |dg| stand at least 20 bounds above the bound."""
    for side in ('q', 'g'):
        act = f[side + '_ap'] >= 0
        if not ((1 - f[side + '_ap'][act]) >= 20 * f['e_' + side + '_ap'][act]).all():
            return False
    return all(np.abs(f[n]).max() >= 20 * f['e_' + n].max() for n in ('dq', 'dg'))


def batch_case(shape, tau=0.01, normalize=True, margin=False):
    """(inputs, gscale, reference) of a shape.  ``margin``: the inputs are the first seed from the shape's base on whose REFERENCE passes
    margins_hold -- a gallery of two rows whose positive leads by 10 tau has 1 - AP = e^-10 and a gradient to match, which no bound can
    stand 20 times below; the choice looks at the fp64 reference alone, never at the code under test."""
    key = ('batch', shape, tau, normalize, margin)
    if key not in _CASE:
        P, N, Mg, D, pos, invalid = shape
        gs = np.linspace(0.5, 1.5, P).astype(np.float32) * np.where(np.arange(P) % 2, -1, 1)
        for seed in range(100 + N + Mg, 164 + N + Mg):
            c = labelled_case(P, N, Mg, D, pos, seed, invalid)
            f = R.forward(*c, tau, normalize, gscale=gs)
            both = N == 1 or Mg == 1 or pos == 'G-1' or f['n_active'].min() > 0       # both directions active where the shape allows it
            if not margin or (f['flag'].sum() > 0 and both and margins_hold(f)):
                break
        else:
            raise AssertionError(f'no seed of {shape} gives the reference its margins')
        _CASE[key] = (c, gs, f)
    return _CASE[key]


@pytest.mark.parametrize('shape', BATCH_CASES, ids=lambda s: 'P{}-N{}-Mg{}-D{}-pos{}-inv{}'.format(*s))
def test_batch_form_against_the_reference(ops, shape):
    """Random directions at tau = 0.01.  1 - AP of every active anchor and the largest |dq|, |dg| stand at least 20 bounds above the bound
    (where a side has a gradient at all), so a kernel that returned a constant would fail."""
    c, gs, f = batch_case(shape, margin=True)
    o = run(ops, *c, 0.01, gscale=gs)
    check(o, f, need_margin=True)
    assert float(o['dq'].abs().max()) > 0 and float(o['dg'].abs().max()) > 0
    if c[4] is not None:                                         # invalid rows (NaN data): exactly zero gradients
        assert not bool(o['dq'][dev(c[4]).reshape(-1) == 0].any()) and not bool(o['dg'][dev(c[5]) == 0].any())


def test_without_gradients_the_gradient_part_is_skipped(ops):
    c, gs, f = batch_case(BATCH_CASES[3])
    o = run(ops, *c, 0.01, with_grad=False)
    check(o, f)
    full = run(ops, *c, 0.01, gscale=gs)
    for k in ('q_ap', 'g_ap', 'q_npos', 'g_npos', 'result'):
        assert torch.equal(bits(o[k]), bits(full[k])), k
    assert o['ws'].numel() < full['ws'].numel()


@pytest.mark.parametrize('tau', [0.001, 0.1])
def test_temperatures_stay_finite_and_inside_the_bounds(ops, tau):
    shape = BATCH_CASES[4]
    c, gs, f = batch_case(shape, tau)
    o = run(ops, *c, tau, gscale=gs)
    for k in ('q_ap', 'g_ap', 'result', 'dq', 'dg'):
        assert bool(torch.isfinite(o[k]).all()), k
    check(o, f)


def test_rows_used_as_they_are(ops):
    shape = (1, 3, 64, 32, 2, 0.0)
    c, gs, f = batch_case(shape, 0.1, False)
    check(run(ops, *c, 0.1, normalize=False, gscale=gs), f)


def test_zero_rows_hit_the_clamp(ops):
    """A zero q row and a zero g row: x^ = 0, every score of theirs 0; the gradient goes through G / eps and stays finite."""
    P, N, Mg, D = 1, 5, 7, 32
    q, g, ql, gl, _, _ = labelled_case(P, N, Mg, D, 2, 3)
    q[0, 2] = 0.0; g[4] = 0.0
    f = R.forward(q, g, ql, gl, tau=0.05)
    o = run(ops, q, g, ql, gl, None, None, 0.05)
    check(o, f)
    assert bool(torch.isfinite(o['dq']).all()) and float(o['dq'][2].abs().max()) > 1e6 and float(o['dg'][4].abs().max()) > 1e6


def test_a_pair_without_an_active_anchor(ops):
    """Pair 1 holds only invalid q rows: no anchor and no gallery in either direction -> flag 0, loss 0, zero gradients from it."""
    P, N, Mg, D = 2, 4, 6, 32
    q, g, ql, gl, _, _ = labelled_case(P, N, Mg, D, 2, 5)
    qv = np.ones((P, N), np.uint8); qv[1] = 0
    q[1] = np.nan
    f = R.forward(q, g, ql, gl, qv, None, tau=0.05, gscale=[1.0, 3.0])
    assert f['flag'].tolist() == [1.0, 0.0] and f['loss'][1] == 0
    o = run(ops, q, g, ql, gl, qv, None, 0.05, gscale=[1.0, 3.0])
    check(o, f)
    assert float(o['result'][4]) == 0.0 and float(o['result'][5]) == 0.0 and not bool(o['dq'][N:].any())
    # every anchor sees positives only: nothing is active anywhere
    z = np.zeros
    o = run(ops, q, g, z(N, np.int64), z(Mg, np.int64), qv, None, 0.05)
    assert not bool(o['result'].any()) and not bool(o['dq'].any()) and not bool(o['dg'].any()) and bool((o['q_ap'] == -1).all())


def test_two_runs_give_the_same_bits(ops):
    c, gs, f = batch_case(BATCH_CASES[4])
    a, b = run(ops, *c, 0.01, gscale=gs), run(ops, *c, 0.01, gscale=gs, pad=0)
    for k in ('q_ap', 'g_ap', 'q_npos', 'g_npos', 'result', 'dq', 'dg'):
        assert torch.equal(bits(a[k]), bits(b[k])), k


# ---------------------------------------------------------------------------------------------------------------- 2. the ring form
def ring_reference(ring, q, g, labels, qv, gv, tau, gscale=None):
    return R.forward(q, g, labels, labels, qv, gv, tau, ring=ring.host(), gscale=gscale)


def test_ring_form_three_enqueues_against_the_reference(ops):
    """Capacity 96, batches of 40: partly filled after one and two enqueues, the third wraps.  The device ring is checked against the fp64
    ring (rows within the unit-row bound, labels, validity and cursor exactly); the loss then ranks the rows the device holds."""
    P, N, D, M, tau = 3, 40, 96, 96, 0.01
    ring, ref = DeviceRing(M, P + 1, D), R.Ring(M, P + 1, D)
    for step in range(3):
        q, g, labels, _, qv, gv = labelled_case(P, N, N, D, 2, 50 + step, invalid=0.1)
        gs = [1.0, -2.0, 0.5]
        o = run(ops, q, g, labels, labels, qv, gv, tau, ring=ring, gscale=gs, enqueue=True)
        ref.enqueue(np.nan_to_num(q), np.nan_to_num(g), labels, qv, gv)
        rows, rl, rv = ring.host()
        assert ring.cursor.tolist() == [ref.cursor, ref.written] == [(40 * (step + 1)) % 96, 40 * (step + 1)]
        assert np.array_equal(rl, ref.labels) and np.array_equal(rv, ref.valid)
        live = rv != 0
        assert np.abs(rows - ref.rows)[live].max() <= R.e_unit(D)
        f = ring_reference(ring, q, g, labels, qv, gv, tau, gs)
        assert f['flag'].sum() == P
        check(o, f, need_margin=True)
        assert not bool(o['dq'][dev(qv).reshape(-1) == 0].any()) and not bool(o['dg'][dev(gv) == 0].any())
    # enqueue=False: the ring keeps its bits, the same batch gives the same bits as the run that filed it
    before = [bits(t) for t in ring.mem()] + [bits(ring.cursor)]
    o2 = run(ops, q, g, labels, labels, qv, gv, tau, ring=ring, gscale=gs, enqueue=False)
    assert all(torch.equal(a, bits(t)) for a, t in zip(before, list(ring.mem()) + [ring.cursor]))
    for k in ('q_ap', 'g_ap', 'result', 'dq', 'dg'):
        assert torch.equal(bits(o[k]), bits(o2[k])), k


@pytest.mark.parametrize('M', [4096, 8192])
def test_ring_at_the_sizes_that_opt_into_more_lds(ops, M):
    """A full ring of 4096 / 8192 slots (the rank kernel's score row, lists and coefficients take more than 64 KiB of LDS from 3450 slots
    on, 152 KiB at 8192) against two anchors per side."""
    P, N, D, tau = 1, 2, 32, 0.01
    key = ('big', M)
    if key not in _CASE:
        r = np.random.default_rng(M)
        rows = R.unit_rows(r.standard_normal((P + 1, M, D)))[0].astype(np.float32)
        rl, rv = r.integers(0, 64, M).astype(np.int64), (r.random((P + 1, M)) >= 0.05).astype(np.uint8)
        q, g, _, _, _, _ = labelled_case(P, N, N, D, 1, 7)
        labels = np.array([3, 11], np.int64)
        _CASE[key] = (rows, rl, rv, q, g, labels, R.forward(q, g, labels, labels, None, None, tau, ring=(rows, rl, rv)))
    rows, rl, rv, q, g, labels, f = _CASE[key]
    ring = DeviceRing(M, P + 1, D)
    ring.fill(rows, rl, rv)
    assert f['n_active'].tolist() == [[2.0, 2.0]] and f['q_npos'].min() > 30
    check(run(ops, q, g, labels, labels, None, None, tau, ring=ring), f, need_margin=True)


def test_public_ring_call_and_a_backward_after_a_second_forward():
    from prcv2025reid_amd import losses, _lib
    _lib.set_flavor('bf16')
    P, N, D, M, tau = 2, 40, 32, 96, 0.05
    mem = losses.CrossBatchMemory(M, P + 1, D)
    q1, g1, l1, _, qv1, gv1 = labelled_case(P, N, N, D, 2, 60, invalid=0.1)
    q2, g2, l2, _, _, _ = labelled_case(P, N, N, D, 2, 61)
    a, b = dev(q1).requires_grad_(True), dev(g1).requires_grad_(True)
    L1, flag1, rows1 = losses.smooth_ap_xbm(a, b, dev(l1), mem, dev(qv1), dev(gv1), temperature=tau)
    assert int(mem.rows_written) == N and int(mem.filled) == N
    host1 = (mem.rows.cpu().numpy().copy(), mem.labels.cpu().numpy().copy(), mem.valid.cpu().numpy().copy())
    f1 = R.forward(q1, g1, l1, l1, qv1, gv1, tau, ring=host1, gscale=[1.0, 2.0])
    # a second forward files 40 more rows, a third wraps over the rows the first one ranked
    c, d = dev(q2).requires_grad_(True), dev(g2).requires_grad_(True)
    for _ in range(2):
        L2, _, _ = losses.smooth_ap_xbm(c, d, dev(l2), mem, temperature=tau)
    assert int(mem.rows_written) == 3 * N and not torch.equal(mem.rows.cpu(), torch.from_numpy(host1[0]))
    (L1 * torch.tensor([1.0, 2.0], device='cuda')).sum().backward()
    assert np.abs(L1.detach().cpu().numpy() - f1['loss']).max() <= f1['e_loss'].max() and flag1.tolist() == [1.0, 1.0]
    assert (np.abs(a.grad.cpu().numpy() - f1['dq']) <= f1['e_dq']).all() and (np.abs(b.grad.cpu().numpy() - f1['dg']) <= f1['e_dg']).all()
    assert float(a.grad.abs().max()) > 0 and set(rows1) == {'q_ap', 'g_ap', 'q_npos', 'g_npos', 'n_active'} and rows1['q_ap'].shape == (P, N)
    # enqueue=False and no_grad leave the ring alone; without gradients the workspace is the small one
    before = bits(mem.rows)
    with torch.no_grad():
        L3, _, _ = losses.smooth_ap_xbm(c, d, dev(l2), mem, temperature=tau, enqueue=False)
    L4, _, _ = losses.smooth_ap_xbm(c, d, dev(l2), mem, temperature=tau, enqueue=False)
    assert torch.equal(bits(mem.rows), before) and int(mem.rows_written) == 3 * N and torch.equal(bits(L3), bits(L4)) and not L3.requires_grad
    with pytest.raises(TypeError, match='CrossBatchMemory'):
        losses.smooth_ap_xbm(c, d, dev(l2), mem.rows)
    with pytest.raises(ValueError, match='sides'):
        losses.smooth_ap_xbm(c[:1], d, dev(l2), mem)
    with pytest.raises(ValueError, match='does not fit'):
        losses.smooth_ap_xbm(c, d, dev(l2), losses.CrossBatchMemory(8, P + 1, D))
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.smooth_ap_xbm(c, d, dev(l2), losses.CrossBatchMemory(M, P + 1, 64))


def test_public_batch_call():
    from prcv2025reid_amd import losses, _lib
    _lib.set_flavor('bf16')
    c, gs, f = batch_case(BATCH_CASES[4])
    q, g, ql, gl, qv, gv = c
    a, b = dev(q).requires_grad_(True), dev(g).requires_grad_(True)
    L, flag, rows = losses.smooth_ap(a, b, dev(ql), dev(gl), dev(qv).bool(), dev(gv).bool())
    (L * dev(gs)).sum().backward()
    assert (np.abs(L.detach().cpu().numpy() - f['loss']) <= f['e_loss']).all() and np.array_equal(flag.cpu().numpy(), f['flag'])
    assert np.array_equal(rows['n_active'].cpu().numpy(), f['n_active']) and np.array_equal(rows['q_npos'].cpu().numpy(), f['q_npos'])
    assert (np.abs(a.grad.cpu().numpy() - f['dq']) <= f['e_dq']).all() and (np.abs(b.grad.cpu().numpy() - f['dg']) <= f['e_dg']).all()
    L1, _, r1 = losses.smooth_ap(a[0], b, dev(ql), dev(gl), dev(qv)[0], dev(gv))            # [N, D] = one modality
    assert L1.shape == (1,) and torch.equal(bits(L1[0]), bits(L[0])) and r1['q_ap'].shape == (1, q.shape[1])
    with torch.no_grad():
        Ln, _, _ = losses.smooth_ap(a, b, dev(ql), dev(gl), dev(qv), dev(gv))
    assert torch.equal(bits(Ln), bits(L)) and not Ln.requires_grad
    with pytest.raises(ValueError, match='q_labels'):
        losses.smooth_ap(a, b, dev(gl), dev(gl))


# ---------------------------------------------------------------------------------------------------------------- 3. graphs
def test_graph_replay_equals_eager_bit_for_bit(ops):
    """The term is atomic-free: enqueue, forward and backward captured once as ONE linear chain on the capture stream and replayed three
    times give the bits of three eager rounds -- every round files the batch again, so the ring and the loss move."""
    P, N, D, M, tau = 2, 24, 96, 64, 0.05
    q, g, labels, _, qv, gv = labelled_case(P, N, N, D, 2, 70, invalid=0.1)
    q2, g2, lab = dev(np.nan_to_num(q)).reshape(P * N, D), dev(np.nan_to_num(g)), dev(labels)
    qvd, gvd, gs = dev(qv).reshape(-1).contiguous(), dev(gv), dev(np.array([1.0, -0.5], np.float32))

    def buffers():
        b = dict(rows=torch.zeros(P + 1, M, D, device='cuda'), labels=torch.zeros(M, dtype=torch.int64, device='cuda'),
                 valid=torch.zeros(P + 1, M, dtype=torch.uint8, device='cuda'), cursor=torch.zeros(2, dtype=torch.int32, device='cuda'),
                 ws=torch.empty(ops.smooth_ap_ws_floats(P, N, N, D, M, M, True), device='cuda'), ap=torch.empty(2 * P * N, device='cuda'),
                 npos=torch.empty(2 * P * N, dtype=torch.int32, device='cuda'), res=torch.empty(4 * P, device='cuda'),
                 dq=torch.empty(P * N, D, device='cuda'), dg=torch.empty(N, D, device='cuda'))
        return b

    def round_(b):
        mem = (b['rows'], b['labels'], b['valid'])
        ops.xbm_enqueue(q2, g2, lab, qvd, gvd, True, R.EPS, *mem, b['cursor'], P=P)
        ops.smooth_ap_fwd(q2, g2, lab, lab, qvd, gvd, tau, True, R.EPS, True, b['ap'][:P * N], b['npos'][:P * N], b['ap'][P * N:], b['npos'][P * N:],
                          b['ws'], b['res'], P=P, ring=mem)
        ops.smooth_ap_bwd(qvd, gvd, b['ws'], gs, b['dq'], b['dg'], P=P)

    keys = ('res', 'ap', 'npos', 'dq', 'dg', 'rows', 'cursor')
    eager, outs = buffers(), []
    for _ in range(3):
        round_(eager)
        torch.cuda.synchronize()
        outs.append([bits(eager[k]) for k in keys])
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][5], outs[2][5])        # the rounds differ: the ring fills
    graphed = buffers()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        round_(graphed)
    for k in ('rows', 'labels', 'valid', 'cursor'):
        graphed[k].zero_()                                           # (capture launches nothing; start from the empty ring all the same)
    for i in range(3):
        gr.replay()
        torch.cuda.synchronize()
        for k, want in zip(keys, outs[i]):
            assert torch.equal(bits(graphed[k]), want), (i, k)


# ---------------------------------------------------------------------------------------------------------------- 4. optimisation
def test_five_sgd_steps_follow_the_reference_trajectory():
    """Free unit-length features (P = 2, N = Mg = 16, D = 32), tau = 0.1, plain SGD with lr = 0.05 on the sum of the pair losses.  The
    fp64 reference runs its own trajectory x64.  With a = the largest element-wise deviation of the device's x from x64 so far,
      gradient  |g_dev(x_dev) - g64(x64)| <= e(x_dev) + |g64(x_dev) - g64(x64)|: the derived bound of the kernels at the device's own
                point (fp32 values are fp64 values) plus the reference's own sensitivity between the two points, both from fp64 runs of
                the reference -- neither is taken from the gradient under test;
      x         a' = a + lr * (that) + 2 u max|x|  (the fp32 multiply-add of the step)."""
    from prcv2025reid_amd import losses, _lib
    _lib.set_flavor('bf16')
    P, N, D, tau, lr = 2, 16, 32, 0.1, 0.05
    q, g, ql, gl, _, _ = labelled_case(P, N, N, D, 2, 80)
    q, g = R.unit_rows(q)[0].astype(np.float32), R.unit_rows(g)[0].astype(np.float32)
    qd, gd = dev(q).requires_grad_(True), dev(g).requires_grad_(True)
    q64, g64, a = q.astype(np.float64), g.astype(np.float64), 0.0
    first = None
    for step in range(5):
        f = R.forward(q64, g64, ql, gl, tau=tau)
        here = R.forward(qd.detach().cpu().numpy(), gd.detach().cpu().numpy(), ql, gl, tau=tau)
        L, _, _ = losses.smooth_ap(qd, gd, dev(ql), dev(gl), temperature=tau)
        L.sum().backward()
        e_loss = np.abs(L.detach().cpu().numpy() - here['loss'])
        print(f'step {step}: loss {float(L.detach().sum()):.6f} reference {f["loss"].sum():.6f} deviation of x {a:.3e}')
        assert (e_loss <= here['e_loss']).all()
        first = f['loss'].sum() if first is None else first
        e_q = here['e_dq'] + np.abs(here['dq'] - f['dq'])
        e_g = here['e_dg'] + np.abs(here['dg'] - f['dg'])
        assert (np.abs(qd.grad.cpu().numpy() - f['dq']) <= e_q).all() and (np.abs(gd.grad.cpu().numpy() - f['dg']) <= e_g).all()
        with torch.no_grad():
            qd.add_(qd.grad, alpha=-lr); gd.add_(gd.grad, alpha=-lr)
            qd.grad = gd.grad = None
        q64, g64 = q64 - lr * f['dq'], g64 - lr * f['dg']
        a = a + lr * max(e_q.max(), e_g.max()) + 2 * U * max(np.abs(q64).max(), np.abs(g64).max())
        dev_x = max(np.abs(qd.detach().cpu().numpy() - q64).max(), np.abs(gd.detach().cpu().numpy() - g64).max())
        assert dev_x <= a, (step, dev_x, a)
    assert R.forward(q64, g64, ql, gl, tau=tau)['loss'].sum() < first - 0.01          # the steps descend


# ---------------------------------------------------------------------------------------------------------------- 5. model level
BASE_KEYS = ['total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt']
NEW_KEYS = ['smooth_ap_loss', 'smooth_ap_active_cnt']


def _tiny8(**over):
    """The tiny frozen model with a batch of 8 instances (4 identities x 2, every modality present), as tests/test_loss_terms_gpu.py."""
    from helpers import load_case, case_inputs
    from prcv2025reid_amd.synthetic import synthetic_batch
    from test_model_gpu import build_model
    z, meta = load_case('tiny_train_frozen')
    cfg, arch, state, _, _ = case_inputs(meta)
    batch = synthetic_batch(4, 2, arch, seed=7, mask_drop=0.0, num_classes=int(meta['num_classes']))
    return meta, state, batch, (lambda **kw: build_model(meta, state, True, **{**over, **kw}))


def _inputs(batch):
    return ({m: t.cuda() for m, t in batch['images'].items()}, {m: t.cuda() for m, t in batch['modality_mask'].items()}, batch['person_id'].cuda())


def _pairs_of(out):
    """(q [P, B, D], g [B, D], q_valid [P, B], g_valid [B]) the model's term must have used, as numpy."""
    raw, fm = out['raw_modality_features'], out['feature_masks']
    mods = [m for m in raw if m != 'vis' and m in fm]
    assert len(mods) >= 2
    q = torch.stack([raw[m].detach() for m in mods]).cpu().numpy()
    qv = torch.stack([fm[m].cuda() > 0 for m in mods]).cpu().numpy().astype(np.uint8)
    return q, raw['vis'].detach().cpu().numpy(), qv, (fm['vis'].cuda() > 0).cpu().numpy().astype(np.uint8)


def test_weight_zero_is_the_model_without_the_fields():
    from helpers import case_config
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    meta, state, batch, make = _tiny8()
    images, masks, labels = _inputs(batch)
    cfg = case_config(meta, device='cuda')
    cfg.compute_dtype = 'bf16'
    bare = types.SimpleNamespace(**{k: v for k, v in vars(cfg).items() if not k.startswith('smooth_ap_')})
    assert not hasattr(bare, 'smooth_ap_weight') and hasattr(cfg, 'smooth_ap_weight')
    old = CLIPBasedMultiModalReIDModel(bare)
    old.set_num_classes(int(meta['num_classes'])); old.load_state_dict(state, strict=True); apply_reference_freeze(old)
    old.contrastive_weight = meta['contrastive_weight']; old.set_epoch(2); old.train(True)
    L_old = old.compute_loss(old(images=images, texts=batch['texts'], modality_masks=masks), labels)
    new = make(smooth_ap_weight=0.0, smooth_ap_size=16)
    L_new = new.compute_loss(new(images=images, texts=batch['texts'], modality_masks=masks), labels)
    assert list(L_old) == list(L_new) == BASE_KEYS and new.smooth_ap_memory is None and old.smooth_ap_memory is None
    for k in BASE_KEYS[:-1]:
        assert torch.equal(bits(L_old[k]), bits(L_new[k])), k
    assert int(L_old['ce_valid_cnt']) == int(L_new['ce_valid_cnt'])
    late = make(smooth_ap_weight=0.5, smooth_ap_start_epoch=5)       # before its start epoch the term is off as well
    assert list(late.compute_loss(late(images=images, texts=batch['texts'], modality_masks=masks), labels)) == BASE_KEYS


@pytest.mark.parametrize('size', [0, 16])
def test_model_loss_with_the_smooth_ap_term(size):
    meta, state, batch, make = _tiny8()
    images, masks, labels = _inputs(batch)
    w, tau = 0.5, 0.05
    model = make(smooth_ap_weight=w, smooth_ap_temperature=tau, smooth_ap_size=size)
    model.contrastive_weight = 0.0                                   # the weight alone builds the stack
    keys_before = set(model.state_dict())
    out = model(images=images, texts=batch['texts'], modality_masks=masks)
    model.smooth_ap_weight = 0.0
    L0 = model.compute_loss(out, labels)
    assert list(L0) == BASE_KEYS and model.smooth_ap_memory is None
    model.smooth_ap_weight = w
    L1 = model.compute_loss(out, labels)
    assert list(L1) == BASE_KEYS + NEW_KEYS
    assert torch.equal(L1['total_loss'], L0['total_loss'] + w * L1['smooth_ap_loss'])     # the previous total plus weight * term, bit for bit
    q, g, qv, gv = _pairs_of(out)
    P, B, D = q.shape
    lab = labels.cpu().numpy()
    ring = None
    if size:
        mem = model.smooth_ap_memory
        assert mem is not None and mem is not model.xbm_memory and (mem.capacity, mem.sides, mem.dim) == (size, P + 1, D) and int(mem.rows_written) == B
        ring = (mem.rows.cpu().numpy(), mem.labels.cpu().numpy(), mem.valid.cpu().numpy())
    else:
        assert model.smooth_ap_memory is None
    f = R.forward(q, g, lab, lab, qv, gv, tau, ring=ring)
    want = f['loss'].sum() / max(f['flag'].sum(), 1)
    assert f['flag'].sum() > 0 and int(L1['smooth_ap_active_cnt']) == int(f['n_active'].sum()) > 0
    assert abs(float(L1['smooth_ap_loss'].detach()) - want) <= f['e_loss'].sum() / f['flag'].sum() + 2 * U * want
    model.lora_arena.grad = None
    L1['total_loss'].backward()
    assert float(model.lora_arena.grad.abs().max()) > 0
    assert set(model.state_dict()) == keys_before                    # the ring is no parameter and no buffer
    if size:
        # eval() and no_grad(): the loss is there, the ring stays; reset empties it; another modality set is refused
        before = bits(mem.rows)
        with torch.no_grad():
            Ln = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), labels)
        model.eval()
        Le = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), labels)
        torch.cuda.synchronize()
        assert 'smooth_ap_loss' in Ln and 'smooth_ap_loss' in Le and torch.equal(bits(mem.rows), before) and int(mem.rows_written) == B
        model.train(True)
        model.compute_loss(out, labels)
        assert int(mem.rows_written) == 2 * B
        model.reset_smooth_ap()
        assert model.smooth_ap_memory is mem and int(mem.rows_written) == 0 and int(mem.filled) == 0 and not bool(mem.valid.any())
        model._smooth_ap_sides = ('nir',)
        with pytest.raises(ValueError, match='Smooth-AP memory was made for'):
            model.compute_loss(out, labels)
    else:
        model.reset_smooth_ap()                                      # nothing to empty: no error


def test_graphed_step_with_the_smooth_ap_term_matches_eager():
    """The shapes, warm-up, comparison and tolerance of test_cluster_nce_gpu.test_graphed_step_with_the_cluster_term_matches_eager (2
    warm-up steps and 3 replays against 5 eager steps; the rest of the step has atomics, hence the 2e-3): the ring lives on the device,
    its cursor too, so the replays keep filing rows.  One linear chain; no queue setting is touched."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_triplet_gpu import _tiny
    meta, state, batch_, build = _tiny()
    images = {m: t.cuda() for m, t in batch_['images'].items()}
    masks = dict(batch_['modality_mask'])
    labels = batch_['person_id'].cuda()
    B = labels.shape[0]

    def make():
        m = build(smooth_ap_weight=0.5, smooth_ap_temperature=0.05, smooth_ap_size=3 * B)
        gs = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in m.get_learnable_params()]
        return m, StepDriver(m, FusedAdamW(gs, weight_decay=1e-4))

    a, da = make()
    tok = a.tokenizer(batch_['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
    tok = {k: v.cuda() for k, v in tok.items()}
    g = GraphedStep(da, images, tok, masks, labels, warmup=2)
    for _ in range(3):
        La = g.step(images, tok, masks, labels)
    torch.cuda.synchronize()
    b, db = make()
    for _ in range(5):
        Lb = db.step(images, tok, masks, labels)
    assert da.opt.step_count == db.opt.step_count == 5
    assert float(Lb['smooth_ap_loss'].detach()) > 0 and int(Lb['smooth_ap_active_cnt']) == int(La['smooth_ap_active_cnt']) > 0
    for k in ('total_loss', 'smooth_ap_loss'):
        va, vb = float(La[k].detach()), float(Lb[k].detach())
        assert abs(va - vb) <= 2e-3 * max(1.0, abs(vb)), k
    ma, mb = a.smooth_ap_memory, b.smooth_ap_memory
    assert int(mb.rows_written) == 5 * B and int(mb.filled) == 3 * B
    if int(ma.rows_written) == 5 * B:                                # (a capture pass that files a batch of its own only shifts the cursor)
        assert torch.equal(ma.labels, mb.labels) and torch.equal(ma.valid, mb.valid)
        assert bool(((ma.rows - mb.rows).abs() <= 2e-3).all())
