"""GPU: the cross-batch memory kernels (csrc/xbm.hip) -- the ring, the mining against it, the anchors-only backward -- per element
against the fp64 reference (xbm_ref.py) along a stream of batches, in both library flavours, and the loss behind the public call,
inside the model and in the graphed step.

Every output and every tensor of the memory lives between 32 guard elements that hold a sentinel pattern and must keep it; padded
input rows carry NaN in their padding.

Bounds (u = 2^-24): those of test_cross_triplet_gpu.py --
  * the ring: rows, labels, validity bytes and cursor EQUAL the shadow ring after every step; the stored rows bit for bit
    ops.l2norm_rows of the batch (normalize = 1) or the batch (normalize = 0);
  * distances: |d - d64| <= cross_triplet_ref.dist_bound at the kernel's own selection; selection: for EVERY active anchor the fp64
    distance of the kernel's choice is within that bound of the fp64 extreme (no exemptions); counts and flags exact;
  * L_p: 4 u (1 + |L|) + the distance bound averaged over the active anchors of both directions;
  * gradients: per element against the fp64 gradient at the kernel's own selection (the memory constant), relative to the row's
    largest |dx|: 1e-5 for normalize = 0 (the project's gate), GATE_NORM for normalize = 1.

GATE_NORM = twice the worst case measured over all cases of this file against xbm_ref.gradient on an MI355X, rounded up to one
significant digit (the rule of test_cross_triplet_gpu.GRAD_GATE).  Measured (both flavours give the same bits, the kernels are fp32):
normalize = 1: 4.94e-6 of the row maximum -> GATE_NORM = 1e-5 (2 x 4.94e-6 = 9.9e-6, rounded up); normalize = 0: 4.70e-6 (gate 1e-5).
Distances: at most 0.018 of their bound with normalize = 1 and 0.35 with normalize = 0; L_p: 0.10 of its tolerance; profiles/xbm_summary.md.

A fresh memory after one enqueue holds the batch alone: the loss then EQUALS the in-batch loss of ops.cross_triplet_fwd bit for bit,
because triplet::mine_tile and triplet::refine_anchor are reused unchanged (test_fresh_memory_equals_the_in_batch_loss).
"""
import pytest
import torch

import cross_triplet_ref as R
import xbm_ref as X
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 32
U = R.U
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
# normalize -> gate on |dx - dx64| / row maximum.  True: twice the worst case measured over every case of this file (4.94e-6), rounded up
# to one significant digit
GRAD_GATE = {False: 1e-5, True: 1e-5}
WORST = {}
_BATCH = {}                              # (P, N, D, ratio, s) -> the stream's batch on the device
_MINED = {}                              # (shape, ratio, normalize, s) -> the reference's selection, shared by margins and flavours
BYTE = 0xA5


@pytest.fixture(scope='module', autouse=True)
def report_worst():
    yield
    print(f'\n  worst over the module: {WORST}')


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


def guarded(n, dtype):
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


def note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))


class Mem:
    """A fresh memory as the C ABI takes it, every tensor between guards."""

    def __init__(self, P, M, D):
        self.P, self.M, self.D = P, M, D
        self.b_rows, rows = guarded((P + 1) * M * D, torch.float32)
        self.b_labels, self.labels = guarded(2 * M, torch.int64)
        self.b_cursor, self.cursor = guarded(2, torch.int32)
        self.b_valid = torch.full((2 * 4 * GUARD + (P + 1) * M,), BYTE, dtype=torch.uint8, device='cuda')
        self.valid = self.b_valid[4 * GUARD:4 * GUARD + (P + 1) * M].view(P + 1, M)
        self.rows = rows.view(P + 1, M, D)
        for t in (self.rows, self.labels, self.cursor, self.valid):
            t.zero_()

    def tensors(self):
        return self.rows, self.labels, self.valid

    def assert_intact(self):
        n = (self.P + 1) * self.M
        assert untouched(self.b_rows, n * self.D) and untouched(self.b_labels, 2 * self.M) and untouched(self.b_cursor, 2), 'memory guards'
        assert bool((self.b_valid[:4 * GUARD] == BYTE).all()) and bool((self.b_valid[4 * GUARD + n:] == BYTE).all()), 'validity guards'

    def bits(self):
        return [self.rows.view(torch.int32).clone(), self.labels.clone(), self.valid.clone(), self.cursor.clone()]


def batch(P, N, D, ratio, s):
    key = (P, N, D, ratio, s)
    if key not in _BATCH:
        _BATCH[key] = X.stream_step(P, N, D, ratio, s, 'cuda')
    return _BATCH[key]


def u8(v):
    return None if v is None else v.to(torch.uint8).reshape(-1).contiguous()


def run_enqueue(ops, mem, q, g, labels, qv, gv, normalize, pad=0):
    ops.xbm_enqueue(strided(q, pad), strided(g, pad), labels, u8(qv), u8(gv), normalize, R.EPS, *mem.tensors(), mem.cursor, P=q.shape[0])
    torch.cuda.synchronize()
    mem.assert_intact()


def run_fwd(ops, mem, q, g, labels, qv, gv, margin, normalize, pad=0):
    """The forward of q [P, N, D], g [N, D] against ``mem`` as it stands; every output between guards.  Returns the outputs (flat, as the
    C ABI has them) and the selection as [P, N] tensors."""
    P, N, D = q.shape
    sizes = dict(q_d=2 * P * N, q_idx=2 * P * N, g_d=2 * P * N, g_idx=2 * P * N, result=4 * P, ws=ops.xbm_ws_floats(P, N, mem.M, D))
    bufs = {k: guarded(n, torch.int32 if k.endswith('idx') else torch.float32) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    o['q2'], o['g2'], o['qv'], o['gv'] = strided(q, pad), strided(g, pad), u8(qv), u8(gv)
    ops.xbm_triplet_fwd(o['q2'], o['g2'], labels, o['qv'], o['gv'], -1.0 if margin is None else margin, normalize, R.EPS, *mem.tensors(),
                        o['q_d'], o['q_idx'], o['g_d'], o['g_idx'], o['ws'], o['result'], P=P)
    torch.cuda.synchronize()
    mem.assert_intact()
    for k, (buf, view) in bufs.items():
        assert untouched(buf, view.numel()), f'{k}: guard elements overwritten'
        if k != 'ws':                                               # (ws: only the parts this case needs are written)
            assert not bool((view.view(torch.int32) == SENTINEL32).any()), f'{k}: elements not written'
    o['sel'] = dict(q_idx_p=o['q_idx'][:P * N].view(P, N).long(), q_idx_n=o['q_idx'][P * N:].view(P, N).long(),
                    g_idx_p=o['g_idx'][:P * N].view(P, N).long(), g_idx_n=o['g_idx'][P * N:].view(P, N).long())
    o['d'] = dict(q_d_ap=o['q_d'][:P * N].view(P, N), q_d_an=o['q_d'][P * N:].view(P, N),
                  g_d_ap=o['g_d'][:P * N].view(P, N), g_d_an=o['g_d'][P * N:].view(P, N))
    o['res'] = o['result'].view(P, 4)
    o.update(P=P, margin=margin, normalize=normalize)
    return o


def run_bwd(ops, o, gscale, pad=4):
    """The backward from what run_fwd left (the memory is not an argument); dq [P N, D] and dg [N, D] between guard rows and
    sentinel padding columns."""
    outs = []
    for x in (o['q2'], o['g2']):
        rows, D = x.shape
        buf = torch.full((rows + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda').view(torch.float32)
        outs.append((buf, buf[GUARD:GUARD + rows, :D]))
    (bq, dq), (bg, dg) = outs
    ops.xbm_triplet_bwd(o['q2'], o['g2'], o['qv'], o['gv'], -1.0 if o['margin'] is None else o['margin'], o['normalize'], R.EPS, o['q_d'],
                        o['q_idx'], o['g_d'], o['g_idx'], o['ws'], o['result'], torch.tensor(gscale, dtype=torch.float32, device='cuda'),
                        dq, dg, P=o['P'])
    torch.cuda.synchronize()
    for name, buf, dx in (('dq', bq, dq), ('dg', bg, dg)):
        raw, rows, D = buf.view(torch.int32), dx.shape[0], dx.shape[1]
        assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + rows:] == SENTINEL32).all()), f'{name}: guard rows overwritten'
        assert bool((raw[GUARD:GUARD + rows, D:] == SENTINEL32).all()), f'{name}: padding columns overwritten'
        assert bool(torch.isfinite(dx).all()), name
    return dq, dg


def check_fwd(o, ring, q, g, labels, qv, gv, mined=None):
    """Every forward output against the reference on the shadow ring (``mined``: its selection, when the caller keeps one); returns
    the reference at the kernel's own selection."""
    P, N, D = q.shape
    margin, normalize = o['margin'], o['normalize']
    m = F32(margin) if margin is not None else None
    ref = dict(mined if mined is not None else X.mine(ring, q, g, labels, qv, gv, normalize))
    ref.update(X.evaluate(ring, q, g, ref, m, normalize))
    sel = o['sel']
    own = X.evaluate(ring, q, g, sel, m, normalize)
    assert [float(v) for v in o['res'][:, 2]] == ref['n_q'] == own['n_q'] and [float(v) for v in o['res'][:, 3]] == ref['n_g'] == own['n_g']
    assert [float(v) for v in o['res'][:, 1]] == ref['flag']
    tol_L = []
    for s in 'qg':
        ip, inn = sel[f'{s}_idx_p'], sel[f'{s}_idx_n']
        act = ref[f'{s}_idx_p'] >= 0
        assert bool(((ip >= 0) == act).all()) and bool(((inn >= 0) == act).all())
        assert bool((ip[~act] == -1).all()) and bool((inn[~act] == -1).all())
        assert bool((ip[act] < ring.M).all()) and bool((inn[act] < ring.M).all())
        mean_bound = torch.zeros(P, dtype=torch.float64, device=q.device)
        for k in ('d_ap', 'd_an'):
            # selection: the fp64 distance of the kernel's choice against the fp64 extreme -- every anchor
            best, mine_ = ref[f'{s}_{k}'], own[f'{s}_{k}']
            bound = R.dist_bound(D, best, normalize)
            short = (best - mine_) if k == 'd_ap' else (mine_ - best)
            assert bool((short[act] >= -1e-13).all()) and bool((short[act] <= bound[act]).all()), (s, k, float((short / bound)[act].max()))
            # distances: the kernel's value against fp64 at its own selection
            got = o['d'][f'{s}_{k}'].double()
            err, allow = (got - mine_).abs(), R.dist_bound(D, mine_, normalize)
            if bool(act.any()):
                note(f'{k} err / bound (normalize={int(normalize)})', (err / allow)[act].max())
            assert bool((err[act] <= allow[act]).all()), (s, k, float((err / allow)[act].max()))
            assert bool((got[~act] == 0).all())
            mean_bound += (allow * act).sum(1) / act.sum(1).clamp(min=1)
        # the chosen slots hold a valid row of the right kind
        lab_p, lab_n = ring.labels[ip.clamp(min=0)], ring.labels[inn.clamp(min=0)]
        assert bool((lab_p == labels[None, :])[act].all()) and bool((lab_n != labels[None, :])[act].all())
        tol_L.append(mean_bound)
    for p in range(P):
        tol = 4 * U * (1 + abs(own['L'][p])) + 0.5 * float(tol_L[0][p] + tol_L[1][p])
        err = abs(float(o['res'][p, 0]) - own['L'][p])
        note('L err / tol', err / tol)
        assert err <= tol, (p, float(o['res'][p, 0]), own['L'][p], tol)
        if ref['flag'][p] == 0:
            assert float(o['res'][p, 0]) == 0.0
    return own


def check_bwd(dq, dg, ring, q, g, o, gscale):
    """dq, dg against the fp64 gradient at the kernel's own selection, the ring (as it stood at the forward) constant; returns it."""
    margin, normalize = o['margin'], o['normalize']
    rq, rg = X.gradient(ring, q, g, F32(margin) if margin is not None else None, normalize, o['sel'], [F32(v) for v in gscale])
    rq = rq.reshape(-1, rq.shape[-1])
    for name, dx, ref in (('dq', dq, rq), ('dg', dg, rg)):
        rowmax = ref.abs().max(dim=1, keepdim=True).values
        err = (dx.double() - ref).abs()
        live = rowmax.flatten() > 0
        if bool(live.any()):
            note(f'dx err / row max (normalize={int(normalize)})', (err[live] / rowmax[live]).max())
        assert bool((err <= GRAD_GATE[bool(normalize)] * rowmax).all()), (name, float((err / rowmax.clamp(min=1e-300)).max()))
    return rq, rg


def assert_live(grads, L):
    """The comparison that went before is not 0 against 0."""
    assert max(L) > 0 and all(float(t.abs().max()) > 0 for t in grads)


def stored(ops, x, normalize):
    """What the ring must hold for the rows x [.., D]: ops.l2norm_rows of them, or the rows."""
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    if not normalize:
        return x2.reshape(x.shape)
    y = torch.empty_like(x2)
    ops.l2norm_rows(x2, y=y, eps=R.EPS)
    return y.reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------- 1. the ring
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('shape', X.SHAPES)
def test_enqueue_files_the_stream_as_the_shadow_ring(ops, shape, normalize):
    P, N, D, M, pad = shape
    mem, raw, kept = Mem(P, M, D), X.Ring(P, M, D, 'cuda'), X.Ring(P, M, D, 'cuda')        # kept: the shadow ring of the STORED rows
    for s in range(1, X.STEPS + 1):
        q, g, lab = batch(P, N, D, 30.0, s)
        qv = torch.ones(P, N, dtype=torch.uint8, device='cuda'); gv = torch.ones(N, dtype=torch.uint8, device='cuda')
        if s in (2, 5):                                          # invalid rows are stored, with validity 0
            qv[P - 1, N // 2] = 0; gv[N - 1] = 0
        run_enqueue(ops, mem, q, g, lab, qv if s != 1 else None, gv if s != 1 else None, normalize, pad)
        raw.enqueue(q, g, lab, qv, gv)
        kept.enqueue(stored(ops, q, normalize), stored(ops, g, normalize), lab, qv, gv)
        assert torch.equal(mem.rows.view(torch.int32), kept.rows.view(torch.int32)), s
        assert torch.equal(mem.labels, raw.labels) and torch.equal(mem.valid != 0, raw.valid) and bool((mem.valid <= 1).all()), s
        assert mem.cursor.tolist() == [raw.cursor, raw.written] == [(s * N) % M, s * N], s
        if s * N < M:                                            # slots never written: validity 0, rows untouched
            assert not bool(mem.valid[:, s * N:].any()) and float(mem.rows[:, s * N:].abs().max()) == 0.0
    if N > 1:
        assert raw.written > M and not bool(raw.valid.all())


# ---------------------------------------------------------------------------------------------------------------- 2. along the stream
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, 1.5, None])
@pytest.mark.parametrize('ratio', [0.0, 30.0, 100.0])
@pytest.mark.parametrize('shape', X.SHAPES)
def test_forward_and_backward_along_the_stream(ops, shape, ratio, margin, normalize):
    P, N, D, M, pad = shape
    mem, ring = Mem(P, M, D), X.Ring(P, M, D, 'cuda')
    gscale = [0.75 - 0.5 * p for p in range(P)]                 # per pair, some of them negative
    older = 0
    for s in range(1, X.STEPS + 1):
        q, g, lab = batch(P, N, D, ratio, s)
        run_enqueue(ops, mem, q, g, lab, None, None, normalize, pad)
        slots = ring.enqueue(q, g, lab)
        key = (shape, ratio, normalize, s)
        if key not in _MINED:
            _MINED[key] = X.mine(ring, q, g, lab, None, None, normalize)
        o = run_fwd(ops, mem, q, g, lab, None, None, margin, normalize, pad)
        own = check_fwd(o, ring, q, g, lab, None, None, mined=_MINED[key])
        dq, dg = run_bwd(ops, o, gscale)
        rq, rg = check_bwd(dq, dg, ring, q, g, o, gscale)
        act_q = (o['sel']['q_idx_p'] >= 0).reshape(-1)
        act_g = (o['sel']['g_idx_p'] >= 0).any(0)
        if not bool(act_q.any() | act_g.any()):                  # (one row: one identity, nobody is active)
            assert N == 1 and own['flag'] == [0.0] * P and float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0
        elif margin is None or normalize:                       # soft margin, or unit rows (d < 2: hinges at 0.3 and 1.5 are open)
            assert_live((rq, rg), own['L'])
        if margin is None:                                      # every hinge open: every active anchor's row carries gradient
            assert bool((dq.abs().max(dim=1).values > 0)[act_q].all()) and bool((dg.abs().max(dim=1).values > 0)[act_g].all())
        assert not bool((dq.abs().max(dim=1).values > 0)[~act_q].any()) and not bool((dg.abs().max(dim=1).values > 0)[~act_g].any())
        cur = set(slots.tolist())
        older += sum(1 for k in o['sel'] for j in o['sel'][k].flatten().tolist() if j >= 0 and j not in cur)
    if N > 1 and M >= 2 * N:
        assert older > 0                                         # the memory mattered: rows of older batches were kept
    print(f'  {shape} ratio={ratio:g} margin={margin} normalize={normalize}: L={[round(v, 4) for v in own["L"]]} older picks {older} '
          f'worst so far {WORST}')


# ---------------------------------------------------------------------------------------------------------------- 3. fresh memory
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('fixture', R.EXACT_INDEX)
def test_fresh_memory_equals_the_in_batch_loss(ops, fixture, normalize):
    """An empty memory, cursor 0, one enqueue + forward: the candidates are the batch alone, in slots 0 .. N-1 -- the indices, the
    distances, L_p, the counts and the flags EQUAL those of ops.cross_triplet_fwd on the same batch BIT FOR BIT (mine_tile and
    refine_anchor are reused unchanged; mining is not split over workgroups).  (The fixtures' two sides are cut to their common
    length: row i of every side is one instance here.)"""
    shape, ratio = fixture
    q, g, ql, gl = R.fixture(shape, ratio, 'cuda')
    n = min(q.shape[1], g.shape[0])
    q, g, lab = q[:, :n].contiguous(), g[:n].contiguous(), ql[:n].contiguous()
    assert torch.equal(lab, gl[:n])
    P, _, D = q.shape
    for M in (n, n + 5, 300):
        mem = Mem(P, M, D)
        run_enqueue(ops, mem, q, g, lab, None, None, normalize)
        o = run_fwd(ops, mem, q, g, lab, None, None, 0.3, normalize)
        ws = torch.empty(ops.cross_triplet_ws_floats(P, n, n, D), device='cuda')
        qd = torch.empty(2 * P * n, device='cuda'); qi = torch.empty(2 * P * n, dtype=torch.int32, device='cuda')
        gd = torch.empty(2 * P * n, device='cuda'); gi = torch.empty(2 * P * n, dtype=torch.int32, device='cuda')
        res = torch.empty(P, 4, device='cuda')
        ops.cross_triplet_fwd(q.reshape(P * n, D), g, lab, lab, None, None, 0.3, normalize, R.EPS, qd, qi, gd, gi, ws, res, P=P)
        torch.cuda.synchronize()
        assert torch.equal(o['q_idx'], qi) and torch.equal(o['g_idx'], gi), M
        assert torch.equal(o['q_d'].view(torch.int32), qd.view(torch.int32)) and torch.equal(o['g_d'].view(torch.int32), gd.view(torch.int32)), M
        assert torch.equal(o['res'].view(torch.int32), res.view(torch.int32)), M
    if n > 1:                                                    # (between unit rows the hinge at 0.3 is open; unnormalised it may be shut)
        assert float(res[:, 1].min()) == 1.0 and (float(res[:, 0].max()) > 0 or not normalize)


# ---------------------------------------------------------------------------------------------------------------- 4. ties, degenerate cases
def tie_case(device='cuda'):
    """P = 1, N = 64, D = 96, M = 576: nine batches.  For q anchor 0 of the LAST batch (slots 512 .. 575), in memory side 0: tied
    farthest positives in slots 44 and 300 (the same lane of two 256-slot candidate pieces), tied nearest negatives in slots 10 and 80
    (two waves of one piece).  For g anchor 5 of the last batch, in memory side 1: tied farthest positives in slot 11 (an old batch)
    and slot 512 + 7 (the current one), tied nearest negatives in slots 45 and 512 + 20.  (The tied positives are -3 x the anchor: the
    farthest row with unit rows, at distance 2, and without; the tied negatives the anchor + 0.5 per column, a quarter of the typical
    distance.  Ratio 0: every batch of the stream has its own common mean, which would outweigh both.)  Returns the nine batches."""
    P, N, D = 1, 64, 96
    bs = [[t.clone() for t in X.stream_step(P, N, D, 0.0, s, device)] for s in range(1, 10)]
    w = 0.5 * torch.sign(torch.randn(D, generator=torch.Generator().manual_seed(4))).to(device)
    (q9, g9, l9) = bs[8]
    row = lambda slot: (bs[slot // N], slot % N)
    a, la = q9[0, 0], int(l9[0])
    for slot in (44, 300):
        (q_, g_, l_), i = row(slot)
        g_[i] = -3.0 * a; l_[i] = la
    for slot in (10, 80):
        (q_, g_, l_), i = row(slot)
        g_[i] = a + w; l_[i] = la + 100
    b, lb = g9[5], int(l9[5])
    for slot in (11, 512 + 7):
        (q_, g_, l_), i = row(slot)
        q_[0, i] = -3.0 * b; l_[i] = lb
    for slot in (45, 512 + 20):
        (q_, g_, l_), i = row(slot)
        q_[0, i] = b + w; l_[i] = lb + 200
    return bs


def tie_reference(bs, normalize):
    ring = X.Ring(1, 576, 96, bs[0][0].device)
    for q, g, lab in bs:
        ring.enqueue(q, g, lab)
    q, g, lab = bs[8]
    ref = X.reference(ring, q, g, lab, None, None, F32(0.3), normalize)
    assert (int(ref['q_idx_p'][0, 0]), int(ref['q_idx_n'][0, 0])) == (44, 10) and float(ref['q_gap_p'][0, 0]) == 0.0 == float(ref['q_gap_n'][0, 0])
    assert (int(ref['g_idx_p'][0, 5]), int(ref['g_idx_n'][0, 5])) == (11, 45) and float(ref['g_gap_p'][0, 5]) == 0.0 == float(ref['g_gap_n'][0, 5])
    return ring


@pytest.mark.parametrize('normalize', [True, False])
def test_exact_ties_go_to_the_lowest_slot(ops, normalize):
    bs = tie_case()
    ring = tie_reference(bs, normalize)
    mem = Mem(1, 576, 96)
    for q, g, lab in bs:
        run_enqueue(ops, mem, q, g, lab, None, None, normalize)
    q, g, lab = bs[8]
    o = run_fwd(ops, mem, q, g, lab, None, None, 0.3, normalize)
    assert (int(o['sel']['q_idx_p'][0, 0]), int(o['sel']['q_idx_n'][0, 0])) == (44, 10)
    assert (int(o['sel']['g_idx_p'][0, 5]), int(o['sel']['g_idx_n'][0, 5])) == (11, 45)
    own = check_fwd(o, ring, q, g, lab, None, None)
    dq, dg = run_bwd(ops, o, [1.0])
    assert_live(check_bwd(dq, dg, ring, q, g, o, [1.0]), own['L'])


@pytest.mark.parametrize('normalize', [True, False])
def test_all_invalid_batch_and_single_identity(ops, normalize):
    P, N, D, M = 2, 16, 96, 48
    mem, ring = Mem(P, M, D), X.Ring(P, M, D, 'cuda')
    q, g, lab = batch(P, N, D, 30.0, 1)
    # one identity only: every anchor has positives and no negative
    one = torch.full_like(lab, 7)
    run_enqueue(ops, mem, q, g, one, None, None, normalize); ring.enqueue(q, g, one)
    o = run_fwd(ops, mem, q, g, one, None, None, 0.3, normalize)
    check_fwd(o, ring, q, g, one, None, None)
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    assert all(bool((v == -1).all()) for v in o['sel'].values()) and float(o['res'].abs().max()) == 0.0
    assert float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0
    # an all-invalid batch: stored with validity 0, nobody is an anchor -- though the memory holds candidates of both kinds for them
    q2, g2, lab2 = batch(P, N, D, 30.0, 2)
    zq, zg = torch.zeros(P, N, dtype=torch.uint8, device='cuda'), torch.zeros(N, dtype=torch.uint8, device='cuda')
    run_enqueue(ops, mem, q2, g2, lab2, zq, zg, normalize); ring.enqueue(q2, g2, lab2, zq, zg)
    assert not bool(mem.valid[:, N:2 * N].any()) and bool(mem.valid[:, :N].all())
    o = run_fwd(ops, mem, q2, g2, lab2, zq, zg, 0.3, normalize)
    check_fwd(o, ring, q2, g2, lab2, zq, zg)
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    assert all(bool((v == -1).all()) for v in o['sel'].values()) and float(o['res'].abs().max()) == 0.0
    assert float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0
    # the same batch, valid, mined WITHOUT being enqueued: its own slots are invalid, the single-identity batch supplies the negatives
    # only -> still nobody active; after a valid third batch the anchors are
    o = run_fwd(ops, mem, q2, g2, lab2, None, None, 0.3, normalize)
    check_fwd(o, ring, q2, g2, lab2, None, None)
    assert float(o['res'][:, 1].max()) == 0.0
    q3, g3, lab3 = batch(P, N, D, 30.0, 3)
    run_enqueue(ops, mem, q3, g3, lab3, None, None, normalize); ring.enqueue(q3, g3, lab3)
    o = run_fwd(ops, mem, q3, g3, lab3, None, None, 0.3, normalize)
    own = check_fwd(o, ring, q3, g3, lab3, None, None)
    assert own['flag'] == [1.0] * P and own['n_q'] == [N] * P


@pytest.mark.parametrize('normalize', [True, False])
def test_an_identity_whose_positives_were_overwritten_is_inactive(ops, normalize):
    """Identity 50 lives in rows 0 .. 3 of batch 1 only; in batch 2 row 0 carries it on the q side while its vis row is invalid.  With
    M = 2 N batch 1 is still in the memory and q anchor 0 finds its positives there; with M = N batch 2 has just overwritten them."""
    P, N, D = 1, 8, 96
    q1, g1, lab1 = [t.clone() for t in batch(P, N, D, 30.0, 1)]
    q2, g2, lab2 = [t.clone() for t in batch(P, N, D, 30.0, 2)]
    lab1[:4] = 50; lab2[0] = 50
    gv2 = torch.ones(N, dtype=torch.uint8, device='cuda'); gv2[0] = 0
    for M, active in ((2 * N, True), (N, False)):
        mem, ring = Mem(P, M, D), X.Ring(P, M, D, 'cuda')
        run_enqueue(ops, mem, q1, g1, lab1, None, None, normalize); ring.enqueue(q1, g1, lab1)
        run_enqueue(ops, mem, q2, g2, lab2, None, gv2, normalize); ring.enqueue(q2, g2, lab2, None, gv2)
        o = run_fwd(ops, mem, q2, g2, lab2, None, gv2, None, normalize)
        own = check_fwd(o, ring, q2, g2, lab2, None, gv2)
        dq, dg = run_bwd(ops, o, [1.0])
        check_bwd(dq, dg, ring, q2, g2, o, [1.0])
        ip = int(o['sel']['q_idx_p'][0, 0])
        assert (0 <= ip < 4) if active else ip == -1
        assert (float(dq[0].abs().max()) > 0) == active and float(dg[0].abs().max()) == 0.0
        assert own['n_q'] == [N if active else N - 1] and own['n_g'] == [N - 1]


def test_hinge_exactly_at_zero_has_no_gradient(ops):
    # integers as floats: q anchor 0 has d_ap = 5 (slot 1), d_an = 6 (slot 2), margin 1 -> d_ap - d_an + margin == 0 exactly
    g = torch.tensor([[0, 0, 0, 0], [3, 4, 0, 0], [6, 0, 0, 0], [0, 0, 0, 20]], dtype=torch.float32, device='cuda')
    q = (g + torch.tensor([0.0, 0.0, 7.0, 0.0], device='cuda'))[None].contiguous()
    q[0, 0] = 0.0
    lab = torch.tensor([0, 0, 1, 1], device='cuda')
    mem, ring = Mem(1, 6, 4), X.Ring(1, 6, 4, 'cuda')
    run_enqueue(ops, mem, q, g, lab, None, None, False); ring.enqueue(q, g, lab)
    o = run_fwd(ops, mem, q, g, lab, None, None, 1.0, False)
    own = check_fwd(o, ring, q, g, lab, None, None)
    assert (int(o['sel']['q_idx_p'][0, 0]), int(o['sel']['q_idx_n'][0, 0])) == (1, 2)
    assert (float(o['d']['q_d_ap'][0, 0]), float(o['d']['q_d_an'][0, 0])) == (5.0, 6.0) and float(own['q_row_loss'][0, 0]) == 0.0
    dq, dg = run_bwd(ops, o, [1.0])
    grads = check_bwd(dq, dg, ring, q, g, o, [1.0])
    assert float(dq[0].abs().max()) == 0.0
    assert_live(grads, own['L'])
    # the check discriminates: with anchor 0's hinge open (a `>=` in the derivative) dq[0] would be c ((x0 - m1) / 5 - (x0 - m2) / 6)
    opened, _ = X.gradient(ring, q, g, 1.0 + 1e-9, False, o['sel'], [1.0])
    assert float((dq[0].double() - opened[0, 0]).abs().max()) > 0.01


def test_soft_margin_does_not_overflow(ops):
    # q anchor 0: d_ap = 60, d_an = 10 -> z = +50;  q anchor 1: d_ap = 10, d_an = 61.6 -> z = -51.6;  the g anchors: z = -1.6 and 0 (an
    # anchor has only its own two terms here, so every row's z stays where the fp32 sigmoid is a normal number; the positive and the
    # negative of an anchor are not collinear with it: its two terms must not cancel)
    q = torch.tensor([[[0, 0, 0, 0], [0, 10, 10, 0]]], dtype=torch.float32, device='cuda')
    g = torch.tensor([[60, 0, 0, 0], [0, 10, 0, 0]], dtype=torch.float32, device='cuda')
    lab = torch.tensor([0, 1], device='cuda')
    mem, ring = Mem(1, 4, 4), X.Ring(1, 4, 4, 'cuda')
    run_enqueue(ops, mem, q, g, lab, None, None, False); ring.enqueue(q, g, lab)
    ref = X.reference(ring, q, g, lab, None, None, None, False)
    z = ref['q_d_ap'] - ref['q_d_an']
    assert float(z[0, 0]) == 50.0 and -52.0 < float(z[0, 1]) < -50.0
    o = run_fwd(ops, mem, q, g, lab, None, None, None, False)
    own = check_fwd(o, ring, q, g, lab, None, None)
    assert bool(torch.isfinite(o['result']).all()) and all(bool(torch.isfinite(v).all()) for v in o['d'].values()) and 12.4 < own['L'][0] < 12.9
    dq, dg = run_bwd(ops, o, [1.0])
    assert_live(check_bwd(dq, dg, ring, q, g, o, [1.0]), own['L'])
    assert float(dq[0].abs().max()) > 0 and float(dq[1].abs().max()) > 0


@pytest.mark.parametrize('normalize', [True, False])
def test_true_duplicate_as_the_only_positive_is_clamped(ops, normalize):
    # one row per identity: the only positive of q anchor i is slot i of the vis side and the other way round.  margin 1000: every hinge
    # is open, so every term carries c = 0.5 / n and a term that should vanish would show
    N, D, margin = 6, 96, 1000.0
    gen = torch.Generator().manual_seed(13)
    q = (torch.randn(1, N, D, generator=gen) + 1.0).cuda(); g = (torch.randn(N, D, generator=gen) + 1.0).cuda()
    lab = torch.arange(N, device='cuda')
    g[2] = q[0, 2]                                              # a true duplicate: d2 = 0 in both directions (bit-equal unit rows too)
    if not normalize:
        q[0, 4, 0] = 0.0; g[4] = q[0, 4]; g[4, 0] = 5e-7        # d2 = 2.5e-13 <= 1e-12 with a non-zero difference
    mem, ring = Mem(1, 9, D), X.Ring(1, 9, D, 'cuda')
    run_enqueue(ops, mem, q, g, lab, None, None, normalize); ring.enqueue(q, g, lab)
    o = run_fwd(ops, mem, q, g, lab, None, None, margin, normalize)
    own = check_fwd(o, ring, q, g, lab, None, None)
    clamp = float(torch.tensor(1e-12, dtype=torch.float32).sqrt())
    rows = (2,) if normalize else (2, 4)
    assert [float(o['d']['q_d_ap'][0, i]) for i in rows] == [clamp] * len(rows) == [float(o['d']['g_d_ap'][0, i]) for i in rows]
    dq, dg = run_bwd(ops, o, [1.0])
    assert_live(check_bwd(dq, dg, ring, q, g, o, [1.0]), own['L'])
    if not normalize:
        # an unclamped term would put c * 5e-7 / 1e-6 = 0.25 / n into column 0 of row 4: far outside check_bwd's tolerance
        assert 0.25 / N > 100 * 1e-5 * float(dq[4].abs().max())


# ---------------------------------------------------------------------------------------------------------------- 5. later enqueues
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('slots_per_row', [1, 2])
def test_backward_is_independent_of_later_enqueues(ops, slots_per_row, normalize):
    """Forward on batch 2 (batch 1 is in the memory too when M = 2 N), two more enqueues that overwrite every slot, then the backward:
    the same bits as without them."""
    P, N, D = 2, 16, 96
    M = slots_per_row * N
    runs = []
    for extra in (False, True):
        mem = Mem(P, M, D)
        for s in (1, 2):
            q, g, lab = batch(P, N, D, 30.0, s)
            run_enqueue(ops, mem, q, g, lab, None, None, normalize)
        o = run_fwd(ops, mem, q, g, lab, None, None, None, normalize)
        before = mem.rows.clone()
        if extra:
            for s in (3, 4):
                run_enqueue(ops, mem, *batch(P, N, D, 30.0, s), None, None, normalize)
            assert bool((mem.rows != before).any(dim=2).all())   # every slot of every side holds another row now
        dq, dg = run_bwd(ops, o, [1.0, -0.5])
        runs.append((dq.view(torch.int32).clone(), dg.view(torch.int32).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool((runs[0][0] != 0).any(dim=1).all())             # soft margin: every q row is an active anchor with gradient


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize('normalize', [True, False])
def test_two_runs_give_the_same_bits(ops, normalize):
    P, N, D, M, pad = X.SHAPES[2]
    runs = []
    for _ in range(2):
        mem, bits = Mem(P, M, D), []
        for s in (1, 2, 3):
            q, g, lab = batch(P, N, D, 30.0, s)
            run_enqueue(ops, mem, q, g, lab, None, None, normalize)
            o = run_fwd(ops, mem, q, g, lab, None, None, None, normalize)      # soft margin: every dx row of an active anchor is live
            dq, dg = run_bwd(ops, o, [1.0, -0.5, 0.25, 2.0])
            bits += [o[k].view(torch.int32).clone() for k in ('q_d', 'q_idx', 'g_d', 'g_idx', 'result')]
            bits += [dq.view(torch.int32).clone(), dg.view(torch.int32).clone()] + mem.bits()
        runs.append(bits)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool((runs[0][5] != 0).any(dim=1).all())              # dq of step 1


# ---------------------------------------------------------------------------------------------------------------- 7. public call
def test_public_call_and_autograd(ops):
    """The autograd boundary by value, with upstream factors that are not 1; enqueue=False; the argument errors."""
    from prcv2025reid_amd import losses, _lib
    P, N, D, M, _ = X.SHAPES[2]
    qv = torch.ones(P, N, dtype=torch.bool, device='cuda'); qv[1, 3] = False
    for margin, normalize in ((0.3, True), (None, False)):
        memory = losses.CrossBatchMemory(M, P + 1, D, 'cuda')
        mem = Mem(P, M, D)
        assert int(memory.rows_written) == 0 == int(memory.filled) and memory.cursor.tolist() == [0, 0] and not bool(memory.valid.any())
        for s in (1, 2, 3):                                     # the third batch wraps
            q, g, lab = batch(P, N, D, 30.0, s)
            qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
            L, flag, rows = losses.xbm_cross_triplet(qa, ga, lab, memory, q_valid=qv, margin=margin, normalize=normalize)
            run_enqueue(ops, mem, q, g, lab, qv, None, normalize)
            o = run_fwd(ops, mem, q, g, lab, qv, None, margin, normalize)
            assert int(memory.rows_written) == s * N and int(memory.filled) == min(M, s * N)
        assert L.shape == (P,) and flag.tolist() == [1.0] * P and set(rows) == {'q_d_ap', 'q_d_an', 'q_idx_p', 'q_idx_n', 'g_d_ap', 'g_d_an',
                                                                                'g_idx_p', 'g_idx_n', 'n_active'}
        assert all(rows[k].shape == (P, N) for k in rows if k != 'n_active') and rows['n_active'].shape == (P, 2)
        assert [torch.equal(a, b) for a, b in zip((memory.rows, memory.labels, memory.valid, memory.cursor), mem.tensors() + (mem.cursor,))] == [True] * 4
        assert torch.equal(L.detach(), o['res'][:, 0]) and torch.equal(rows['n_active'], o['res'][:, 2:])
        for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
            assert torch.equal(rows[k].long(), o['sel'][k])
        assert bool(((rows['q_idx_p'] >= 32) & (rows['q_idx_p'] < 128)).any())      # slots of the older batches (the third one sits in 128 .. 159, 0 .. 31)
        for k in ('q_d_ap', 'g_d_an'):
            assert torch.equal(rows[k], o['d'][k])
        for v in rows.values():
            v.zero_()                                           # the arrays handed out are copies: writing into them must not reach the backward
        gscale = [2.0, -0.7, 1.0, 0.25]
        (L * torch.tensor(gscale, device='cuda')).sum().backward()
        dq, dg = run_bwd(ops, o, gscale, pad=0)
        assert torch.equal(qa.grad.reshape(P * N, D), dq) and torch.equal(ga.grad, dg)
        assert float(dq.abs().max()) > 0 and float(dg.abs().max()) > 0 and float(dq[N + 3].abs().max()) == 0.0
        # enqueue=False: the memory as it stands, ring and cursor untouched; the batch is not in it, so other rows are chosen
        before = [t.clone() for t in (memory.rows, memory.labels, memory.valid, memory.cursor)]
        q4, g4, lab4 = batch(P, N, D, 30.0, 4)
        L4, _, rows4 = losses.xbm_cross_triplet(q4, g4, lab4, memory, margin=margin, normalize=normalize, enqueue=False)
        o4 = run_fwd(ops, mem, q4, g4, lab4, None, None, margin, normalize)
        assert [torch.equal(a, b) for a, b in zip(before, (memory.rows, memory.labels, memory.valid, memory.cursor))] == [True] * 4
        assert torch.equal(L4, o4['res'][:, 0]) and torch.equal(rows4['g_idx_n'].long(), o4['sel']['g_idx_n']) and float(L4.max()) > 0
        memory.reset()
        assert memory.cursor.tolist() == [0, 0] and not bool(memory.valid.any()) and int(memory.filled) == 0
    q, g, lab = batch(P, N, D, 30.0, 1)
    memory = losses.CrossBatchMemory(M, P + 1, D, 'cuda')
    with pytest.raises(ValueError, match='margin'):
        losses.xbm_cross_triplet(q, g, lab, memory, margin=-1.0)
    with pytest.raises(ValueError, match='does not fit'):
        losses.xbm_cross_triplet(q, g, lab, losses.CrossBatchMemory(N - 1, P + 1, D, 'cuda'))
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.xbm_cross_triplet(q[:, :, :8], g[:, :8], lab, memory)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.xbm_cross_triplet(q.cpu(), g.cpu(), lab.cpu(), memory)
    assert memory.cursor.tolist() == [0, 0]                      # a refused call files nothing


# ---------------------------------------------------------------------------------------------------------------- 8. model level
BASE_KEYS = {'total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt'}


def _step(model, batch_, backward=True):
    images = {m: t.cuda() for m, t in batch_['images'].items()}
    masks = {m: t.cuda() for m, t in batch_['modality_mask'].items()}
    labels = batch_['person_id'].cuda()
    out = model(images=images, texts=batch_['texts'], modality_masks=masks)
    L = model.compute_loss(out, labels)
    if backward:
        model.lora_arena.grad = None
        L['total_loss'].backward()
    return out, L, labels


def test_model_loss_with_the_xbm_term():
    from test_triplet_gpu import _tiny
    meta, state, batch_, make = _tiny()
    B = int(batch_['person_id'].shape[0])
    m0 = make(xbm_weight=0.0)
    _, L0, _ = _step(m0, batch_)
    assert set(L0) == BASE_KEYS and m0.xbm_memory is None       # off: today's dict, nothing allocated
    g0 = m0.lora_arena.grad.detach().clone()
    late = make(xbm_weight=0.5, xbm_start_epoch=3)
    late.set_epoch(1)
    _, Ll, _ = _step(late, batch_)
    assert set(Ll) == BASE_KEYS and late.xbm_memory is None     # before its first epoch: nothing launched
    model = make(xbm_weight=0.5, xbm_size=3 * B)
    keys_before = set(model.state_dict())
    ring = None
    for s in range(1, 5):
        out, L, labels = _step(model, batch_)
        assert set(L) == BASE_KEYS | {'xbm_loss', 'xbm_active_cnt'}
        want = model.ce_weight * float(L['ce_loss'].detach()) + model.contrastive_weight * float(L['sdm_loss'].detach()) + 0.5 * float(L['xbm_loss'].detach())
        assert abs(float(L['total_loss'].detach()) - want) <= 8 * U * (1 + abs(want))
        raw, fm = out['raw_modality_features'], out['feature_masks']
        mods = [m for m in raw if m != 'vis' and m in fm]
        assert 'vis' in raw and len(mods) >= 1
        q = torch.stack([raw[m].detach() for m in mods]); g = raw['vis'].detach()
        qv = torch.stack([fm[m].cuda() > 0 for m in mods]); gv = fm['vis'].cuda() > 0
        D = g.shape[1]
        if ring is None:
            ring = X.Ring(len(mods), 3 * B, D, 'cuda')
        ring.enqueue(q, g, labels, qv, gv)
        ref = X.reference(ring, q, g, labels, qv, gv, F32(0.3), True)
        n_pairs = max(1.0, sum(ref['flag']))
        want_x = sum(ref['L']) / n_pairs
        tol = 0.0
        for p in range(len(mods)):
            b = 0.0
            for side in 'qg':
                act = ref[f'{side}_idx_p'][p] >= 0
                b += float(((R.dist_bound(D, ref[f'{side}_d_ap'][p], True) + R.dist_bound(D, ref[f'{side}_d_an'][p], True)) * act).sum()) / max(1, int(act.sum()))
            tol += (4 * U * (1 + ref['L'][p]) + 0.5 * b) / n_pairs
        tol += 4 * U * (1 + want_x)                              # the sum over the pairs and the division
        got = float(L['xbm_loss'].detach())
        assert want_x > 0 and int(L['xbm_active_cnt']) == sum(ref['n_q']) + sum(ref['n_g']) > 0
        assert abs(got - want_x) <= tol, (s, got, want_x, tol)
        assert model.xbm_memory.cursor.tolist() == [(s * B) % (3 * B), s * B]
    assert float((model.lora_arena.grad - g0).abs().max()) > 0
    assert set(model.state_dict()) == keys_before                # the memory is no parameter and no buffer
    # the sides are fixed by modality name: a batch that brings another set is refused before anything is filed
    assert len(mods) >= 2
    fewer = dict(out, raw_modality_features={k: v for k, v in raw.items() if k != mods[-1]})
    with pytest.raises(ValueError, match='modalities'):
        model.compute_loss(fewer, labels)
    assert model.xbm_memory.cursor.tolist() == [(4 * B) % (3 * B), 4 * B]
    # eval() and no_grad: the memory is mined, the cursor does not move
    cur = model.xbm_memory.cursor.tolist()
    with torch.no_grad():
        _, Ln, _ = _step(model, batch_, backward=False)
    assert 'xbm_loss' in Ln and model.xbm_memory.cursor.tolist() == cur
    model.eval()
    _step(model, batch_, backward=False)
    assert model.xbm_memory.cursor.tolist() == cur
    model.reset_xbm()
    assert model.xbm_memory.cursor.tolist() == [0, 0] and not bool(model.xbm_memory.valid.any())


# ---------------------------------------------------------------------------------------------------------------- 9. graphed step
def test_graphed_step_with_the_xbm_term_matches_eager():
    """The shapes and warm-up of test_triplet_gpu.test_graphed_step_with_the_triplet_term_matches_eager, with this loss on: the cursor
    lives on the device, so the replays keep filing rows (3 B slots: the ring wraps)."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_triplet_gpu import _tiny
    meta, state, batch_, build = _tiny()
    B = int(batch_['person_id'].shape[0])
    images = {m: t.cuda() for m, t in batch_['images'].items()}
    masks = dict(batch_['modality_mask'])
    labels = batch_['person_id'].cuda()

    def make():
        m = build(xbm_weight=0.5, xbm_size=3 * B)
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
    assert a.xbm_memory.cursor.tolist() == b.xbm_memory.cursor.tolist() == [(5 * B) % (3 * B), 5 * B]
    assert float(Lb['xbm_loss'].detach()) > 0 and int(Lb['xbm_active_cnt']) == int(La['xbm_active_cnt']) > 0
    for k in ('total_loss', 'xbm_loss'):
        va, vb = float(La[k].detach()), float(Lb[k].detach())
        assert abs(va - vb) <= 2e-3 * max(1.0, abs(vb)), k
