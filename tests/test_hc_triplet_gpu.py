"""GPU: the hetero-center triplet loss kernels (csrc/hc_triplet.hip) per element against the fp64 reference (hc_triplet_ref.py), in
both library flavours, and the loss behind the public call, inside the model and in the graphed step.

Every output lives between 32 guard elements (guard rows and padding columns for dq / dg) that hold a sentinel NaN pattern and must
keep it; padded input rows carry NaN in their padding.

Bounds (u = 2^-24), derived from the operation count:
  * lead, count, the centres' labels, n_q, n_g, flag, idx_p (a centre has at most one positive) and which anchors are active: exact;
  * centres (read from ws), in norm: normalize = 1: (D / 2 + 3) u for the unit rows (section 14: the D-term sum of squares, the square
    root, one division, one product) + (c + 1) / 2 u for the c - 1 additions (the partial sums of unit rows have norm <= 2 .. c, the sum
    is divided by c) + u for the division; normalize = 0: ((c + 1) / 2 + 1) u times the largest row norm (the rows carry no error of
    their own, and centre differences cancel a common mean, so the term is absolute in the row magnitude);
  * distances: two centres move d by the sum of their bounds, the difference-form sum adds D u / 2 relative:
    normalize = 1: |d - d64| <= (D + 9 + c_max) u + (D u / 2) d;   normalize = 0: (3 + c_max) u max|x| + (D u / 2) d
    (the issue expected (D + 6 + 2 c_max) u for the first: the derivation gives c_max + 3 for the sum and the division of two centres,
    not 2 c_max; the derivation stands);
  * selection: for EVERY anchor the fp64 distance of the kernel's negative is within that bound of the fp64 minimum (no exemptions);
    on the fixtures test_hc_triplet_cpu.py asserts cleared (the first four shapes at ratio 0) the indices equal the reference's;
  * L_p: 4 u (1 + |L|) + the distance bounds of d_ap and d_an averaged over the active anchors;
  * gradients: per element against the fp64 autograd gradient at the kernel's own selection, relative to the row's largest |dx|: 1e-5,
    the project's gate;
  * two runs: identical bits.
The measured fractions of every gate are in profiles/hc_triplet_summary.md.
"""
import pytest
import torch

import hc_triplet_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 32
U = R.U
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
GRAD_GATE = 1e-5
WORST = {}
_MINED = {}                              # (shape, ratio, normalize) -> the reference's centres and selection: made once, shared by margins and flavours


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
    """([GUARD + n + GUARD] sentinel buffer of int32, its middle n elements as ``dtype``)."""
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


def run_fwd(ops, q, g, ql, gl, qv, gv, margin, normalize, pad=0):
    """The forward on q [P, N, D], g [Mg, D]; every output between guards.  Returns the outputs (flat, as the C ABI has them), the
    selection as [P, N + Mg] tensors and the per-side arrays."""
    P, N, D = q.shape
    Mg = g.shape[0]
    Rr, Uu = P * N + Mg, N + Mg
    sizes = dict(lead=Rr, count=Rr, clabel=2 * Rr, d=2 * P * Uu, idx=2 * P * Uu, result=4 * P, ws=ops.hc_triplet_ws_floats(P, N, Mg, D))
    kinds = dict(lead=torch.int32, count=torch.int32, clabel=torch.int64, d=torch.float32, idx=torch.int32, result=torch.float32, ws=torch.float32)
    bufs = {k: guarded(n, kinds[k]) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    o['q2'], o['g2'] = strided(q, pad), strided(g, pad)
    o['qv'] = None if qv is None else qv.reshape(-1).contiguous()
    ops.hc_triplet_fwd(o['q2'], o['g2'], ql, gl, o['qv'], gv, -1.0 if margin is None else margin, normalize, R.EPS, o['lead'], o['count'],
                       o['clabel'], o['d'], o['idx'], o['ws'], o['result'], P=P)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert untouched(buf, sizes[k]), f'{k}: guard elements overwritten'
        if k != 'ws':                                               # (ws holds slots behind the centre counts that nobody writes or reads)
            assert not bool((buf[GUARD:GUARD + sizes[k]] == SENTINEL32).any()), f'{k}: elements not written'
    o['sel'] = dict(idx_p=o['idx'][:P * Uu].view(P, Uu).long(), idx_n=o['idx'][P * Uu:].view(P, Uu).long())
    o['dist'] = dict(d_ap=o['d'][:P * Uu].view(P, Uu), d_an=o['d'][P * Uu:].view(P, Uu))
    o['res'] = o['result'].view(P, 4)
    o.update(P=P, N=N, Mg=Mg, D=D, gv=gv, margin=margin, normalize=normalize)
    return o


def run_bwd(ops, o, gscale, pad=4):
    """The backward from what run_fwd left; dq [P N, D] and dg [Mg, D] between guard rows and NaN-pattern padding columns."""
    outs = []
    for x in (o['q2'], o['g2']):
        rows, D = x.shape
        buf = torch.full((rows + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda').view(torch.float32)
        outs.append((buf, buf[GUARD:GUARD + rows, :D]))
    (bq, dq), (bg, dg) = outs
    ops.hc_triplet_bwd(o['q2'], o['g2'], -1.0 if o['margin'] is None else o['margin'], o['normalize'], R.EPS, o['lead'], o['count'], o['ws'],
                       o['result'], torch.tensor(gscale, dtype=torch.float32, device='cuda'), dq, dg, P=o['P'])
    torch.cuda.synchronize()
    for name, buf, dx in (('dq', bq, dq), ('dg', bg, dg)):
        raw, rows, D = buf.view(torch.int32), dx.shape[0], dx.shape[1]
        assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + rows:] == SENTINEL32).all()), f'{name}: guard rows overwritten'
        assert bool((raw[GUARD:GUARD + rows, D:] == SENTINEL32).all()), f'{name}: padding columns overwritten'
        assert bool(torch.isfinite(dx).all()), name
    return dq, dg


def mined(q, g, ql, gl, qv, gv, normalize):
    prep = R.prepare(q, g, ql, gl, qv, gv, normalize)
    return prep, R.mine(q, g, ql, gl, qv, gv, normalize, prep=prep)


def check_fwd(o, q, g, ql, gl, qv, gv, exact_index=False, mined_=None):
    """Every forward output against the reference; returns the reference evaluated at the kernel's own selection."""
    P, N, D = q.shape
    Mg = g.shape[0]
    Uu = N + Mg
    margin, normalize = o['margin'], o['normalize']
    m = F32(margin) if margin is not None else None
    prep, ref = mined_ if mined_ is not None else mined(q, g, ql, gl, qv, gv, normalize)
    ref = dict(ref)
    ref.update(R.evaluate(q, g, ref, m, normalize, ql, gl, qv, gv))
    cmax, rowmax = prep['cmax'], prep['rowmax']
    # leaders, counts, labels: exact
    PN = P * N
    assert torch.equal(o['lead'][:PN].view(P, N).long(), prep['q_lead']) and torch.equal(o['lead'][PN:].long(), prep['g_lead'])
    assert torch.equal(o['count'][:PN].view(P, N).long(), prep['q_count']) and torch.equal(o['count'][PN:].long(), prep['g_count'])
    assert torch.equal(o['clabel'][:PN].view(P, N), prep['q_label']) and torch.equal(o['clabel'][PN:], prep['g_label'])
    # centres, from ws: unit rows (P N + Mg) D, then pair p's compact block [S_q[p] q centres | S_g g centres] at p (N + Mg) D
    cen = o['ws'][(PN + Mg) * D:(PN + Mg) * D + P * Uu * D].view(P, Uu, D).double()
    for p in range(P):
        Sq, Sg = prep['S_q'][p], prep['S_g']
        for got, want, cnt in ((cen[p, :Sq], prep['cq'][p], prep['q_count'][p][:Sq]), (cen[p, Sq:Sq + Sg], prep['cg'], prep['g_count'][:Sg])):
            if want.shape[0]:
                frac = (got - want).norm(dim=1) / R.centre_bound(D, normalize, cnt.double(), rowmax)
                note(f'centre err / bound (normalize={int(normalize)})', frac.max())
                assert bool((frac <= 1).all()), (p, float(frac.max()))
    sel = o['sel']
    own = R.evaluate(q, g, sel, m, normalize, ql, gl, qv, gv)
    assert [float(v) for v in o['res'][:, 2]] == [float(v) for v in ref['n_q']] == [float(v) for v in own['n_q']]
    assert [float(v) for v in o['res'][:, 3]] == [float(v) for v in ref['n_g']] == [float(v) for v in own['n_g']]
    assert [float(v) for v in o['res'][:, 1]] == ref['flag']
    act = ref['idx_p'] >= 0
    assert torch.equal(sel['idx_p'], ref['idx_p'])                   # at most one positive: no choice to make
    assert bool(((sel['idx_n'] >= 0) == act).all()) and bool((sel['idx_n'][~act] == -1).all())
    if exact_index:
        assert torch.equal(sel['idx_n'], ref['idx_n'])
    # selection: the fp64 distance of the kernel's negative against the fp64 minimum -- every anchor
    best, mine_ = ref['d_an'], own['d_an']
    bound = R.dist_bound(D, best, normalize, cmax, rowmax)
    short = mine_ - best
    if bool(act.any()):
        note(f'selection shortfall / bound (normalize={int(normalize)})', (short / bound)[act].max())
    assert bool((short[act] >= -1e-13).all()) and bool((short[act] <= bound[act]).all()), float((short / bound)[act].max())
    # distances: the kernel's value against fp64 at its own selection
    mean_bound = torch.zeros(P, dtype=torch.float64, device=q.device)
    for k in ('d_ap', 'd_an'):
        got, want = o['dist'][k].double(), own[k]
        err, allow = (got - want).abs(), R.dist_bound(D, want, normalize, cmax, rowmax)
        if bool(act.any()):
            note(f'{k} err / bound (normalize={int(normalize)})', (err / allow)[act].max())
        assert bool((err[act] <= allow[act]).all()), (k, float((err / allow)[act].max()))
        assert bool((got[~act] == 0).all())
        mean_bound += (allow * act).sum(1) / act.sum(1).clamp(min=1)
    for p in range(P):
        tol = 4 * U * (1 + abs(own['L'][p])) + float(mean_bound[p])
        err = abs(float(o['res'][p, 0]) - own['L'][p])
        note('L err / tol', err / tol)
        assert err <= tol, (p, float(o['res'][p, 0]), own['L'][p], tol)
        if ref['flag'][p] == 0:
            assert float(o['res'][p, 0]) == 0.0
    return own


def check_bwd(dq, dg, q, g, ql, gl, qv, gv, o, gscale):
    """dq, dg against the fp64 autograd gradient at the kernel's own selection; returns it."""
    margin, normalize = o['margin'], o['normalize']
    rq, rg = R.gradient(q, g, F32(margin) if margin is not None else None, normalize, o['sel'], ql, gl, qv, gv, [F32(v) for v in gscale])
    rq = rq.reshape(-1, rq.shape[-1])
    for name, dx, ref in (('dq', dq, rq), ('dg', dg, rg)):
        rowmax = ref.abs().max(dim=1, keepdim=True).values
        err = (dx.double() - ref).abs()
        live = rowmax.flatten() > 0
        if bool(live.any()):
            note(f'dx err / row max (normalize={int(normalize)})', (err[live] / rowmax[live]).max())
        assert bool((err <= GRAD_GATE * rowmax).all()), (name, float((err / rowmax.clamp(min=1e-300)).max()))
    return rq, rg


def assert_live(grads, L):
    """The comparison that went before is not 0 against 0."""
    assert max(L) > 0 and all(float(t.abs().max()) > 0 for t in grads)


# ---------------------------------------------------------------------------------------------------------------- generated cases
CASES = [(s, r, m, n) for s in R.SHAPES for r in (0.0, 30.0) for m in (0.3, None) for n in (True, False)
         if not (s == R.SHAPES[-1] and m is None)]                  # the global batch of config 3: margin 0.3 only


@pytest.mark.parametrize('shape,ratio,margin,normalize', CASES)
def test_forward_and_backward_against_fp64(ops, shape, ratio, margin, normalize):
    P, N, Mg, D, pad = shape
    q, g, ql, gl = R.fixture(shape, ratio, 'cuda')
    key = (shape, ratio, normalize)
    if key not in _MINED:
        _MINED[key] = mined(q, g, ql, gl, None, None, normalize)
    o = run_fwd(ops, q, g, ql, gl, None, None, margin, normalize, pad)
    own = check_fwd(o, q, g, ql, gl, None, None, exact_index=(shape, ratio) in R.EXACT_INDEX, mined_=_MINED[key])
    assert sum(own['n_q']) > 0 and sum(own['n_g']) > 0
    gscale = [0.75 - 0.5 * p for p in range(P)]                 # per pair, one of them negative
    dq, dg = run_bwd(ops, o, gscale)
    grads = check_bwd(dq, dg, q, g, ql, gl, None, None, o, gscale)
    if margin is None:                                          # soft margin: every active anchor has a gradient
        assert_live(grads, own['L'])
    print(f'  {shape} ratio={ratio:g} margin={margin} normalize={normalize}: L={[round(v, 4) for v in own["L"]]}')


# ---------------------------------------------------------------------------------------------------------------- named cases
def _uneven(device='cuda'):
    """Labels interleaved and unsorted with 1 .. 5 rows per identity, in another order and with other counts on the vis side."""
    q, g, _, _ = R.make_case(2, 15, 15, 36, 30.0, seed=23, device=device)
    ql = torch.tensor([4, 2, 4, 3, 1, 4, 2, 3, 0, 4, 3, 1, 2, 4, 3], device=device)      # 0: 1, 1: 2, 2: 3, 3: 4, 4: 5 rows
    gl = torch.tensor([0, 3, 0, 1, 0, 2, 1, 0, 4, 1, 0, 2, 1, 3, 5], device=device)      # 0: 5, 1: 4, 2: 2, 3: 2, 4: 1, 5: 1 rows
    return q, g, ql, gl


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
def test_interleaved_labels_with_uneven_counts(ops, margin, normalize):
    q, g, ql, gl = _uneven()
    o = run_fwd(ops, q, g, ql, gl, None, None, margin, normalize, pad=4)
    own = check_fwd(o, q, g, ql, gl, None, None)
    assert o['lead'][:15].tolist() == [0, 1, 0, 2, 3, 0, 1, 2, 4, 0, 2, 3, 1, 0, 2] and o['count'][:15].tolist() == [5, 3, 4, 2, 1] + [0] * 10
    assert o['clabel'][30:].tolist() == [0, 3, 1, 2, 4, 5] + [0] * 9 and o['count'][30:].tolist() == [5, 2, 4, 2, 1, 1] + [0] * 9
    assert own['n_q'] == [5, 5] and own['n_g'] == [5, 5]         # identity 5 is on the vis side alone
    assert int(o['sel']['idx_p'][0, 15 + 5]) == -1 and int(o['sel']['idx_p'][0, 15 + 1]) == 2      # g centre 1 = identity 3 = q centre 2
    dq, dg = run_bwd(ops, o, [1.0, -0.5])
    grads = check_bwd(dq, dg, q, g, ql, gl, None, None, o, [1.0, -0.5])
    if margin is None:
        assert_live(grads, own['L'])
    # a row receives its centre's gradient over the count: the rows of one centre get equal gradients when normalize = 0
    if not normalize:
        assert torch.equal(dq[0], dq[2]) and torch.equal(dq[0], dq[13]) and torch.equal(dg[0], dg[10])


@pytest.mark.parametrize('normalize', [True, False])
def test_single_identity_gives_nothing(ops, normalize):
    q, g, ql, gl = R.make_case(2, 9, 7, 36, 0.0, seed=29, device='cuda')
    ql, gl = torch.zeros_like(ql), torch.zeros_like(gl)
    o = run_fwd(ops, q, g, ql, gl, None, None, None, normalize)
    own = check_fwd(o, q, g, ql, gl, None, None)
    assert own['flag'] == [0.0, 0.0] and float(o['res'].abs().max()) == 0.0 and bool((o['idx'] == -1).all()) and float(o['d'].abs().max()) == 0.0
    assert o['count'].tolist() == ([9] + [0] * 8) * 2 + [7] + [0] * 6 and bool((o['lead'] == 0).all())
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    assert float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
@pytest.mark.parametrize('kind', ['identity_invalid', 'pair_invalid', 'g_all_invalid'])
def test_validity(ops, kind, margin, normalize):
    P, N, Mg, D = 3, 16, 12, 96
    q, g, ql, gl = R.make_case(P, N, Mg, D, 30.0, seed=17, device='cuda')
    qv = torch.ones(P, N, dtype=torch.uint8, device='cuda'); gv = torch.ones(Mg, dtype=torch.uint8, device='cuda')
    if kind == 'identity_invalid':
        gv[4:8] = 0                                              # identity 1 has no valid row on the vis side: its q centres have no positive
        qv[0, 0] = 0; qv[2, 9] = 0                               # (and two single rows: the leader of identity 0 in pair 0 becomes row 1)
        q[0, 0] = float('inf')                                   # what an invalid row holds is never looked at
    elif kind == 'pair_invalid':
        qv[1] = 0
    else:
        gv[:] = 0
    o = run_fwd(ops, q, g, ql, gl, qv, gv, margin, normalize)
    if kind == 'identity_invalid':
        q[0, 0] = 0.0                                            # (the reference multiplies by the row: keep it finite there)
    own = check_fwd(o, q, g, ql, gl, qv, gv)
    gscale = [1.0, -2.0, 0.5]
    dq, dg = run_bwd(ops, o, gscale)
    grads = check_bwd(dq, dg, q, g, ql, gl, qv, gv, o, gscale)
    dq3 = dq.reshape(P, N, D)
    sel = o['sel']
    if kind == 'identity_invalid':
        assert bool((sel['idx_p'][:, 1] == -1).all()) and bool((sel['idx_n'][:, 1] == -1).all())       # q centre 1 = identity 1: inactive
        assert own['n_q'] == [2, 2, 2] and own['n_g'] == [2, 2, 2] and o['lead'][P * N:].tolist() == [0] * 4 + [-1] * 4 + [1] * 4
        assert int(o['lead'][0]) == -1 and int(o['lead'][1]) == 0 and int(o['count'][0]) == 3
        assert float(dq3[0, 0].abs().max()) == 0.0 and float(dq3[2, 9].abs().max()) == 0.0 and float(dg[4:8].abs().max()) == 0.0
        if margin is None:
            assert_live(grads, own['L'])
    elif kind == 'pair_invalid':
        assert own['flag'] == [1.0, 0.0, 1.0] and float(o['res'][1, 0]) == 0.0 and float(dq3[1].abs().max()) == 0.0
        # the other pairs are what they are without pair 1: the same bits as a run on pairs 0 and 2 alone
        keep = [0, 2]
        o2 = run_fwd(ops, q[keep], g, ql, gl, qv[keep], gv, margin, normalize)
        assert torch.equal(o2['res'].view(torch.int32), o['res'][keep].view(torch.int32))
        dq2, dg2 = run_bwd(ops, o2, [gscale[0], gscale[2]])
        assert torch.equal(dq2.reshape(2, N, D), dq3[keep]) and torch.equal(dg2, dg)
        if margin is None:
            assert_live(grads, own['L'])
    else:
        assert own['flag'] == [0.0] * 3 and float(o['res'].abs().max()) == 0.0
        assert all(bool((v == -1).all()) for v in sel.values()) and float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0


@pytest.mark.parametrize('normalize', [True, False])
def test_duplicate_centres_are_clamped_and_tie_to_the_lowest_index(ops, normalize):
    """Identity 2's rows are the same bits on both sides: its two centres coincide, so d_ap of either is the clamp value and carries no
    gradient, and every other anchor whose nearest negative is identity 2 sees an exact tie between the q-side centre (index 2) and the
    g-side centre (index N + 2): the lowest index wins.  margin 1000: every hinge is open, a term that should vanish
    would show."""
    N, D, K, margin = 12, 96, 2, 1000.0
    q, g, ql, gl = R.make_case(1, N, N, D, 0.0, seed=31, K=K, device='cuda')
    q[0, 4:6] = 0.5 * (q[0].mean(0) + g.mean(0)) + 0.05 * q[0, 4:6]      # near the middle of everything: many anchors' nearest negative
    g[4:6] = q[0, 4:6]
    prep, ref = mined(q, g, ql, gl, None, None, normalize)
    act = ref['idx_p'] >= 0
    tied = act & (ref['gap_n'] == 0)
    bound = R.dist_bound(D, R.evaluate(q, g, ref, margin, normalize, ql, gl)['d_an'], normalize, prep['cmax'], prep['rowmax'])
    assert int(tied[0, :N].sum()) >= 2 and int(tied[0, N:].sum()) >= 2 and bool((ref['idx_n'][tied] == 2).all())      # anchors of both sides
    assert bool((ref['gap_n'][act & ~tied] > 2 * bound[act & ~tied]).all())                   # the others are clear: indices must be equal
    o = run_fwd(ops, q, g, ql, gl, None, None, margin, normalize)
    own = check_fwd(o, q, g, ql, gl, None, None, exact_index=True)
    clamp = float(torch.tensor(1e-12, dtype=torch.float32).sqrt())
    assert float(o['dist']['d_ap'][0, 2]) == clamp == float(o['dist']['d_ap'][0, N + 2])
    dq, dg = run_bwd(ops, o, [1.0])
    assert_live(check_bwd(dq, dg, q, g, ql, gl, None, None, o, [1.0]), own['L'])


def test_a_row_of_zeros_gets_the_g_over_eps_gradient(ops):
    P, N, Mg, D = 2, 8, 8, 96
    q, g, ql, gl = R.make_case(P, N, Mg, D, 0.0, seed=19, device='cuda')
    q[1, 2] = 0.0                                               # |x| < eps: the unit row is 0, its centre the mean of three unit rows and it
    o = run_fwd(ops, q, g, ql, gl, None, None, None, True)     # (soft margin: the centre's anchor has a gradient whatever its distances)
    assert all(bool(torch.isfinite(o[k]).all()) for k in ('d', 'result'))
    own = check_fwd(o, q, g, ql, gl, None, None)
    assert int(o['sel']['idx_p'][1, 0]) >= 0
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    rq, _ = check_bwd(dq, dg, q, g, ql, gl, None, None, o, [1.0, 1.0])
    assert float(rq[N + 2].abs().max()) > 1e9 and float(dq[N + 2].abs().max()) > 1e9
    assert_live((dq, dg), own['L'])


@pytest.mark.parametrize('normalize', [True, False])
def test_two_runs_give_the_same_bits(ops, normalize):
    shape = R.SHAPES[3]
    q, g, ql, gl = R.fixture(shape, 30.0, 'cuda')
    runs = []
    for _ in range(2):
        o = run_fwd(ops, q, g, ql, gl, None, None, None, normalize)      # soft margin: every dx row of an active anchor is live
        dq, dg = run_bwd(ops, o, [1.0, -0.5, 0.25])
        runs.append([o[k].view(torch.int32).clone() for k in ('lead', 'count', 'clabel', 'd', 'idx', 'result')]
                    + [dq.view(torch.int32).clone(), dg.view(torch.int32).clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool((runs[0][-1].view(torch.float32).abs().max(dim=1).values > 0).all())      # dg: every vis row has a positive (N > Mg)


def test_public_call_and_autograd(ops):
    """The autograd boundary by value, with upstream factors that are not 1, and q [N, D] as P = 1."""
    from prcv2025reid_amd import losses, _lib
    shape = R.SHAPES[2]
    P, N, Mg, D, _ = shape
    q, g, ql, gl = R.fixture(shape, 30.0, 'cuda')
    qv = torch.ones(P, N, dtype=torch.bool, device='cuda'); qv[1, 3] = False
    names = {f'{s}_{k}' for s in 'qg' for k in ('lead', 'count', 'label', 'd_ap', 'd_an', 'idx_p', 'idx_n')} | {'n_active'}
    for margin, normalize in ((0.3, True), (None, False)):
        qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
        L, flag, rows = losses.hetero_center_triplet(qa, ga, ql, gl, q_valid=qv, margin=margin, normalize=normalize)
        assert L.shape == (P,) and flag.tolist() == [1.0] * P and set(rows) == names
        assert rows['q_lead'].shape == (P, N) and rows['g_count'].shape == (Mg,) and rows['q_idx_p'].shape == (P, N) \
            and rows['g_idx_n'].shape == (P, Mg) and rows['n_active'].shape == (P, 2)
        o = run_fwd(ops, q, g, ql, gl, qv.to(torch.uint8), None, margin, normalize)
        assert torch.equal(L.detach(), o['res'][:, 0]) and torch.equal(rows['n_active'], o['res'][:, 2:])
        assert torch.equal(rows['q_lead'].reshape(-1), o['lead'][:P * N]) and torch.equal(rows['g_lead'], o['lead'][P * N:])
        assert torch.equal(rows['q_count'].reshape(-1), o['count'][:P * N]) and torch.equal(rows['g_label'], o['clabel'][P * N:])
        for k in ('idx_p', 'idx_n'):
            assert torch.equal(rows[f'q_{k}'].long(), o['sel'][k][:, :N]) and torch.equal(rows[f'g_{k}'].long(), o['sel'][k][:, N:])
        assert torch.equal(rows['q_d_ap'], o['dist']['d_ap'][:, :N]) and torch.equal(rows['g_d_an'], o['dist']['d_an'][:, N:])
        for v in rows.values():
            v.zero_()                                           # the arrays handed out are copies: writing into them must not reach the backward
        gscale = [2.0, -0.7, 1.0, 0.25]
        (L * torch.tensor(gscale, device='cuda')).sum().backward()
        dq, dg = run_bwd(ops, o, gscale, pad=0)
        assert torch.equal(qa.grad.reshape(P * N, D), dq) and torch.equal(ga.grad, dg)
        assert_live(check_bwd(dq, dg, q, g, ql, gl, qv, None, o, gscale), [float(v) for v in L.detach()])
    # L.sum().backward() = the direct backward call with gscale 1; q [N, D] = P = 1
    q1 = q[2].clone().requires_grad_(True)
    g1 = g.clone().requires_grad_(True)
    L1, flag1, rows1 = losses.hetero_center_triplet(q1, g1, ql, gl)
    L1.sum().backward()
    o1 = run_fwd(ops, q[2:3], g, ql, gl, None, None, 0.3, True)
    dq1, dg1 = run_bwd(ops, o1, [1.0], pad=0)
    assert L1.shape == (1,) and torch.equal(L1.detach(), o1['res'][:, 0]) and rows1['q_idx_p'].shape == (1, N)
    assert torch.equal(q1.grad, dq1) and torch.equal(g1.grad, dg1) and float(dq1.abs().max()) > 0
    with pytest.raises(ValueError, match='margin'):
        losses.hetero_center_triplet(q, g, ql, gl, margin=-1.0)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.hetero_center_triplet(q.cpu(), g.cpu(), ql.cpu(), gl.cpu())
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.hetero_center_triplet(q[:, :, :6], g[:, :6], ql, gl)


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny():
    """(meta, state, batch, make) of the tiny model the triplet model tests use; make(strip=True) builds it from a config that does
    not have the hc_triplet_* fields at all."""
    from helpers import load_case, case_inputs, case_config
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    z, meta = load_case('tiny_train_frozen')
    cfg0, arch, state, batch, tokens = case_inputs(meta)

    def make(strip=False, **over):
        cfg = case_config(meta, device='cuda')
        cfg.compute_dtype = 'bf16'
        for k, v in over.items():
            setattr(cfg, k, v)
        if strip:
            import types
            cfg = types.SimpleNamespace(**{k: v for k, v in vars(cfg).items() if not k.startswith('hc_triplet_')})
        model = CLIPBasedMultiModalReIDModel(cfg)
        model.set_num_classes(int(meta['num_classes']))
        model.load_state_dict(state, strict=True)
        apply_reference_freeze(model)
        model.contrastive_weight = meta['contrastive_weight']
        model.set_epoch(2)
        model.train(True)
        return model
    return meta, state, batch, make


def _loss_and_grad(model, batch, key='total_loss'):
    """(outputs, loss dict, labels, the adapters' gradient of loss dict entry ``key``) of one training forward."""
    images = {m: t.cuda() for m, t in batch['images'].items()}
    masks = {m: t.cuda() for m, t in batch['modality_mask'].items()}
    labels = batch['person_id'].cuda()
    out = model(images=images, texts=batch['texts'], modality_masks=masks)
    L = model.compute_loss(out, labels)
    L[key].backward()
    return out, L, labels, model.lora_arena.grad.detach().clone()


def test_model_loss_with_the_hc_triplet_term():
    from prcv2025reid_amd.model import LazyCount
    meta, state, batch, make = _tiny()
    base_keys = {'total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt'}
    _, L_old, _, _ = _loss_and_grad(make(strip=True), batch)        # a config object without the new fields still works
    _, L0, _, _ = _loss_and_grad(make(hc_triplet_weight=0.0), batch)
    # weight 0: the keys and every value are what a model built without the new fields returns, bit for bit
    assert set(L0) == set(L_old) == base_keys
    for k in base_keys:
        a, b = L0[k], L_old[k]
        assert (int(a) == int(b)) if isinstance(a, LazyCount) else torch.equal(a, b), k
    model = make(hc_triplet_weight=0.3)
    out, L, labels, g_hc = _loss_and_grad(model, batch, 'hc_triplet_loss')      # the gradient of this loss alone
    assert set(L) == base_keys | {'hc_triplet_loss', 'hc_triplet_active_cnt'}
    for k in ('ce_loss', 'sdm_loss'):
        assert torch.equal(L[k], L0[k]), k
    want = float(L0['total_loss'].detach()) + F32(0.3) * float(L['hc_triplet_loss'].detach())
    assert abs(float(L['total_loss'].detach()) - want) <= 4 * U * (1 + abs(want))                 # two fp32 roundings
    # the reference on raw_modality_features, every non-vis modality with a mask against vis
    raw, fm = out['raw_modality_features'], out['feature_masks']
    mods = [m for m in raw if m != 'vis' and m in fm]
    assert 'vis' in raw and len(mods) >= 1
    q = torch.stack([raw[m].detach() for m in mods]); g = raw['vis'].detach()
    qv = torch.stack([fm[m].cuda() > 0 for m in mods]); gv = fm['vis'].cuda() > 0
    ref = R.reference(q, g, labels, labels, qv, gv, F32(0.3), True)
    D = g.shape[1]
    n_pairs = max(1.0, sum(ref['flag']))
    want_hc = sum(ref['L']) / n_pairs
    tol = 0.0
    for p in range(len(mods)):
        act = ref['idx_p'][p] >= 0
        b = sum(float((R.dist_bound(D, ref[k][p], True, ref['cmax'], ref['rowmax']) * act).sum()) for k in ('d_ap', 'd_an')) / max(1, int(act.sum()))
        tol += (4 * U * (1 + ref['L'][p]) + b) / n_pairs
    tol += 4 * U * (1 + want_hc)                                                          # the sum over the pairs and the division
    assert sum(ref['flag']) >= 1 and want_hc > 0
    assert int(L['hc_triplet_active_cnt']) == sum(ref['n_q']) + sum(ref['n_g']) > 0
    got_hc = float(L['hc_triplet_loss'].detach())
    assert abs(got_hc - want_hc) <= tol, (got_hc, want_hc, tol)
    # the gradient reaches lora_B of vis and of a non-vis modality
    from prcv2025reid_amd.weights import param_spec
    for m in ('vis', [m for m in mods if m in model.vision_modalities][0]):
        keys = [k for k in param_spec(model.arch, None) if f'.loras.{m}.lora_B.' in k]
        assert keys and max(float(model.layout.ref_view(g_hc, k).abs().max()) for k in keys) > 0, m


def test_graphed_step_with_the_hc_triplet_term_matches_eager():
    """The shapes and warm-up of test_triplet_gpu.test_graphed_step_with_the_triplet_term_matches_eager, with this loss on."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    meta, state, batch, build = _tiny()
    images = {m: t.cuda() for m, t in batch['images'].items()}
    masks = dict(batch['modality_mask'])
    labels = batch['person_id'].cuda()

    def make():
        m = build(hc_triplet_weight=0.3)
        gs = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in m.get_learnable_params()]
        return m, StepDriver(m, FusedAdamW(gs, weight_decay=1e-4))

    a, da = make()
    tok = a.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
    tok = {k: v.cuda() for k, v in tok.items()}
    g = GraphedStep(da, images, tok, masks, labels, warmup=2)
    for _ in range(3):
        La = g.step(images, tok, masks, labels)
    torch.cuda.synchronize()
    b, db = make()
    for _ in range(5):
        Lb = db.step(images, tok, masks, labels)
    assert da.opt.step_count == db.opt.step_count == 5
    assert float(Lb['hc_triplet_loss'].detach()) > 0 and int(Lb['hc_triplet_active_cnt']) == int(La['hc_triplet_active_cnt']) > 0
    for k in ('total_loss', 'hc_triplet_loss'):
        a, b = float(La[k].detach()), float(Lb[k].detach())
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), k
