"""GPU: the cross-modal batch-hard triplet loss kernels (csrc/cross_triplet.hip) per element against the fp64 reference
(cross_triplet_ref.py), in both library flavours, and the loss behind the public call, inside the model and in the graphed step.

Every output lives between 32 guard elements (guard rows and padding columns for dq / dg) that hold a sentinel NaN pattern and must
keep it; padded input rows carry NaN in their padding.

Bounds (u = 2^-24):
  * distances, normalize = 0: relative D u / 2 (a D-term sum of non-negative fp32 terms, the square root halves it);
  * distances, normalize = 1: |d - d64| <= (D + 6) u + (D u / 2) d -- each unit-row element is within (D / 2 + 3) u relative (the
    D-term sum of squares, the square root, one division, one product), two such rows move d by at most twice that, the
    difference-form sum adds D u / 2 relative;
  * selection: for EVERY anchor the fp64 distance of the kernel's choice is within that bound of the fp64 extreme (no exemptions); on
    the fixtures test_cross_triplet_cpu.py has cleared (the first four shapes at ratio 0) the indices equal the reference's;
  * n_qg, n_gq, flag: exact;  L_p: 4 u (1 + |L|) + the distance bound averaged over the active anchors of both directions;
  * gradients: per element against the fp64 gradient evaluated at the kernel's own selection, relative to the row's largest |dx|:
    1e-5 for normalize = 0 (the project's gate), GATE_NORM for normalize = 1 (the projection adds a D-term dot product).

GATE_NORM = twice the worst case measured over all cases of this file, rounded up to one significant digit.  Measured on an MI355X
(both flavours give the same bits, the kernels are fp32): normalize = 1: 3.43e-6 of the row maximum -> GATE_NORM = 7e-6;
normalize = 0: 4.79e-6 (gate 1e-5).  Distances: at most 0.018 of their bound with normalize = 1 and 0.24 with normalize = 0 (the two
distances an anchor keeps are re-evaluated with an fp64 sum: half an ulp of d plus the rounding of d2); L_p: 0.012 of its tolerance;
profiles/cross_triplet_summary.md.
"""
import pytest
import torch

import cross_triplet_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 32
U = R.U
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
# normalize -> gate on |dx - dx64| / row maximum.  True: twice the worst case measured over every case of this file (3.43e-6), rounded
# up to one significant digit
GRAD_GATE = {False: 1e-5, True: 7e-6}
WORST = {}
_MINED = {}                              # (shape, ratio, normalize) -> the reference's selection: mined once, shared by margins and flavours


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
    """([GUARD + n + GUARD] sentinel buffer, its middle n elements)."""
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
    """The forward on q [P, N, D], g [Mg, D]; every output between guards.  Returns the outputs (flat, as the C ABI has them) and the
    selection as [P, n] tensors."""
    P, N, D = q.shape
    Mg = g.shape[0]
    sizes = dict(q_d=2 * P * N, q_idx=2 * P * N, g_d=2 * P * Mg, g_idx=2 * P * Mg, result=4 * P, ws=ops.cross_triplet_ws_floats(P, N, Mg, D))
    bufs = {k: guarded(n, torch.int32 if k.endswith('idx') else torch.float32) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    o['q2'], o['g2'] = strided(q, pad), strided(g, pad)
    o['qv'] = None if qv is None else qv.reshape(-1).contiguous()
    ops.cross_triplet_fwd(o['q2'], o['g2'], ql, gl, o['qv'], gv, -1.0 if margin is None else margin, normalize, R.EPS, o['q_d'], o['q_idx'],
                          o['g_d'], o['g_idx'], o['ws'], o['result'], P=P)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert untouched(buf, view.numel()), f'{k}: guard elements overwritten'
        if k != 'ws':                                               # (normalize = 0 leaves the unit-row part of ws alone)
            assert not bool((view.view(torch.int32) == SENTINEL32).any()), f'{k}: elements not written'
    o['sel'] = dict(q_idx_p=o['q_idx'][:P * N].view(P, N).long(), q_idx_n=o['q_idx'][P * N:].view(P, N).long(),
                    g_idx_p=o['g_idx'][:P * Mg].view(P, Mg).long(), g_idx_n=o['g_idx'][P * Mg:].view(P, Mg).long())
    o['d'] = dict(q_d_ap=o['q_d'][:P * N].view(P, N), q_d_an=o['q_d'][P * N:].view(P, N),
                  g_d_ap=o['g_d'][:P * Mg].view(P, Mg), g_d_an=o['g_d'][P * Mg:].view(P, Mg))
    o['res'] = o['result'].view(P, 4)
    o.update(P=P, gv=gv, margin=margin, normalize=normalize)
    return o


def run_bwd(ops, o, gscale, pad=4):
    """The backward from what run_fwd left; dq [P N, D] and dg [Mg, D] between guard rows and NaN-pattern padding columns."""
    outs = []
    for x in (o['q2'], o['g2']):
        rows, D = x.shape
        buf = torch.full((rows + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda').view(torch.float32)
        outs.append((buf, buf[GUARD:GUARD + rows, :D]))
    (bq, dq), (bg, dg) = outs
    ops.cross_triplet_bwd(o['q2'], o['g2'], o['qv'], o['gv'], -1.0 if o['margin'] is None else o['margin'], o['normalize'], R.EPS, o['q_d'],
                          o['q_idx'], o['g_d'], o['g_idx'], o['ws'], o['result'], torch.tensor(gscale, dtype=torch.float32, device='cuda'),
                          dq, dg, P=o['P'])
    torch.cuda.synchronize()
    for name, buf, dx in (('dq', bq, dq), ('dg', bg, dg)):
        raw, rows, D = buf.view(torch.int32), dx.shape[0], dx.shape[1]
        assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + rows:] == SENTINEL32).all()), f'{name}: guard rows overwritten'
        assert bool((raw[GUARD:GUARD + rows, D:] == SENTINEL32).all()), f'{name}: padding columns overwritten'
        assert bool(torch.isfinite(dx).all()), name
    return dq, dg


def check_fwd(o, q, g, ql, gl, qv, gv, exact_index=False, mined=None):
    """Every forward output against the reference (``mined``: its selection, when the caller keeps one); returns the reference at the
    kernel's own selection."""
    P, N, D = q.shape
    margin, normalize = o['margin'], o['normalize']
    m = F32(margin) if margin is not None else None
    ref = dict(mined if mined is not None else R.mine(q, g, ql, gl, qv, gv, normalize))
    ref.update(R.evaluate(q, g, ref, m, normalize))
    sel = o['sel']
    own = R.evaluate(q, g, sel, m, normalize)
    assert [float(v) for v in o['res'][:, 2]] == ref['n_qg'] == own['n_qg'] and [float(v) for v in o['res'][:, 3]] == ref['n_gq'] == own['n_gq']
    assert [float(v) for v in o['res'][:, 1]] == ref['flag']
    tol_L = []
    for s in 'qg':
        ip, inn = sel[f'{s}_idx_p'], sel[f'{s}_idx_n']
        act = ref[f'{s}_idx_p'] >= 0
        assert bool(((ip >= 0) == act).all()) and bool(((inn >= 0) == act).all())
        assert bool((ip[~act] == -1).all()) and bool((inn[~act] == -1).all())
        if exact_index:
            assert torch.equal(ip, ref[f'{s}_idx_p']) and torch.equal(inn, ref[f'{s}_idx_n']), s
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
        tol_L.append(mean_bound)
    for p in range(P):
        tol = 4 * U * (1 + abs(own['L'][p])) + 0.5 * float(tol_L[0][p] + tol_L[1][p])
        err = abs(float(o['res'][p, 0]) - own['L'][p])
        note('L err / tol', err / tol)
        assert err <= tol, (p, float(o['res'][p, 0]), own['L'][p], tol)
        if ref['flag'][p] == 0:
            assert float(o['res'][p, 0]) == 0.0
    return own


def check_bwd(dq, dg, q, g, o, gscale):
    """dq, dg against the fp64 gradient at the kernel's own selection; returns it."""
    margin, normalize = o['margin'], o['normalize']
    rq, rg = R.gradient(q, g, F32(margin) if margin is not None else None, normalize, o['sel'], [F32(v) for v in gscale])
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


# ---------------------------------------------------------------------------------------------------------------- generated cases
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
@pytest.mark.parametrize('ratio', [0.0, 30.0])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_forward_and_backward_against_fp64(ops, shape, ratio, margin, normalize):
    P, N, Mg, D, pad = shape
    q, g, ql, gl = R.fixture(shape, ratio, 'cuda')
    key = (shape, ratio, normalize)
    if key not in _MINED:
        _MINED[key] = R.mine(q, g, ql, gl, None, None, normalize)
    o = run_fwd(ops, q, g, ql, gl, None, None, margin, normalize, pad)
    own = check_fwd(o, q, g, ql, gl, None, None, exact_index=(shape, ratio) in R.EXACT_INDEX, mined=_MINED[key])
    gscale = [0.75 - 0.5 * p for p in range(P)]                 # per pair, one of them negative
    dq, dg = run_bwd(ops, o, gscale)
    grads = check_bwd(dq, dg, q, g, o, gscale)
    if N == 1:
        assert own['flag'] == [0.0] and float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0
    elif margin is None or normalize:                          # soft margin, or unit rows (d < 2, the hinge at 0.3 is mostly open)
        assert_live(grads, own['L'])
    print(f'  {shape} ratio={ratio:g} margin={margin} normalize={normalize}: L={[round(v, 4) for v in own["L"]]} worst so far {WORST}')


# ---------------------------------------------------------------------------------------------------------------- named cases
def _tie_case(normalize):
    """Exact ties for one anchor of either direction: duplicated rows 70 apart (two waves of one 256-row candidate piece) and 300 apart
    (two candidate pieces)."""
    q, g, ql, gl = R.make_case(2, 360, 360, 96, 30.0, seed=9, device='cuda')
    ql, gl = ql.clone(), gl.clone()
    # (the far rows sit 5 sigma out in a random direction, not further: an outlier row's own two gradient terms are nearly parallel
    # unit vectors, and their difference must stay well conditioned for the per-element check of the gradient)
    v = 5.0 * torch.sign(torch.randn(96, generator=torch.Generator().manual_seed(3))).cuda()
    # (and the near rows a third of the typical distance away, not next to the anchor: the difference of two fp32 UNIT rows that nearly
    # coincide has few significant bits left, whatever the kernel does -- test_near_duplicate_... looks at that case's distance)
    w = 0.5 * torch.sign(torch.randn(96, generator=torch.Generator().manual_seed(4))).cuda()
    # q -> g, anchor q[0, 0] (identity 0): tied farthest positives in two pieces, tied nearest negatives in two waves
    gl[44] = 0; gl[344] = 0
    g[44] = q[0, 0] + v; g[344] = g[44]
    g[10] = q[0, 0] + w; g[80] = g[10]
    # g -> q, anchor g[5] (identity 1) against pair 1: the other way round
    ql[11] = 1; ql[81] = 1
    q[1, 11] = g[5] - v; q[1, 81] = q[1, 11]
    q[1, 45] = g[5] + w; q[1, 345] = q[1, 45]
    return q, g, ql, gl


@pytest.mark.parametrize('normalize', [True, False])
def test_exact_ties_go_to_the_lowest_index_in_both_directions(ops, normalize):
    q, g, ql, gl = _tie_case(normalize)
    ref = R.reference(q, g, ql, gl, None, None, F32(0.3), normalize)
    assert (int(ref['q_idx_p'][0, 0]), int(ref['q_idx_n'][0, 0])) == (44, 10) and float(ref['q_gap_p'][0, 0]) == 0.0 == float(ref['q_gap_n'][0, 0])
    assert (int(ref['g_idx_p'][1, 5]), int(ref['g_idx_n'][1, 5])) == (11, 45) and float(ref['g_gap_p'][1, 5]) == 0.0 == float(ref['g_gap_n'][1, 5])
    o = run_fwd(ops, q, g, ql, gl, None, None, 0.3, normalize)
    assert (int(o['sel']['q_idx_p'][0, 0]), int(o['sel']['q_idx_n'][0, 0])) == (44, 10)
    assert (int(o['sel']['g_idx_p'][1, 5]), int(o['sel']['g_idx_n'][1, 5])) == (11, 45)
    own = check_fwd(o, q, g, ql, gl, None, None)
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    assert_live(check_bwd(dq, dg, q, g, o, [1.0, 1.0]), own['L'])


@pytest.mark.parametrize('normalize,ratio', [(False, 30.0), (True, 0.0)])
def test_near_duplicate_cross_modal_negative_keeps_the_distance_bound(ops, normalize, ratio):
    P, N, Mg, D = 2, 64, 64, 512
    q, g, ql, gl = R.make_case(P, N, Mg, D, ratio, seed=11, device='cuda')
    g[7] = q[0, 0] + 1e-3 * torch.randn(D, generator=torch.Generator().manual_seed(5)).cuda()      # g row 7 (identity 1) 1e-3 sigma from q[0, 0] (identity 0)
    ref = R.reference(q, g, ql, gl, None, None, F32(0.3), normalize)
    assert int(ref['q_idx_n'][0, 0]) == 7 and int(ref['g_idx_n'][0, 7]) == 0
    assert float(ref['q_d_an'][0, 0]) < 2e-3 * float(ref['q_d_ap'][0, 0])
    o = run_fwd(ops, q, g, ql, gl, None, None, 0.3, normalize)
    check_fwd(o, q, g, ql, gl, None, None)
    assert int(o['sel']['q_idx_n'][0, 0]) == 7 and int(o['sel']['g_idx_n'][0, 7]) == 0
    d64 = float(ref['q_d_an'][0, 0])
    err = abs(float(o['d']['q_d_an'][0, 0]) - d64)
    print(f'  near-duplicate d_an = {d64:.3e}: error {err:.2e} (bound {float(R.dist_bound(D, torch.tensor(d64), normalize)):.2e})')
    assert err <= float(R.dist_bound(D, torch.tensor(d64), normalize))
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    if not normalize:
        # (between UNIT rows the term (x^_i - x^_a) / d of such a pair is ill-conditioned in fp32 itself: the elements of a unit row
        # carry 2^-24 * 0.04 of rounding, the difference is 3e-5 per element -- 1e-4 of it, before any arithmetic of the kernel)
        check_bwd(dq, dg, q, g, o, [1.0, 1.0])


@pytest.mark.parametrize('normalize', [True, False])
def test_true_duplicate_as_the_only_positive_is_clamped(ops, normalize):
    # one row per identity and side: every anchor has exactly one positive.  margin 1000: every hinge is open, so every term carries
    # c = 0.5 / n and a term that should vanish would show
    N, D, margin = 6, 96, 1000.0
    gen = torch.Generator().manual_seed(13)
    q = (torch.randn(1, N, D, generator=gen) + 1.0).cuda(); g = (torch.randn(N, D, generator=gen) + 1.0).cuda()
    ql = gl = torch.arange(N, device='cuda')
    g[2] = q[0, 2]                                              # a true duplicate: d2 = 0 in both directions (bit-equal unit rows too)
    if not normalize:
        q[0, 4, 0] = 0.0; g[4] = q[0, 4]; g[4, 0] = 5e-7        # d2 = 2.5e-13 <= 1e-12 with a non-zero difference
    o = run_fwd(ops, q, g, ql, gl, None, None, margin, normalize)
    own = check_fwd(o, q, g, ql, gl, None, None, exact_index=True)
    clamp = float(torch.tensor(1e-12, dtype=torch.float32).sqrt())
    rows = (2,) if normalize else (2, 4)
    assert [float(o['d']['q_d_ap'][0, i]) for i in rows] == [clamp] * len(rows) == [float(o['d']['g_d_ap'][0, i]) for i in rows]
    dq, dg = run_bwd(ops, o, [1.0])
    assert_live(check_bwd(dq, dg, q, g, o, [1.0]), own['L'])
    if not normalize:
        # an unclamped term would put c * 5e-7 / 1e-6 = 0.25 / n into column 0 of row 4: far outside check_bwd's tolerance
        assert 0.25 / N > 100 * 1e-5 * float(dq[4].abs().max())


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
@pytest.mark.parametrize('kind', ['some_invalid', 'pair_invalid', 'g_all_invalid'])
def test_validity(ops, kind, margin, normalize):
    P, N, Mg, D = 3, 15, 11, 96
    q, g, ql, gl = R.make_case(P, N, Mg, D, 30.0, seed=17, device='cuda')
    qv = torch.ones(P, N, dtype=torch.uint8, device='cuda'); gv = torch.ones(Mg, dtype=torch.uint8, device='cuda')
    if kind == 'some_invalid':
        qv[0, 1] = 0; qv[2, 5] = 0; gv[6] = 0
        q[0, 1] = float('inf')                                   # what an invalid row holds is never looked at
    elif kind == 'pair_invalid':
        qv[1] = 0
    else:
        gv[:] = 0
    o = run_fwd(ops, q, g, ql, gl, qv, gv, margin, normalize)
    own = check_fwd(o, q, g, ql, gl, qv, gv)
    gscale = [1.0, -2.0, 0.5]
    dq, dg = run_bwd(ops, o, gscale)
    if kind == 'some_invalid':
        q[0, 1] = 0.0                                            # (the reference multiplies by the row: keep it finite there)
    grads = check_bwd(dq, dg, q, g, o, gscale)
    dq3 = dq.reshape(P, N, D)
    sel = o['sel']
    if kind == 'some_invalid':
        assert_live(grads, own['L'])
        assert int(sel['q_idx_p'][0, 1]) == -1 and int(sel['q_idx_p'][2, 5]) == -1 and bool((sel['g_idx_p'][:, 6] == -1).all())
        assert 6 not in sel['q_idx_p'].flatten().tolist() + sel['q_idx_n'].flatten().tolist()       # an invalid row is never chosen
        assert 1 not in sel['g_idx_p'][0].tolist() + sel['g_idx_n'][0].tolist() and 5 not in sel['g_idx_p'][2].tolist() + sel['g_idx_n'][2].tolist()
        assert float(dq3[0, 1].abs().max()) == 0.0 and float(dq3[2, 5].abs().max()) == 0.0 and float(dg[6].abs().max()) == 0.0
    elif kind == 'pair_invalid':
        assert own['flag'] == [1.0, 0.0, 1.0] and float(o['res'][1, 0]) == 0.0 and float(dq3[1].abs().max()) == 0.0
        # the other pairs are what they are without pair 1: the same bits as a run on pairs 0 and 2 alone
        keep = [0, 2]
        o2 = run_fwd(ops, q[keep], g, ql, gl, qv[keep], gv, margin, normalize)
        assert torch.equal(o2['res'].view(torch.int32), o['res'][keep].view(torch.int32))
        dq2, dg2 = run_bwd(ops, o2, [gscale[0], gscale[2]])
        assert torch.equal(dq2.reshape(2, N, D), dq3[keep]) and torch.equal(dg2, dg)
        assert_live(grads, own['L'])
    else:
        assert own['flag'] == [0.0] * 3 and float(o['res'].abs().max()) == 0.0
        assert all(bool((v == -1).all()) for v in sel.values()) and float(dq.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0


def test_a_row_of_zeros_gets_the_g_over_eps_gradient(ops):
    P, N, Mg, D = 2, 8, 8, 96
    q, g, ql, gl = R.make_case(P, N, Mg, D, 0.0, seed=19, device='cuda')
    q[1, 2] = 0.0                                               # |x| < eps: the unit row is 0, at distance 1 from every g row
    o = run_fwd(ops, q, g, ql, gl, None, None, 0.3, True)
    assert all(bool(torch.isfinite(o[k]).all()) for k in ('q_d', 'g_d', 'result'))
    own = check_fwd(o, q, g, ql, gl, None, None)
    assert int(o['sel']['q_idx_p'][1, 2]) >= 0 and abs(float(o['d']['q_d_ap'][1, 2]) - 1.0) < 1e-5
    dq, dg = run_bwd(ops, o, [1.0, 1.0])
    rq, _ = check_bwd(dq, dg, q, g, o, [1.0, 1.0])             # (the reference's row is G / eps: test_cross_triplet_cpu.py)
    assert float(rq[N + 2].abs().max()) > 1e9 and float(dq[N + 2].abs().max()) > 1e9
    assert_live((dq, dg), own['L'])


def test_soft_margin_does_not_overflow(ops):
    # q anchor 0: d_ap = 60, d_an = 10 -> z = +50;  q anchor 1: d_ap = 10, d_an = 60 -> z = -50;  the g anchors: z = -443.6 and -490.1
    # (fp32 sigmoid underflows there; every row's largest term has z = +-50.  The positive and the negative of an anchor are not collinear
    # with it: its two terms must not cancel)
    q = torch.tensor([[[0, 0, 0, 0], [0, 0, 0, 500]]], dtype=torch.float32, device='cuda')
    g = torch.tensor([[60, 0, 0, 0], [0, 10, 0, 0], [0, 0, 10, 500], [0, 0, 0, 560]], dtype=torch.float32, device='cuda')
    ql, gl = torch.tensor([0, 2], device='cuda'), torch.tensor([0, 1, 2, 3], device='cuda')
    ref = R.reference(q, g, ql, gl, None, None, None, False)
    assert (ref['q_d_ap'] - ref['q_d_an']).tolist() == [[50.0, -50.0]] and ref['n_gq'] == [2]
    o = run_fwd(ops, q, g, ql, gl, None, None, None, False)
    own = check_fwd(o, q, g, ql, gl, None, None, exact_index=True)
    assert bool(torch.isfinite(o['result']).all()) and 12.4 < own["L"][0] < 12.6
    dq, dg = run_bwd(ops, o, [1.0])
    assert_live(check_bwd(dq, dg, q, g, o, [1.0]), own['L'])


@pytest.mark.parametrize('normalize', [True, False])
def test_two_runs_give_the_same_bits(ops, normalize):
    shape = R.SHAPES[4]
    q, g, ql, gl = R.fixture(shape, 30.0, 'cuda')
    runs = []
    for _ in range(2):
        o = run_fwd(ops, q, g, ql, gl, None, None, None, normalize)      # soft margin: every dx row of an active anchor is live
        dq, dg = run_bwd(ops, o, [1.0, -0.5])
        runs.append([o[k].view(torch.int32).clone() for k in ('q_d', 'q_idx', 'g_d', 'g_idx', 'result')] + [dq.view(torch.int32).clone(), dg.view(torch.int32).clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool((runs[0][-2].view(torch.float32).abs().max(dim=1).values > 0).all())      # dq (every q row has a positive; g rows 260.. have none)


def test_public_call_and_autograd(ops):
    """The autograd boundary by value, with upstream factors that are not 1, and q [N, D] as P = 1."""
    from prcv2025reid_amd import losses, _lib
    shape = R.SHAPES[3]
    P, N, Mg, D, _ = shape
    q, g, ql, gl = R.fixture(shape, 30.0, 'cuda')
    qv = torch.ones(P, N, dtype=torch.bool, device='cuda'); qv[1, 3] = False
    for margin, normalize in ((0.3, True), (None, False)):
        qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
        L, flag, rows = losses.cross_modal_triplet(qa, ga, ql, gl, q_valid=qv, margin=margin, normalize=normalize)
        assert L.shape == (P,) and flag.tolist() == [1.0] * P and set(rows) == {'q_d_ap', 'q_d_an', 'q_idx_p', 'q_idx_n', 'g_d_ap', 'g_d_an',
                                                                                'g_idx_p', 'g_idx_n', 'n_active'}
        assert rows['q_idx_p'].shape == (P, N) and rows['g_idx_n'].shape == (P, Mg) and rows['n_active'].shape == (P, 2)
        o = run_fwd(ops, q, g, ql, gl, qv.to(torch.uint8), None, margin, normalize)
        assert torch.equal(L.detach(), o['res'][:, 0]) and torch.equal(rows['n_active'], o['res'][:, 2:])
        for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
            assert torch.equal(rows[k].long(), o['sel'][k])
        for k in ('q_d_ap', 'g_d_an'):
            assert torch.equal(rows[k], o['d'][k])
        for v in rows.values():
            v.zero_()                                           # the arrays handed out are copies: writing into them must not reach the backward
        gscale = [2.0, -0.7, 1.0, 0.25]
        (L * torch.tensor(gscale, device='cuda')).sum().backward()
        dq, dg = run_bwd(ops, o, gscale, pad=0)
        assert torch.equal(qa.grad.reshape(P * N, D), dq) and torch.equal(ga.grad, dg)
        assert_live(check_bwd(dq, dg, q, g, o, gscale), [float(v) for v in L.detach()])
    # L.sum().backward() = the direct backward call with gscale 1; q [N, D] = P = 1
    q1 = q[2].clone().requires_grad_(True)
    g1 = g.clone().requires_grad_(True)
    L1, flag1, rows1 = losses.cross_modal_triplet(q1, g1, ql, gl)
    L1.sum().backward()
    o1 = run_fwd(ops, q[2:3], g, ql, gl, None, None, 0.3, True)
    dq1, dg1 = run_bwd(ops, o1, [1.0], pad=0)
    assert L1.shape == (1,) and torch.equal(L1.detach(), o1['res'][:, 0]) and rows1['q_idx_p'].shape == (1, N)
    assert torch.equal(q1.grad, dq1) and torch.equal(g1.grad, dg1) and float(dq1.abs().max()) > 0
    with pytest.raises(ValueError, match='margin'):
        losses.cross_modal_triplet(q, g, ql, gl, margin=-1.0)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.cross_modal_triplet(q.cpu(), g.cpu(), ql.cpu(), gl.cpu())
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.cross_modal_triplet(q[:, :, :6], g[:, :6], ql, gl)


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny():
    """(meta, state, batch, make) of the tiny model the triplet model test uses; make(strip=True) builds it from a config that does
    not have the cross_triplet_* fields at all."""
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
            cfg = types.SimpleNamespace(**{k: v for k, v in vars(cfg).items() if not k.startswith('cross_triplet_')})
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


def test_model_loss_with_the_cross_triplet_term():
    from prcv2025reid_amd.model import LazyCount
    meta, state, batch, make = _tiny()
    base_keys = {'total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt'}
    _, L_old, _, _ = _loss_and_grad(make(strip=True), batch)
    _, L0, _, _ = _loss_and_grad(make(cross_triplet_weight=0.0), batch)
    # weight 0: the keys and every value are what a model built without the new fields returns, bit for bit
    assert set(L0) == set(L_old) == base_keys
    for k in base_keys:
        a, b = L0[k], L_old[k]
        assert (int(a) == int(b)) if isinstance(a, LazyCount) else torch.equal(a, b), k
    model = make(cross_triplet_weight=0.5)
    out, L, labels, g_xt = _loss_and_grad(model, batch, 'cross_triplet_loss')      # the gradient of this loss alone
    assert set(L) == base_keys | {'cross_triplet_loss', 'cross_triplet_active_cnt'}
    for k in ('ce_loss', 'sdm_loss'):
        assert torch.equal(L[k], L0[k]), k
    want = float(L0['total_loss'].detach()) + 0.5 * float(L['cross_triplet_loss'].detach())
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
    want_xt = sum(ref['L']) / n_pairs
    tol = 0.0
    for p in range(len(mods)):
        b = 0.0
        for s in 'qg':
            act = ref[f'{s}_idx_p'][p] >= 0
            b += float(((R.dist_bound(D, ref[f'{s}_d_ap'][p], True) + R.dist_bound(D, ref[f'{s}_d_an'][p], True)) * act).sum()) / max(1, int(act.sum()))
        tol += (4 * U * (1 + ref['L'][p]) + 0.5 * b) / n_pairs
    tol += 4 * U * (1 + want_xt)                                                          # the sum over the pairs and the division
    assert sum(ref['flag']) >= 1 and want_xt > 0
    assert int(L['cross_triplet_active_cnt']) == sum(ref['n_qg']) + sum(ref['n_gq']) > 0
    got_xt = float(L['cross_triplet_loss'].detach())
    assert abs(got_xt - want_xt) <= tol, (got_xt, want_xt, tol)
    # the gradient reaches lora_B of vis and of a non-vis modality
    from prcv2025reid_amd.weights import param_spec
    for m in ('vis', [m for m in mods if m in model.vision_modalities][0]):
        keys = [k for k in param_spec(model.arch, None) if f'.loras.{m}.lora_B.' in k]
        assert keys and max(float(model.layout.ref_view(g_xt, k).abs().max()) for k in keys) > 0, m


def test_graphed_step_with_the_cross_triplet_term_matches_eager():
    """The shapes and warm-up of test_triplet_gpu.test_graphed_step_with_the_triplet_term_matches_eager, with this loss on."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    meta, state, batch, build = _tiny()
    images = {m: t.cuda() for m, t in batch['images'].items()}
    masks = dict(batch['modality_mask'])
    labels = batch['person_id'].cuda()

    def make():
        m = build(cross_triplet_weight=0.5)
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
    assert float(Lb['cross_triplet_loss'].detach()) > 0 and int(Lb['cross_triplet_active_cnt']) == int(La['cross_triplet_active_cnt']) > 0
    for k in ('total_loss', 'cross_triplet_loss'):
        a, b = float(La[k].detach()), float(Lb[k].detach())
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), k
