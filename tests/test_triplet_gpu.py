"""GPU: the batch-hard triplet loss kernels (csrc/triplet.hip) per element against the fp64 reference (triplet_ref.py), in both
library flavours, and the loss inside the model, the graphed step and the data-parallel path.

Every output lives between 32 guard elements (guard rows and padding columns for dx) that hold a sentinel NaN pattern and must keep it.

Bounds (u = 2^-24):
  * d_ap, d_an: relative D u / 2 -- a D-term sum of non-negative fp32 terms is within D u of the exact d2, the square root halves it;
  * loss: 4 u (1 + |loss|) + (D u / 2) * mean over the active anchors of (d_ap + d_an): the row loss is 1-Lipschitz in either distance;
  * n_active: exact;  idx_p / idx_n: the fp64 choice, except for anchors whose fp64 relative gap between the best and the runner-up
    candidate is below 2e-6 (at most 1 % of a case's anchors);
  * dx: per element 1e-5 of the row's largest |dx| of the fp64 gradient evaluated at the kernel's own selection.

Measured on an MI355X (both flavours give the same bits, the kernels are fp32; u = 2^-24): d_ap 3.3 u, d_an 3.7 u, loss 19 u (1 + |loss|),
dx 8.8e-6 of the row maximum (the soft-margin cases: sigmoid of the saved fp32 distances), 1 exempt anchor of 1024 in one case, 0 elsewhere;
profiles/triplet_summary.md.
"""
import os
import sys
import time

import pytest
import torch

import triplet_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 32
U = 2.0 ** -24
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
# P, K, D, ldx - D
SHAPES = [(4, 2, 512, 0), (5, 3, 96, 8), (16, 4, 512, 0), (1, 1, 4, 0), (65, 4, 256, 0), (256, 4, 512, 0), (3, 2, 1024, 0)]
WORST = {}


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
    """x in a [B, D + pad] buffer whose padding columns are NaN (a kernel that reads them poisons its result)."""
    if pad == 0:
        return x.contiguous()
    buf = torch.full((x.shape[0], x.shape[1] + pad), float('nan'), device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def run_fwd(ops, x, labels, valid, margin):
    B = x.shape[0]
    bufs = {k: guarded(B, torch.int32 if k.startswith('idx') else torch.float32) for k in ('d_ap', 'd_an', 'idx_p', 'idx_n', 'row_loss')}
    bufs['result'] = guarded(2, torch.float32)
    o = {k: v[1] for k, v in bufs.items()}
    ops.triplet_hard_fwd(x, labels, valid, -1.0 if margin is None else margin, o['d_ap'], o['d_an'], o['idx_p'], o['idx_n'], o['row_loss'],
                         o['result'])
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert untouched(buf, view.numel()), f'{k}: guard elements overwritten'
        assert not bool((view.view(torch.int32) == SENTINEL32).any()), f'{k}: elements not written'
    return o


def run_bwd(ops, x, margin, o, dloss, pad=4):
    B, D = x.shape
    buf = torch.full((B + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda').view(torch.float32)
    dx = buf[GUARD:GUARD + B, :D]
    ops.triplet_hard_bwd(x, -1.0 if margin is None else margin, o['d_ap'], o['d_an'], o['idx_p'], o['idx_n'], o['result'],
                         torch.tensor([dloss], device='cuda'), dx)
    torch.cuda.synchronize()
    raw = buf.view(torch.int32)
    assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + B:] == SENTINEL32).all()), 'dx: guard rows overwritten'
    assert bool((raw[GUARD:GUARD + B, D:] == SENTINEL32).all()), 'dx: padding columns overwritten'
    assert not bool(torch.isnan(dx).any())
    return dx


def note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))


def check_fwd(o, ref, D, x, labels, valid, margin, exact_index=False):
    """Every forward output against the reference; returns the number of exempt anchors."""
    B = x.shape[0]
    bound = 0.5 * D * U
    ip, inn = o['idx_p'].long(), o['idx_n'].long()
    assert float(o['result'][1]) == ref['n_active'] == int((ip >= 0).sum())
    assert bool(((ip >= 0) == (ref['idx_p'] >= 0)).all()) and bool(((inn >= 0) == (ref['idx_n'] >= 0)).all())
    assert bool((ip[ref['idx_p'] < 0] == -1).all()) and bool((inn[ref['idx_n'] < 0] == -1).all())
    wrong = (ip != ref['idx_p']) | (inn != ref['idx_n'])
    close = (ref['gap_p'] < 2e-6) | (ref['gap_n'] < 2e-6)
    exempt = int((close & (ref['idx_p'] >= 0)).sum())
    if exact_index:
        assert not bool(wrong.any()), torch.nonzero(wrong).flatten().tolist()
    else:
        assert not bool((wrong & ~close).any()), torch.nonzero(wrong & ~close).flatten().tolist()
        assert exempt <= 0.01 * B, exempt
    # distances and row losses are judged at the kernel's own selection (equal to the reference's outside the exempt anchors)
    own = R.evaluate(x, ip, inn, F32(margin) if margin is not None else None)
    for k in ('d_ap', 'd_an'):
        rel = ((o[k].double() - own[k]).abs() / own[k].clamp(min=1e-300))[ip >= 0]
        if rel.numel():
            note(k + ' rel / u', rel.max() / U)
            assert float(rel.max()) <= bound, (k, float(rel.max()), bound)
        assert bool((o[k][ip < 0] == 0).all())
    tol_rows = 4 * U * (1 + own['row_loss']) + bound * (own['d_ap'] + own['d_an'])
    assert bool(((o['row_loss'].double() - own['row_loss']).abs() <= tol_rows).all())
    tol = 4 * U * (1 + abs(own['loss'])) + bound * float((own['d_ap'] + own['d_an']).sum()) / max(1, own['n_active'])
    err = abs(float(o['result'][0]) - own['loss'])
    note('loss err / (u (1 + |loss|))', err / (U * (1 + abs(own['loss']))))
    assert err <= tol, (float(o['result'][0]), own['loss'], tol)
    return exempt


def check_bwd(dx, x, o, margin, dloss):
    ref = R.gradient(x, o['idx_p'], o['idx_n'], F32(margin) if margin is not None else None, dloss=F32(dloss))
    rowmax = ref.abs().max(dim=1, keepdim=True).values
    err = (dx.double() - ref).abs()
    assert bool((err <= 1e-5 * rowmax).all()), float((err / rowmax.clamp(min=1e-300)).max())
    live = rowmax.flatten() > 0
    if bool(live.any()):
        note('dx err / row max', (err[live] / rowmax[live]).max())
    return ref


_REFS = {}
MARGINS = [4.0, 12.0, None]     # with the generator's distances (d_ap - d_an between -10 and +2 over SHAPES) a hinge of 4 is open for part of
#                                 the anchors at most shapes, a hinge of 12 for every anchor at every shape; None = soft margin


def case(P, K, D, ratio, margin):
    """(x, labels, reference) of a generated case; the data and the mining are made once per (shape, ratio) and shared by the
    margins and the flavours."""
    key = (P, K, D, ratio)
    if key not in _REFS:
        x, labels = R.make_rows(P, K, D, ratio, seed=1000 * P + K + D + int(ratio), device='cuda')
        _REFS[key] = (x, labels, R.mine(x, labels, None))
    x, labels, (d2, ip, inn, gap_p, gap_n) = _REFS[key]
    ref = R.evaluate(x, ip, inn, F32(margin) if margin is not None else None)
    ref.update(idx_p=ip, idx_n=inn, gap_p=gap_p, gap_n=gap_n)
    return x, labels, ref


def assert_live(ref_grad, loss):
    """The comparison that follows is not 0 against 0."""
    assert loss > 0 and float(ref_grad.abs().max()) > 0


@pytest.mark.parametrize('margin', MARGINS)
@pytest.mark.parametrize('ratio', [0.0, 30.0, 100.0])
@pytest.mark.parametrize('P,K,D,pad', SHAPES)
def test_forward_and_backward_against_fp64(ops, P, K, D, pad, ratio, margin):
    x, labels, ref = case(P, K, D, ratio, margin)
    xs = strided(x, pad)
    o = run_fwd(ops, xs, labels, None, margin)
    exempt = check_fwd(o, ref, D, x, labels, None, margin)
    assert ref['n_active'] == (P * K if P > 1 and K > 1 else 0)
    dx = run_bwd(ops, xs, margin, o, 0.75)
    g = check_bwd(dx, x, o, margin, 0.75)
    if ref['n_active'] == 0:
        assert float(o['result'][0]) == 0.0 and float(dx.abs().max()) == 0.0
    elif margin != 4.0:                                         # every hinge open / soft margin: every anchor row carries gradient
        assert_live(g, ref['loss'])
        assert bool((g.abs().max(dim=1).values > 0).all())
    open_ = int((ref['row_loss'] > 0).sum())
    print(f'  P={P} K={K} D={D} ratio={ratio:g} margin={margin}: open {open_}/{P * K}, exempt {exempt}, worst so far {WORST}')


def test_partly_open_hinges_are_exercised():
    """The margin-4 cases mix open and closed hinges where it matters: the large shapes."""
    for P, K, D in ((16, 4, 512), (256, 4, 512)):
        _, _, ref = case(P, K, D, 0.0, 4.0)
        n_open = int((ref['row_loss'] > 0).sum())
        assert 0.25 * P * K < n_open < P * K, n_open


def test_exact_ties_go_to_the_lowest_index(ops):
    P, K, D = 6, 4, 96
    x, labels = R.make_rows(P, K, D, 30.0, seed=7, device='cuda')
    x[2] = x[1] + 50.0; x[3] = x[2]                             # identity 0: rows 2 and 3 equal and the farthest from rows 0 and 1
    x[9] = x[0] + 0.01; x[14] = x[9]                            # identities 2 and 3: equal rows, the nearest negatives of row 0
    ref = R.reference(x, labels, None, F32(12.0))
    assert int(ref['idx_p'][0]) == 2 and int(ref['idx_n'][0]) == 9 and float(ref['gap_p'][0]) == 0.0 and float(ref['gap_n'][0]) == 0.0
    o = run_fwd(ops, x, labels, None, 12.0)
    check_fwd(o, ref, D, x, labels, None, 12.0, exact_index=True)
    assert int(o['idx_p'][0]) == 2 and int(o['idx_p'][1]) == 2 and int(o['idx_n'][0]) == 9
    assert_live(check_bwd(run_bwd(ops, x, 12.0, o, 1.0), x, o, 12.0, 1.0), ref['loss'])


def test_exact_ties_across_waves_and_across_candidate_pieces(ops):
    """The three merge stages of the forward: lanes of one wave (the test above), the four waves of a workgroup (rows 64 apart), and a
    lane's running best over the 256-row candidate pieces (rows 256 apart: the same lane)."""
    P, K, D = 80, 4, 96
    x, labels = R.make_rows(P, K, D, 30.0, seed=9, device='cuda')
    labels = labels.clone()
    # (the far rows sit 5 sigma out in a random direction, not further: an outlier row's own two gradient terms are nearly parallel unit
    # vectors, and their difference must stay well conditioned for the 1e-5-of-the-row-maximum check of dx)
    v = 5.0 * torch.sign(torch.randn(D, generator=torch.Generator().manual_seed(3))).cuda()
    # anchor 0 (identity 0): tied farthest positives in the same lane of two pieces, tied nearest negatives in two waves
    labels[44] = 0; labels[300] = 0
    x[44] = x[0] + v; x[300] = x[44]
    x[10] = x[0] + 0.01; x[74] = x[10]
    # anchor 5 (identity 1): the other way round
    labels[11] = 1; labels[75] = 1
    x[11] = x[5] - v; x[75] = x[11]
    x[45] = x[5] + 0.01; x[301] = x[45]
    ref = R.reference(x, labels, None, F32(12.0))
    want = {0: (44, 10), 5: (11, 45)}
    for a, (p, n) in want.items():
        assert (int(ref['idx_p'][a]), int(ref['idx_n'][a])) == (p, n) and float(ref['gap_p'][a]) == 0.0 and float(ref['gap_n'][a]) == 0.0
    o = run_fwd(ops, x, labels, None, 12.0)
    for a, (p, n) in want.items():
        assert (int(o['idx_p'][a]), int(o['idx_n'][a])) == (p, n), a
    check_fwd(o, ref, D, x, labels, None, 12.0, exact_index=True)
    assert_live(check_bwd(run_bwd(ops, x, 12.0, o, 1.0), x, o, 12.0, 1.0), ref['loss'])


def test_near_duplicate_negative_keeps_the_distance_bound(ops):
    P, K, D = 16, 4, 512
    x, labels = R.make_rows(P, K, D, 100.0, seed=11, device='cuda')
    g = torch.Generator().manual_seed(5)
    x[7] = x[0] + 1e-3 * torch.randn(D, generator=g).cuda()    # row 7 (identity 1) sits 1e-3 sigma from row 0 (identity 0)
    ref = R.reference(x, labels, None, F32(0.3))
    assert int(ref['idx_n'][0]) == 7 and int(ref['idx_n'][7]) == 0
    assert float(ref['d_an'][0]) < 2e-3 * float(ref['d_ap'][0])
    o = run_fwd(ops, x, labels, None, 0.3)
    check_fwd(o, ref, D, x, labels, None, 0.3)
    rel = abs(float(o['d_an'][0]) - float(ref['d_an'][0])) / float(ref['d_an'][0])
    print(f'  near-duplicate d_an = {float(ref["d_an"][0]):.3e}: relative error {rel:.2e} (bound {0.5 * D * U:.2e})')
    assert rel <= 0.5 * D * U
    check_bwd(run_bwd(ops, x, 0.3, o, 1.0), x, o, 0.3, 1.0)


def test_true_duplicate_as_the_only_positive_is_clamped(ops):
    # margin 1000: every hinge is open, so every term carries c = 1 / n_active and a term that should vanish would show
    P, K, D, margin = 5, 2, 96, 1000.0
    x, labels = R.make_rows(P, K, D, 0.0, seed=13, device='cuda')
    x[3] = x[2]                                                 # identity 1: a true duplicate, d2 = 0
    x[4, 0] = 0.0; x[5] = x[4]; x[5, 0] = 5e-7                  # identity 2: d2 = 2.5e-13 <= 1e-12 with a non-zero difference
    ref = R.reference(x, labels, None, margin)
    o = run_fwd(ops, x, labels, None, margin)
    check_fwd(o, ref, D, x, labels, None, margin, exact_index=True)
    clamp = float(torch.tensor(1e-12, dtype=torch.float32).sqrt())
    assert [float(o['d_ap'][i]) for i in (2, 3, 4, 5)] == [clamp] * 4
    dx = run_bwd(ops, x, margin, o, 1.0)
    check_bwd(dx, x, o, margin, 1.0)
    # an unclamped term would put c * 5e-7 / 1e-6 = 0.5 / n_active into column 0 of rows 4 and 5: far outside check_bwd's tolerance
    unclamped = 0.5 / ref['n_active']
    assert unclamped > 100 * 1e-5 * float(dx[4].abs().max())


@pytest.mark.parametrize('kind', ['some_invalid', 'all_invalid', 'one_identity', 'k1'])
@pytest.mark.parametrize('margin', [4.0, None])
def test_validity_and_degenerate_batches(ops, kind, margin):
    P, K, D = 5, 2, 96
    x, labels = R.make_rows(P, K, D, 30.0, seed=17, device='cuda')
    valid = None
    if kind == 'some_invalid':
        valid = torch.ones(P * K, dtype=torch.uint8, device='cuda')
        valid[1] = 0; valid[6] = 0                              # rows 0 and 7 lose their only positive
    elif kind == 'all_invalid':
        valid = torch.zeros(P * K, dtype=torch.uint8, device='cuda')
    elif kind == 'one_identity':
        labels = torch.full_like(labels, 3)
    else:
        labels = torch.arange(P * K, device='cuda')
    ref = R.reference(x, labels, valid, F32(margin) if margin is not None else None)
    o = run_fwd(ops, x, labels, valid, margin)
    check_fwd(o, ref, D, x, labels, valid, margin, exact_index=True)
    dx = run_bwd(ops, x, margin, o, 1.0)
    check_bwd(dx, x, o, margin, 1.0)
    if kind == 'some_invalid':
        assert ref['n_active'] == 6 and [int(o['idx_p'][i]) for i in (0, 1, 6, 7)] == [-1] * 4
        assert float(dx[1].abs().max()) == 0.0 and float(dx[6].abs().max()) == 0.0          # invalid rows are no candidates either
        assert 1 not in o['idx_n'].tolist() and 6 not in o['idx_n'].tolist()
    else:
        assert ref['n_active'] == 0 and float(o['result'][0]) == 0.0 and float(o['result'][1]) == 0.0
        assert bool((o['idx_p'] == -1).all()) and bool((o['idx_n'] == -1).all())
        assert float(dx.abs().max()) == 0.0


def test_hinge_exactly_at_zero_has_no_gradient(ops):
    # integers as floats: anchor 0 has d_ap = 5 (row 1), d_an = 6 (row 2), margin 1 -> d_ap - d_an + margin == 0 exactly
    x = torch.tensor([[0, 0, 0, 0], [3, 4, 0, 0], [6, 0, 0, 0], [0, 0, 0, 20]], dtype=torch.float32, device='cuda')
    labels = torch.tensor([0, 0, 1, 1], device='cuda')
    ref = R.reference(x, labels, None, 1.0)
    o = run_fwd(ops, x, labels, None, 1.0)
    check_fwd(o, ref, 4, x, labels, None, 1.0, exact_index=True)
    assert float(o['d_ap'][0]) == 5.0 and float(o['d_an'][0]) == 6.0 and float(o['row_loss'][0]) == 0.0
    assert float(o['row_loss'][1]) > 0                          # (the other anchors are live, so a `>=` in the derivative would show)
    dx = run_bwd(ops, x, 1.0, o, 1.0)
    check_bwd(dx, x, o, 1.0, 1.0)
    # the check discriminates: with anchor 0's hinge open (a `>=` in the derivative) dx[0] would differ by (x0 - x1) / 5 - (x0 - x2) / 6
    opened = R.gradient(x, o['idx_p'], o['idx_n'], 1.0 + 1e-9)
    assert float((dx[0].double() - opened[0]).abs().max()) > 0.01


def test_soft_margin_does_not_overflow(ops):
    # anchor 0: d_ap = 60, d_an = 10 -> z = +50;  anchor 4: d_ap = 10, d_an = 60 -> z = -50;  anchor 5: z = -60
    x = torch.tensor([[0, 0, 0, 0], [60, 0, 0, 0], [0, 10, 0, 0], [0, 20, 0, 0], [0, 0, 0, 60], [0, 0, 0, 70]], dtype=torch.float32, device='cuda')
    labels = torch.tensor([0, 0, 1, 1, 2, 2], device='cuda')
    ref = R.reference(x, labels, None, None)
    z = (ref['d_ap'] - ref['d_an']).tolist()
    assert z[0] == 50.0 and z[4] == -50.0 and max(z) == 50.0 and min(z) == -60.0, z
    o = run_fwd(ops, x, labels, None, None)
    check_fwd(o, ref, 4, x, labels, None, None, exact_index=True)
    assert bool(torch.isfinite(o['row_loss']).all()) and bool(torch.isfinite(o['result']).all())
    dx = run_bwd(ops, x, None, o, 1.0)
    assert bool(torch.isfinite(dx).all())
    check_bwd(dx, x, o, None, 1.0)


def test_two_runs_give_the_same_bits(ops):
    P, K, D = 65, 4, 256
    x, labels, _ = case(P, K, D, 30.0, None)
    runs = []
    for _ in range(2):
        o = run_fwd(ops, x, labels, None, 12.0)                 # every hinge open: every dx row is live
        dx = run_bwd(ops, x, 12.0, o, 1.0)
        runs.append([o[k].view(torch.int32).clone() for k in ('d_ap', 'd_an', 'idx_p', 'idx_n', 'row_loss', 'result')] + [dx.view(torch.int32).clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool((runs[0][-1].view(torch.float32).abs().max(dim=1).values > 0).all())


def test_public_call_and_autograd(ops):
    """The autograd boundary by value: open hinges (margin 4: a mix; margin None) and an upstream factor that is not 1."""
    from prcv2025reid_amd import losses, _lib
    from prcv2025reid_amd.model import LazyCount
    for margin, up in ((4.0, 2.0), (None, -0.7)):
        x, labels, ref = case(16, 4, 512, 100.0, margin)
        f = x.clone().requires_grad_(True)
        loss, n, rows = losses.batch_hard_triplet(f, labels, margin=margin)
        assert isinstance(n, LazyCount) and int(n) == ref['n_active'] == 64 and set(rows) == {'d_ap', 'd_an', 'idx_p', 'idx_n'}
        assert torch.equal(rows['idx_p'].long(), ref['idx_p']) and torch.equal(rows['idx_n'].long(), ref['idx_n'])
        saved = {k: v.clone() for k, v in rows.items()}
        for v in rows.values():
            v.zero_()                                           # the arrays handed out are copies: writing into them must not reach the backward
        (up * loss).backward()
        g = check_bwd(f.grad, x, saved, margin, up)
        assert_live(g, float(loss.detach()))
        assert int((g.abs().max(dim=1).values > 0).sum()) >= 30   # (margin 4 opens 30 of the 64 hinges of this case, the soft margin all)
        tol = 4 * U * (1 + ref['loss']) + 0.5 * 512 * U * float((ref['d_ap'] + ref['d_an']).mean())
        assert abs(float(loss.detach()) - ref['loss']) <= tol
    with pytest.raises(ValueError, match='margin'):
        losses.batch_hard_triplet(x, labels, margin=-1.0)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.batch_hard_triplet(x.cpu(), labels.cpu())
    with pytest.raises(_lib.ReidHipError):
        ops.triplet_hard_fwd(x[:, :6], labels, None, 0.3, saved['d_ap'], saved['d_an'], saved['idx_p'], saved['idx_n'], saved['d_ap'].clone(),
                             torch.empty(2, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny(**over):
    from helpers import load_case, case_inputs
    from test_model_gpu import build_model
    z, meta = load_case('tiny_train_frozen')
    cfg, arch, state, batch, tokens = case_inputs(meta)
    return meta, state, batch, (lambda **kw: build_model(meta, state, True, **{**over, **kw}))


def _features_reference(out, labels, margin):
    fm = out['feature_masks']
    valid = (torch.stack([t.cuda() for t in fm.values()], dim=0) > 0).any(dim=0)
    return R.reference(out['features'].detach(), labels, valid, F32(margin)), valid


def test_model_loss_with_the_triplet_term():
    meta, state, batch, make = _tiny()
    images = {m: t.cuda() for m, t in batch['images'].items()}
    masks = {m: t.cuda() for m, t in batch['modality_mask'].items()}
    labels = batch['person_id'].cuda()
    grads = {}
    for w in (0.0, 0.3):
        model = make(triplet_weight=w)
        out = model(images=images, texts=batch['texts'], modality_masks=masks)
        L = model.compute_loss(out, labels)
        L['total_loss'].backward()
        grads[w] = model.lora_arena.grad.detach().clone()
        if w == 0.0:
            assert set(L) == {'total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt'}
            continue
        assert set(L) == {'total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt', 'triplet_loss', 'triplet_active_cnt'}
        want = model.ce_weight * float(L['ce_loss']) + model.contrastive_weight * float(L['sdm_loss']) + 0.3 * float(L['triplet_loss'])
        assert abs(float(L['total_loss']) - want) <= 8 * U * (1 + abs(want))       # five fp32 roundings of non-negative terms <= want
        ref, valid = _features_reference(out, labels, 0.3)
        D = out['features'].shape[1]
        tol = 4 * U * (1 + ref['loss']) + 0.5 * D * U * float((ref['d_ap'] + ref['d_an']).sum()) / max(1, ref['n_active'])
        assert ref['n_active'] > 0 and ref['loss'] > 0 and int(L['triplet_active_cnt']) == ref['n_active']
        assert abs(float(L['triplet_loss']) - ref['loss']) <= tol, (float(L['triplet_loss']), ref['loss'])
    assert float((grads[0.3] - grads[0.0]).abs().max()) > 0


def test_graphed_step_with_the_triplet_term_matches_eager():
    """The shapes and warm-up of test_step_gpu.test_graphed_step_matches_eager, with the loss on."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    meta, state, batch, build = _tiny(triplet_weight=0.3)
    images = {m: t.cuda() for m, t in batch['images'].items()}
    masks = dict(batch['modality_mask'])
    labels = batch['person_id'].cuda()

    def make():
        m = build()
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
    assert float(Lb['triplet_loss']) > 0 and int(Lb['triplet_active_cnt']) == int(La['triplet_active_cnt']) > 0
    for k in ('total_loss', 'triplet_loss'):
        assert abs(float(La[k]) - float(Lb[k])) <= 2e-3 * max(1.0, abs(float(Lb[k]))), k


# ---------------------------------------------------------------------------------------------------------------- two ranks
def _dp_build():
    import test_parallel_gpu as tp
    model = tp._build()
    model.triplet_weight = 0.3
    return model, tp


def _dp_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import datetime
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from prcv2025reid_amd.parallel import DataParallel
    model, tp = _dp_build()
    b, tok = tp._batch(model)
    order = _dp_order()
    n = len(order) // world
    sl = order[rank * n:(rank + 1) * n]
    images = {m: t[sl].cuda() for m, t in b['images'].items()}
    masks = {m: torch.ones_like(t[sl]) for m, t in b['modality_mask'].items()}
    tokens = {k: v[sl].cuda() for k, v in tok.items()}
    labels = b['person_id'][sl].cuda()
    dp = DataParallel(model)
    out = dp.forward(images=images, texts=tokens, modality_masks=masks)
    L = dp.compute_loss(out, labels)
    torch.save({'loss': float(L['total_loss'].detach()), 'triplet': float(L['triplet_loss'].detach()), 'n': int(L['triplet_active_cnt'])},
               os.path.join(tmp, f't{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def _dp_order():
    """Rows of the P x K = 4 x 2 batch interleaved: every identity has one row on rank 0 and one on rank 1, so the hardest (only)
    positive of every rank-0 anchor lives on rank 1."""
    import test_parallel_gpu as tp
    return torch.tensor([2 * i for i in range(tp.P)] + [2 * i + 1 for i in range(tp.P)])


def test_two_ranks_mine_the_global_batch(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    port = 31300 + (os.getpid() % 1500)
    ctx = mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=False)
    deadline = time.monotonic() + 300
    while not ctx.join(timeout=5):                              # raises as soon as a rank fails: nothing below runs then
        if time.monotonic() > deadline:
            for pr in ctx.processes:
                pr.kill()
            pytest.fail('the ranks did not finish within 300 s')
    model, tp = _dp_build()
    b, tok = tp._batch(model)
    order = _dp_order()
    out = model(images={m: t[order].cuda() for m, t in b['images'].items()}, texts={k: v[order].cuda() for k, v in tok.items()},
                modality_masks={m: torch.ones_like(t[order]) for m, t in b['modality_mask'].items()})
    labels = b['person_id'][order].cuda()
    L = model.compute_loss(out, labels)
    ref, _ = _features_reference(out, labels, 0.3)
    n = len(order) // world
    assert ref['n_active'] == len(order) and all(int(ref['idx_p'][i]) >= n for i in range(n))      # rank 0's positives live on rank 1
    for r in range(world):
        o = torch.load(os.path.join(str(tmp_path), f't{r}.pt'))
        assert o['n'] == int(L['triplet_active_cnt']) == ref['n_active']
        assert abs(o['triplet'] - float(L['triplet_loss'])) <= 2e-6 * max(1.0, abs(float(L['triplet_loss']))), (r, o, float(L['triplet_loss']))
        assert abs(o['loss'] - float(L['total_loss'])) <= 2e-6 * max(1.0, abs(float(L['total_loss']))), (r, o, float(L['total_loss']))
