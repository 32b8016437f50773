"""GPU: the center-loss kernels (csrc/center.hip) against the two references of center_ref.py, in both library flavours (the kernels
are fp32: the same bits in both), and the loss behind the public call, inside the model and in the graphed step.

Every output and the table live between 32 guard elements that hold a sentinel pattern and must keep it; padded input rows carry
NaN in their padding, padded output rows the sentinel.

  * diff, the centres after an update and dx EQUAL the float32 loop bit for bit (element-wise chains with a fixed order);
  * d2 within (D + 3) u and the loss within (D + 5) u (relative, u = 2^-24) of the fp64 form; n_used exact (center_ref.py: why).
"""
import types

import numpy as np
import pytest
import torch

import center_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 32
U = R.U
_CASE = {}                               # shape -> the case on the CPU with its loop and fp64 references (shared by the flavours)


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


def bits(t):
    t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t
    return t.detach().cpu().contiguous().view(torch.int32)


class Table:
    """centers [C, D] between guards."""

    def __init__(self, init):
        C, D = init.shape
        self.buf, flat = guarded(C * D)
        self.t = flat.view(C, D)
        self.t.copy_(torch.as_tensor(init))

    def intact(self):
        return untouched(self.buf, self.t.numel())


def run_fwd(ops, x, labels, valid, table, pad=0):
    """The forward of x [S, N, D] (on the device) against ``table``; every output between guards."""
    S, N, D = x.shape
    o = dict(S=S, N=N, D=D, x2=strided(x, pad), labels=labels, valid=None if valid is None else valid.reshape(-1).contiguous())
    o['b_ws'], o['ws'] = guarded(ops.center_ws_floats(S, N, D))
    o['b_d2'], o['d2'] = guarded(S * N)
    o['b_res'], o['result'] = guarded(2)
    ops.center_fwd(o['x2'], labels, o['valid'], table.t, o['ws'], o['d2'], o['result'], S=S)
    torch.cuda.synchronize()
    for k in ('ws', 'd2', 'res'):
        view = o['result' if k == 'res' else k]
        assert untouched(o['b_' + k], view.numel()), f'{k}: guard elements overwritten'
        assert not bool((view.view(torch.int32) == SENTINEL32).any()), f'{k}: elements not written'
    assert table.intact()
    o['diff'] = o['ws'][:S * N * D].view(S * N, D)
    return o


def run_update(ops, o, table, alpha):
    ops.center_update(o['labels'], o['valid'], o['d2'], o['ws'], table.t, alpha, S=o['S'])
    torch.cuda.synchronize()
    assert table.intact()


def run_bwd(ops, o, dloss, pad=4):
    """dx [S*N, D] between guard rows and sentinel padding columns."""
    rows, D = o['S'] * o['N'], o['D']
    buf = torch.full((rows + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda').view(torch.float32)
    dx = buf[GUARD:GUARD + rows, :D]
    ops.center_bwd(o['ws'], o['result'], torch.tensor([dloss], dtype=torch.float32, device='cuda'), dx, S=o['S'])
    torch.cuda.synchronize()
    raw = buf.view(torch.int32)
    assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + rows:] == SENTINEL32).all()), 'dx: guard rows overwritten'
    assert bool((raw[GUARD:GUARD + rows, D:] == SENTINEL32).all()), 'dx: padding columns overwritten'
    assert not bool((raw[GUARD:GUARD + rows, :D] == SENTINEL32).any()), 'dx: elements not written'
    return dx


def case(shape):
    if shape not in _CASE:
        S, N, D, C, pad = shape
        x, labels, valid, centers = R.make_case(S, N, D, C, S * 1000 + N)
        f = R.loop_forward(x, labels, valid, centers.numpy())
        L64, n64, d64 = R.ref64_loss(x, labels, valid, centers)
        _CASE[shape] = dict(x=x, labels=labels, valid=valid, centers=centers, loop=f, L64=float(L64), n64=n64, d64=d64,
                            new=R.loop_update(f['diff'], f['d2'], labels, f['used'], centers.numpy(), 0.5),
                            dx=R.loop_backward(f['diff'], f['used'], f['n_used'], -0.7))
    return _CASE[shape]


# ---------------------------------------------------------------------------------------------------------------- 1. one batch
@pytest.mark.parametrize('shape', R.SHAPES)
def test_kernels_against_the_references(ops, shape):
    S, N, D, C, pad = shape
    c = case(shape)
    f = c['loop']
    assert f['n_used'] > 0 and (N < 5 or (not f['used'].all() and 0 < int(c['valid'].reshape(-1).ne(0).sum()) < S * N))
    table = Table(c['centers'])
    o = run_fwd(ops, c['x'].cuda(), c['labels'].cuda(), c['valid'].cuda(), table, pad)
    assert torch.equal(bits(o['diff']), bits(f['diff']))
    d2 = o['d2'].double().cpu()
    assert bool(((d2 - c['d64']).abs() <= R.d2_bound(D) * c['d64']).all()) and bool((d2[~torch.from_numpy(f['used'])] == 0).all())
    assert float(o['result'][1]) == f['n_used'] == c['n64']
    assert abs(float(o['result'][0]) - c['L64']) <= R.loss_bound(D) * c['L64'] and c['L64'] > 0
    assert torch.equal(bits(table.t), bits(c['centers']))       # the forward reads the table only
    dx = run_bwd(ops, o, -0.7, pad=4)
    assert torch.equal(bits(dx), bits(c['dx'])) and float(dx.abs().max()) > 0
    run_update(ops, o, table, 0.5)
    assert torch.equal(bits(table.t), bits(c['new'])) and not torch.equal(bits(table.t), bits(c['centers']))
    # the backward reads what the forward saved: the same bits after the table has moved
    assert torch.equal(bits(run_bwd(ops, o, -0.7, pad=0)), bits(c['dx']))


# ---------------------------------------------------------------------------------------------------------------- 2. a stream
@pytest.mark.parametrize('shape', R.SHAPES)
def test_stream_of_batches_into_one_table(ops, shape):
    S, N, D, C, pad = shape
    table = Table(torch.zeros(C, D))
    shadow = np.zeros((C, D), dtype=np.float32)
    kept = 0
    for s in range(1, R.STEPS + 1):
        x, labels, valid = R.stream_step(S, N, D, C, s)
        f = R.loop_forward(x, labels, valid, shadow)
        before = shadow
        shadow = R.loop_update(f['diff'], f['d2'], labels, f['used'], shadow, 0.5)
        o = run_fwd(ops, x.cuda(), labels.cuda(), valid.cuda(), table, pad)
        assert torch.equal(bits(o['diff']), bits(f['diff'])), s
        run_update(ops, o, table, 0.5)
        assert torch.equal(bits(table.t), bits(shadow)), s
        present = {int(j) for r, j in enumerate(labels.repeat(S).tolist()) if f['used'][r]}
        for j in range(C):
            if j not in present:                                 # absent from the batch: the row keeps its bits
                kept += 1
                assert torch.equal(bits(table.t[j]), bits(before[j])), (s, j)
    assert float(np.abs(shadow).max()) > 0 and (C <= 2 or kept >= R.STEPS)


# ---------------------------------------------------------------------------------------------------------------- 3. edge cases
def test_all_invalid_batch(ops):
    S, N, D, C, pad = R.SHAPES[2]
    c = case(R.SHAPES[2])
    for labels, valid in ((c['labels'], torch.zeros(S, N, dtype=torch.uint8)), (torch.full((N,), C), None), (torch.full((N,), -1), c['valid'])):
        table = Table(c['centers'])
        o = run_fwd(ops, c['x'].cuda(), labels.cuda(), None if valid is None else valid.cuda(), table, pad)
        assert o['result'].tolist() == [0.0, 0.0] and float(o['d2'].abs().max()) == 0.0 and float(o['diff'].abs().max()) == 0.0
        run_update(ops, o, table, 0.5)
        assert torch.equal(bits(table.t), bits(c['centers']))
        dx = run_bwd(ops, o, 3.0)
        assert float(dx.abs().max()) == 0.0 and not bool(torch.signbit(dx).any())


def test_non_finite_rows_do_not_reach_the_centres(ops):
    S, N, D, C = 2, 8, 64, 5
    x, _, _, centers = R.make_case(S, N, D, C, 7)
    labels = torch.tensor([0, 0, 1, 2, 2, 3, 3, 1]); valid = torch.ones(S, N, dtype=torch.uint8)
    x[0, 0, 3] = float('nan'); x[1, 3, 60] = float('inf')      # rows 0 (class 0) and 11 (class 2)
    table = Table(centers)
    o = run_fwd(ops, x.cuda(), labels.cuda(), valid.cuda(), table)
    assert not bool(torch.isfinite(o['result'][0])) and float(o['result'][1]) == S * N
    run_update(ops, o, table, 0.5)
    valid2 = valid.clone(); valid2[0, 0] = 0; valid2[1, 3] = 0
    f = R.loop_forward(torch.nan_to_num(x, 0.0, 0.0, 0.0), labels, valid2, centers.numpy())
    want = R.loop_update(f['diff'], f['d2'], labels, f['used'], centers.numpy(), 0.5)
    assert torch.equal(bits(table.t), bits(want)) and bool(torch.isfinite(table.t).all())
    assert torch.equal(bits(table.t[4]), bits(centers[4])) and not torch.equal(bits(table.t[0]), bits(centers[0]))
    dx = run_bwd(ops, o, 1.0)                                    # the step is skipped on its loss; the other rows' gradient is still finite
    fin = torch.ones(S * N, dtype=torch.bool); fin[0] = False; fin[11] = False
    assert bool(torch.isfinite(dx.cpu()[fin]).all()) and not bool(torch.isfinite(dx[0]).all()) and not bool(torch.isfinite(dx[11]).all())


def test_first_contributing_row_of_a_class_beyond_the_first_64_rows(ops):
    """120 rows: class 2 has ONE contributing row, row 110; class 1's are rows 111 .. 119 (their instances are invalid on sides 0 and 1);
    class 0's spread over both 64-row groups.  The waves of rows 110 and 111 lead from the middle of the second group."""
    S, N, D, C = 3, 40, 8, 3
    x, _, _, centers = R.make_case(S, N, D, C, 9)
    labels = torch.tensor([0] * 30 + [2] + [1] * 9)
    valid = torch.ones(S, N, dtype=torch.uint8); valid[:2, 30:] = 0
    f = R.loop_forward(x, labels, valid, centers.numpy())
    assert [r for r in range(S * N) if f['used'][r] and r % N >= 30] == list(range(110, 120))
    want = R.loop_update(f['diff'], f['d2'], labels, f['used'], centers.numpy(), 0.5)
    table = Table(centers)
    o = run_fwd(ops, x.cuda(), labels.cuda(), valid.cuda(), table)
    run_update(ops, o, table, 0.5)
    assert torch.equal(bits(table.t), bits(want)) and all(not torch.equal(bits(table.t[j]), bits(centers[j])) for j in range(C))


def test_backward_is_independent_of_a_later_forward_and_update(ops):
    shape = R.SHAPES[4]
    S, N, D, C, pad = shape
    c = case(shape)
    x2, labels2, valid2 = R.stream_step(S, N, D, C, 2)
    runs = []
    for later in (False, True):
        table = Table(c['centers'])
        o = run_fwd(ops, c['x'].cuda(), c['labels'].cuda(), c['valid'].cuda(), table)
        if later:
            run_update(ops, o, table, 0.5)
            o2 = run_fwd(ops, x2.cuda(), labels2.cuda(), valid2.cuda(), table)
            run_update(ops, o2, table, 0.5)
            assert not torch.equal(bits(table.t), bits(c['new']))
        runs.append(bits(run_bwd(ops, o, 1.25)))
    assert torch.equal(runs[0], runs[1]) and bool((runs[0] != 0).any())


def test_two_runs_give_the_same_bits(ops):
    S, N, D, C, pad = R.SHAPES[3]
    runs = []
    for _ in range(2):
        table, out = Table(torch.zeros(C, D)), []
        for s in (1, 2, 3):
            x, labels, valid = R.stream_step(S, N, D, C, s)
            o = run_fwd(ops, x.cuda(), labels.cuda(), valid.cuda(), table)
            run_update(ops, o, table, 0.5)
            out += [bits(o['ws']), bits(o['d2']), bits(o['result']), bits(run_bwd(ops, o, -2.0)), bits(table.t)]
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and bool((runs[0][-1] != 0).any())


# ---------------------------------------------------------------------------------------------------------------- 4. argument checks
def test_violated_requirements_are_refused_and_write_nothing(ops):
    from prcv2025reid_amd import _lib
    S, N, D, C = 2, 5, 8, 4
    h = _lib.lib()
    t = {n: torch.full((k,), SENTINEL32, dtype=torch.int32, device='cuda') for n, k in
         (('x', 2 * S * N * D), ('centers', 2 * C * D), ('ws', 2 * (S * N * D + S * N)), ('d2', S * N), ('result', 2), ('dloss', 1),
          ('dx', 2 * S * N * D))}
    t['labels'] = torch.zeros(N, dtype=torch.int64, device='cuda')
    t['valid'] = torch.ones(S * N, dtype=torch.uint8, device='cuda')
    good = dict(S=S, N=N, D=D, C=C, ldx=D, lddx=D, alpha=0.5, stream=_lib.stream_ptr(), **{n: v.data_ptr() for n, v in t.items()})
    seen = set()
    for entry, over, text in R.violations(S, N, D, C):
        rc = R.call(h, entry, R.bad_arguments(good, over))
        assert rc == -1, (entry, over, rc)
        assert text.encode() in h.reid_last_error(), (entry, over, h.reid_last_error())
        seen.add(entry)
    torch.cuda.synchronize()
    assert seen == {'ws', 'fwd', 'update', 'bwd'}
    for n, v in t.items():
        assert bool((v == (0 if n == 'labels' else 1 if n == 'valid' else SENTINEL32)).all()), f'{n} was written'


# ---------------------------------------------------------------------------------------------------------------- 5. public call
@pytest.mark.parametrize('flat', [True, False])
def test_public_call_against_autograd(ops, flat):
    from prcv2025reid_amd import losses, _lib
    S, N, D, C, _ = (1, 16, 512, 6, 0) if flat else R.SHAPES[4]
    x, labels, valid, centers = R.make_case(S, N, D, C, 21)
    xin, vin = (x[0], valid[0]) if flat else (x, valid)
    table = losses.ClassCenters(C, D, 'cuda')
    table.load_state({'centers': centers})
    xa = xin.cuda().requires_grad_(True)
    loss, n_used, rows = losses.center_loss(xa, labels.cuda(), table, valid=vin.cuda() != 0, alpha=0.25)
    x64 = x.double().requires_grad_(True)
    L64, n64, d64 = R.ref64_loss(x64, labels, valid, centers)
    assert int(n_used) == n64 > 0 and rows['d2'].shape == xin.shape[:-1]
    assert abs(float(loss.detach()) - float(L64.detach())) <= R.loss_bound(D) * float(L64.detach())
    assert bool(((rows['d2'].double().cpu().reshape(-1) - d64.detach()).abs() <= R.d2_bound(D) * d64.detach()).all())
    rows['d2'].zero_()                                           # a copy: writing into it must not reach the backward
    (loss * -1.5).backward()
    (L64 * -1.5).backward()
    g = x64.grad[0] if flat else x64.grad
    assert xa.grad.shape == xin.shape and float(g.abs().max()) > 0
    # coef and the product: two roundings of a difference that carries one -> 4 u of the element
    assert bool(((xa.grad.double().cpu() - g).abs() <= 4 * U * g.abs() + 1e-300).all())
    want = R.ref64_update(x, labels, valid, centers, 0.25)
    assert float((table.centers.double().cpu() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert not torch.equal(table.centers.cpu(), centers)
    # update=False leaves the table as it is
    before = bits(table.centers)
    loss2, _, _ = losses.center_loss(xin.cuda(), labels.cuda(), table, valid=vin.cuda(), update=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(table.centers), before) and float(loss2) != float(loss.detach())
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.center_loss(xin.cuda()[..., :8], labels.cuda(), table)
    with pytest.raises(TypeError, match='ClassCenters'):
        losses.center_loss(xin.cuda(), labels.cuda(), table.centers)
    with pytest.raises(ValueError, match='alpha'):
        losses.center_loss(xin.cuda(), labels.cuda(), table, alpha=float('nan'))
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.center_loss(xin, labels, table)
    assert torch.equal(bits(table.centers), before)              # a refused call moves nothing


# ---------------------------------------------------------------------------------------------------------------- 6. model level
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


def _model_inputs(model, out, source):
    """(x [S, B, D], valid [S, B]) the model's center term must have used."""
    raw, fm = out['raw_modality_features'], out['feature_masks']
    if source == 'fused':
        return out['features'].detach()[None], (torch.stack([t.cuda() for t in fm.values()]) > 0).any(0)[None]
    mods = [m for m in raw if m in fm]
    mods = [m for m in mods if m == 'vis'] + [m for m in mods if m != 'vis']
    assert mods[0] == 'vis' and len(mods) >= 2
    return torch.stack([raw[m].detach() for m in mods]), torch.stack([fm[m].cuda() > 0 for m in mods])


@pytest.mark.parametrize('source', ['fused', 'modalities'])
def test_model_loss_with_the_center_term(source):
    from test_triplet_gpu import _tiny
    meta, state, batch_, make = _tiny()
    w = 0.05
    model = make(center_weight=w, center_source=source, center_alpha=0.5)
    assert model.centers is None
    keys_before = set(model.state_dict())
    table = None
    for s in range(1, 4):
        out, L, labels = _step(model, batch_)
        assert set(L) == BASE_KEYS | {'center_loss', 'center_valid_cnt'}
        want = model.ce_weight * float(L['ce_loss'].detach()) + model.contrastive_weight * float(L['sdm_loss'].detach()) + w * float(L['center_loss'].detach())
        assert abs(float(L['total_loss'].detach()) - want) <= 8 * U * (1 + abs(want))
        x, valid = _model_inputs(model, out, source)
        S, B, D = x.shape
        if table is None:
            table = torch.zeros(model.num_classes, D, dtype=torch.float64)
        assert model.centers.centers.shape == (model.num_classes, D)
        L64, n64, _ = R.ref64_loss(x.cpu(), labels.cpu(), valid.cpu().to(torch.uint8), table.float())
        assert int(L['center_valid_cnt']) == n64 > 0 and float(L64) > 0
        assert abs(float(L['center_loss'].detach()) - float(L64)) <= R.loss_bound(D) * float(L64), s
        # the centres moved, by Wen's rule
        new = R.ref64_update(x.cpu(), labels.cpu(), valid.cpu().to(torch.uint8), table.float(), 0.5)
        got = model.centers.centers.double().cpu()
        assert float((got - table).abs().max()) > 0
        assert float((got - new).abs().max()) <= 1e-6 * float(new.abs().max())
        table = got
    assert float(model.lora_arena.grad.abs().max()) > 0
    assert set(model.state_dict()) == keys_before                # the table is no parameter and no buffer
    # eval() and no_grad(): the loss is there, the centres stay
    before = bits(model.centers.centers)
    with torch.no_grad():
        _, Ln, _ = _step(model, batch_, backward=False)
    assert 'center_loss' in Ln and torch.equal(bits(model.centers.centers), before)
    model.eval()
    _, Le, _ = _step(model, batch_, backward=False)
    assert 'center_loss' in Le and torch.equal(bits(model.centers.centers), before)
    held = model.centers.centers
    model.reset_centers()
    assert model.centers.centers is held and float(held.abs().max()) == 0.0
    model.set_num_classes(model.num_classes)                     # the same C keeps the table, another C drops it
    assert model.centers is not None
    model.set_num_classes(model.num_classes + 3)
    assert model.centers is None


def test_weight_zero_is_the_model_without_the_fields():
    from helpers import case_config
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    from test_triplet_gpu import _tiny
    meta, state, batch_, make = _tiny()
    cfg = case_config(meta, device='cuda')
    cfg.compute_dtype = 'bf16'
    bare = types.SimpleNamespace(**{k: v for k, v in vars(cfg).items() if not k.startswith('center_')})
    assert not hasattr(bare, 'center_weight') and hasattr(cfg, 'center_weight')
    old = CLIPBasedMultiModalReIDModel(bare)
    old.set_num_classes(int(meta['num_classes'])); old.load_state_dict(state, strict=True); apply_reference_freeze(old)
    old.contrastive_weight = meta['contrastive_weight']; old.set_epoch(2); old.train(True)
    _, L_old, _ = _step(old, batch_, backward=False)
    new = make(center_weight=0.0, center_source='modalities')
    _, L_new, _ = _step(new, batch_, backward=False)
    assert set(L_old) == set(L_new) == BASE_KEYS and new.centers is None and old.centers is None
    assert torch.equal(bits(L_old['total_loss']), bits(L_new['total_loss']))


# ---------------------------------------------------------------------------------------------------------------- 7. graphed step
def test_graphed_step_with_the_center_term_matches_eager():
    """The shapes, warm-up, comparison and tolerance of test_xbm_gpu.test_graphed_step_with_the_xbm_term_matches_eager: the table lives on
    the device and is updated in place, so the replays keep moving it."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_triplet_gpu import _tiny
    meta, state, batch_, build = _tiny()
    images = {m: t.cuda() for m, t in batch_['images'].items()}
    masks = dict(batch_['modality_mask'])
    labels = batch_['person_id'].cuda()

    def make():
        m = build(center_weight=0.05, center_source='modalities')
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
    assert float(Lb['center_loss'].detach()) > 0 and int(Lb['center_valid_cnt']) == int(La['center_valid_cnt']) > 0
    for k in ('total_loss', 'center_loss'):
        va, vb = float(La[k].detach()), float(Lb[k].detach())
        assert abs(va - vb) <= 2e-3 * max(1.0, abs(vb)), k
    ca, cb = a.centers.centers.double().cpu(), b.centers.centers.double().cpu()
    assert float(cb.abs().max()) > 0
    assert bool(((ca - cb).abs() <= 2e-3 * cb.abs().clamp(min=1.0)).all())
