"""GPU: the cosine-margin identity heads (csrc/margin_ce.hip: NormFace / CosFace / ArcFace / Circle with a fused label-smoothed CE)
element by element, in both library flavors.

The two pieces are called through prcv2025reid_amd.ops on fp32 inputs that are strided views with NaN-sentinel padding columns, every
output inside a sentinel buffer (padding columns and 32 guard rows or elements must keep the sentinel bit for bit):
  x, W -> logits (reid_cos_logits_fwd);  logits -> row losses, (sum, count, mean) (reid_margin_ce_fwd);  -> dlogits
  (reid_margin_ce_bwd);  dlogits -> dx, dW (reid_cos_logits_bwd_prep, reid_cos_logits_bwd_fix).
Each piece is compared with the fp64 reference of margin_ce_ref.py ON THE INPUTS THE PIECE GOT (the CE pieces get the kernel's own
logits, the backward of the logits the kernel's own dlogits), next to the fp32 floor on the same inputs.
GATE (loss_refs.gate_limit, GATE_FACTOR = 4): normalised kernel error <= 4 x max(floor error, 2^-24); err_rows for logits, dlogits,
dx, dW, err_sums for the row losses, their sum and the mean; the count is exact; unused rows are exactly zero.  Arcface's phi jumps
at cos(pi - m): every case asserts on the fp64 reference that all target cosines stay 1e-3 away from it; no element is exempt.

Measured on an MI355X, identical in both flavors: kernel / floor of the sub-case closest to its own gate, and the share of the gate it used
(also in profiles/margin_ce_summary.md):

    output       kernel    floor     share of gate
    logits       3.59e-08  3.59e-08  0.15
    row_loss     1.90e-07  5.83e-08  0.80
    loss_sum     1.36e-07  2.52e-09  0.57
    loss         1.36e-07  2.52e-09  0.57
    dlogits      2.08e-07  9.11e-08  0.57
    dx           1.04e-07  1.38e-07  0.19
    dW           6.80e-07  6.55e-07  0.26
    model ce     4.56e-08  4.56e-08  0.19

With the products formed by reid_sgemm in fp32 (the first version of the kernels) the logits of single-class rows (9.0e-07 against a floor of
2.0e-10) and dW at D = 4 (2.1e-02 against 4.2e-03) were over the gate; the kernels now form products and sums in fp64.

The 2-rank data-parallel case reuses the model and batch of test_parallel_gpu.py (its worker cannot be given another head, so the
worker here is this file's own, in the pattern of test_triplet_gpu.py)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

import loss_refs as L
import margin_ce_ref as R
from helpers import is_sentinel, sentinel_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GUARD = 32
F32 = lambda v: float(np.float32(v))
WORST = {}                                      # output -> (kernel, floor) of the sub-case closest to its gate, over the module


@pytest.fixture(scope='module', autouse=True)
def report_worst():
    yield
    print('\n  margin CE, worst kernel/floor per output: ' + '  '.join(f'{k} {a:.2e}/{b:.2e}' for k, (a, b) in sorted(WORST.items())))


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    """Every test runs once per build flavor (libreid_hip.so = bf16 operands, libreid_hip_f16.so = f16)."""
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


# ---- sentinel buffers --------------------------------------------------------------------------------------------------------------
def padded_in(vals, ld):
    """fp32 device operand [rows, cols] inside a [rows + GUARD, ld] sentinel buffer: what lies beyond a row must never be read."""
    rows, cols = vals.shape
    buf = sentinel_buffer(rows + GUARD, ld, torch.float32)
    buf[:rows, :cols] = vals.cuda()
    return buf[:rows, :cols]


def out_mat(rows, cols, ld):
    buf = sentinel_buffer(rows + GUARD, ld, torch.float32)
    return buf, buf[:rows, :cols]


SENTINEL64 = 0x7FF4BADBADBADBAD                 # a signalling-NaN pattern of fp64, the role helpers.SENTINEL32 plays


def out_vec(n, dtype=torch.float32):
    if dtype == torch.float64:
        buf = torch.full((n + GUARD,), SENTINEL64, dtype=torch.int64, device='cuda').view(torch.float64)
    else:
        buf = sentinel_buffer(1, n + GUARD, torch.float32).view(-1)
    return buf, buf[:n]


def _is_sentinel(t):
    return t.view(torch.int64) == SENTINEL64 if t.dtype == torch.float64 else is_sentinel(t)


def untouched_mat(buf, rows, cols):
    assert bool(is_sentinel(buf[rows:]).all()), 'guard rows were written'
    assert bool(is_sentinel(buf[:rows, cols:]).all()), 'padding columns were written'
    assert not bool(is_sentinel(buf[:rows, :cols]).any()), 'an output element was not written'


def untouched_vec(buf, n):
    assert bool(_is_sentinel(buf[n:]).all()), 'guard elements were written'
    assert not bool(_is_sentinel(buf[:n]).any()), 'an output element was not written'


# ---- one case through both pieces -----------------------------------------------------------------------------------------------------
def make_case(rows, C, D, kind, mode, seed):
    m = F32(R.DEFAULTS[kind][1])
    x, W, lab = R.inputs(rows, C, D, seed, kind, m)
    g = torch.Generator().manual_seed(seed + 1)
    valid = None
    if mode == 'mixed':
        valid = (torch.rand(rows, generator=g) > 0.3).to(torch.uint8); valid[0] = 1
        if rows >= 16:
            valid[8:15] = 1                     # the constructed rows take part
    elif mode == 'zero':
        valid = torch.zeros(rows, dtype=torch.uint8)
    return x, W, lab, valid, m


def run_case(ops, rows, C, D, s, smoothing, mode, kind, pad, seed):
    """All five entry points on one case; returns (kernel errors, floor errors)."""
    x, W, lab, valid, m = make_case(rows, C, D, kind, mode, seed)
    s, sm = F32(s), F32(smoothing)
    x64, W64 = x.double(), W.double()
    l64, _, _ = R.cos_logits_plain(x64, W64, s)
    if kind == 'arcface' and mode != 'zero':
        gap = float((R.target_cosines(l64, lab, valid, s) - R.arc_threshold(m)).abs().min())
        assert gap >= 1e-3, f'a target cosine lies {gap:.2e} from the threshold of arcface: phi jumps there, pick other inputs'
    # ---- logits
    xv, Wv = padded_in(x, D + pad), padded_in(W, D + (pad + 4 if pad else 0))
    rxb, rx = out_vec(rows, torch.float64); rwb, rw = out_vec(C, torch.float64)
    lb, lv = out_mat(rows, C, C + (pad + 3 if pad else 0))
    ops.cos_logits_fwd(xv, Wv, s, R.EPS, rx, rw, lv)
    # ---- margin CE on the kernel's own logits
    labd = lab.cuda(); vd = None if valid is None else valid.cuda()
    rlb, rl = out_vec(rows); resb, res = out_vec(3)
    ops.margin_ce_fwd(lv, labd, vd, kind, s, m, sm, rl, res)
    dloss = torch.tensor([0.7], device='cuda')
    dlb, dlv = out_mat(rows, C, C + (pad + 5 if pad else 0))
    ops.margin_ce_bwd(lv, labd, vd, kind, s, m, sm, res, dloss, dlv)
    # ---- backward of the logits on the kernel's own dlogits
    Gb, G = out_vec(rows * D, torch.float64); Hb, H = out_vec(C * D, torch.float64)
    ops.cos_logits_bwd_prep(dlv, xv, Wv, rx, rw, G, H)
    dxb, dxv = out_mat(rows, D, D + (pad + 8 if pad else 0)); dWb, dWv = out_mat(C, D, D + (pad + 2 if pad else 0))
    ops.cos_logits_bwd_fix(xv, rx, G, dxv, Wv, rw, H, dWv, s, R.EPS)
    torch.cuda.synchronize()
    for buf, r, c in ((lb, rows, C), (dlb, rows, C), (dxb, rows, D), (dWb, C, D)):
        untouched_mat(buf, r, c)
    for buf, n in ((rxb, rows), (rwb, C), (rlb, rows), (resb, 3), (Gb, rows * D), (Hb, C * D)):
        untouched_vec(buf, n)
    lk, dlk = lv.cpu().contiguous(), dlv.cpu().contiguous()
    # ---- references and floors, piece by piece on the piece's inputs
    fl_l, _, _ = R.cos_logits_floor(x, W, s)
    loss64, scale64, _, ok = R.margin_ce_plain(lk.double(), lab, valid, sm, kind, s, m, 1.0)
    cnt = int(ok.sum())
    gs = float(np.float32(0.7) / np.float32(max(cnt, 1)))
    _, _, d64, _ = R.margin_ce_plain(lk.double(), lab, valid, sm, kind, s, m, gs)
    fl_loss, fl_d = R.margin_ce_floor(lk, lab, valid, sm, kind, s, m, gs)
    _, dx64, dW64 = R.cos_logits_plain(x64, W64, s, dlk.double())
    _, fl_dx, fl_dW = R.cos_logits_floor(x, W, s, dlk)
    res = res.cpu()
    assert float(res[1]) == cnt, (float(res[1]), cnt)                                  # the count is exact
    rlk = rl.cpu()
    assert float(rlk[~ok].abs().sum()) == 0.0 and float(dlk[~ok].abs().sum()) == 0.0    # unused rows are exactly zero
    if cnt == 0:
        assert float(res[0]) == 0.0 and float(res[2]) == 0.0 and float(dlk.abs().max()) == 0.0
        assert float(dxv.abs().max()) == 0.0 and float(dWv.abs().max()) == 0.0
    assert bool(torch.isfinite(lk).all()) and bool(torch.isfinite(dlk).all()) and bool(torch.isfinite(dxv).all()) and bool(torch.isfinite(dWv).all())
    total, tscale, n1 = float(loss64.sum()), float(scale64.sum()), max(cnt, 1)
    fl_total = float(fl_loss.sum())
    kernel = dict(logits=L.err_rows(lk, l64), row_loss=L.err_sums(rlk, loss64, scale64),
                  loss_sum=L.err_sums([float(res[0])], [total], [tscale]), loss=L.err_sums([float(res[2])], [total / n1], [tscale / n1]),
                  dlogits=L.err_rows(dlk, d64), dx=L.err_rows(dxv, dx64), dW=L.err_rows(dWv, dW64))
    floor = dict(logits=L.err_rows(fl_l, l64), row_loss=L.err_sums(fl_loss, loss64, scale64),
                 loss_sum=L.err_sums([fl_total], [total], [tscale]),
                 loss=L.err_sums([float(fl_loss.sum() / n1)], [total / n1], [tscale / n1]),
                 dlogits=L.err_rows(fl_d, d64), dx=L.err_rows(fl_dx, dx64), dW=L.err_rows(fl_dW, dW64))
    return kernel, floor


def report(tag, kernel, floor):
    """Print every figure, then assert the gate on each."""
    from prcv2025reid_amd import _lib
    bad = [k for k in kernel if not kernel[k] <= L.gate_limit(floor[k])]
    for k in kernel:
        w = WORST.get(k)
        if w is None or kernel[k] / L.gate_limit(floor[k]) > w[0] / L.gate_limit(w[1]):
            WORST[k] = (kernel[k], floor[k])
    print(f'\n  {tag} [{_lib.flavor()}]: ' + '  '.join(f'{k} {kernel[k]:.2e}/{floor[k]:.2e}' for k in kernel) + '   (kernel/floor)', end='')
    assert not bad, f'{tag}: over the gate: ' + ', '.join(f'{k}: kernel {kernel[k]:.3e} > {L.GATE_FACTOR:g} x max(floor {floor[k]:.3e}, 2^-24)'
                                                         for k in bad)


ROWS, DS, SCALES, MODES = (1, 5, 67), (4, 96, 512), (1, 30, 64), ('none', 'mixed', 'zero')


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C', [1, 7, 64, 65, 400, 1030])
def test_margin_heads_elementwise(ops, C, kind):
    """rows x D for one (C, kind); the scale and the valid mask rotate as Latin squares, so that over the module every (rows, D, scale,
    mask) combination occurs; smoothing and the padding alternate.  Labels 0, C - 1, -1 and C in every case with >= 5 rows; the constructed rows (cos = 1,
    cos = -1, a zero row, arcface's threshold +- 0.05, a circle negative below -m, a row below eps) in every case with 67 rows."""
    ci, ki = (1, 7, 64, 65, 400, 1030).index(C), R.KINDS.index(kind)
    for ri, rows in enumerate(ROWS):
        for di, D in enumerate(DS):
            i = 3 * ri + di
            s, mode, smoothing = SCALES[(ri + di + ci + ki) % 3], MODES[(ri + 2 * di + ki) % 3], (0.0, 0.1)[(i + ci) % 2]
            pad = 0 if (i + ki) % 2 == 0 else 12
            k, f = run_case(ops, rows, C, D, s, smoothing, mode, kind, pad, seed=1000 * i + 10 * C + ki)
            report(f'{kind} rows {rows} C {C} D {D} s {s} smoothing {smoothing} valid {mode} pad {pad}', k, f)


@pytest.mark.parametrize('kind', R.KINDS)
def test_full_size_rows_every_scale_and_mask(ops, kind):
    """67 rows x 1030 classes x 512 columns (more than one workgroup in every kernel, a 64-lane remainder in C) at every scale and
    mask, with the constructed rows."""
    for i, (s, mode) in enumerate(((1, 'mixed'), (30, 'none'), (64, 'mixed'), (30, 'zero'))):
        k, f = run_case(ops, 67, 1030, 512, s, 0.1, mode, kind, 12 if i % 2 else 0, seed=77 + i)
        report(f'{kind} rows 67 C 1030 D 512 s {s} valid {mode}', k, f)


# ---- autograd boundary ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_public_call_equals_the_entry_points_and_is_deterministic(ops, kind):
    """losses.margin_cross_entropy (CosineLinearFn + MarginCEFn) gives the bits of the entry points called by hand (which the tests
    above hold against the reference); two runs of forward + backward give identical bits; a frozen weight gets no gradient."""
    from prcv2025reid_amd import losses
    rows, C, D = 67, 400, 96
    x, W, lab, valid, m = make_case(rows, C, D, kind, 'mixed', 5)
    s = F32(R.DEFAULTS[kind][0])
    runs = []
    for _ in range(2):
        xa, Wa = x.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
        loss, cnt, logits = losses.margin_cross_entropy(xa, Wa, lab.cuda(), valid.cuda().bool(), kind=kind, scale=s, margin=m, smoothing=F32(0.1))
        (loss * 0.7).backward()
        runs.append((loss.detach().clone(), logits.detach().clone(), xa.grad.clone(), Wa.grad.clone()))
        assert int(cnt) == int(((lab >= 0) & (lab < C) & valid.bool()).sum())
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    xd, Wd, labd, vd = x.cuda(), W.cuda(), lab.cuda(), valid.cuda()
    f64 = dict(device='cuda', dtype=torch.float64)
    rx, rw, lg = torch.empty(rows, **f64), torch.empty(C, **f64), torch.empty(rows, C, device='cuda')
    ops.cos_logits_fwd(xd, Wd, s, R.EPS, rx, rw, lg)
    rl, res, dl = torch.empty(rows, device='cuda'), torch.empty(3, device='cuda'), torch.empty(rows, C, device='cuda')
    ops.margin_ce_fwd(lg, labd, vd, kind, s, m, F32(0.1), rl, res)
    ops.margin_ce_bwd(lg, labd, vd, kind, s, m, F32(0.1), res, torch.tensor([0.7], device='cuda'), dl)
    G, H = torch.empty(rows, D, **f64), torch.empty(C, D, **f64)
    ops.cos_logits_bwd_prep(dl, xd, Wd, rx, rw, G, H)
    dx, dW = torch.empty_like(xd), torch.empty_like(Wd)
    ops.cos_logits_bwd_fix(xd, rx, G, dx, Wd, rw, H, dW, s, R.EPS)
    assert torch.equal(runs[0][0], res[2]) and torch.equal(runs[0][1], lg) and torch.equal(runs[0][2], dx) and torch.equal(runs[0][3], dW)
    # only what autograd asks for: a frozen weight costs nothing and the gradient of x keeps its bits
    xa = x.cuda().requires_grad_(True); Wf = W.cuda()
    loss, _, _ = losses.margin_cross_entropy(xa, Wf, labd, vd, kind=kind, scale=s, margin=m, smoothing=F32(0.1))
    (loss * 0.7).backward()
    assert Wf.grad is None and torch.equal(xa.grad, dx)


def test_entry_points_refuse_bad_arguments(ops):
    from prcv2025reid_amd import _lib, losses
    x, W = torch.zeros(4, 8, device='cuda'), torch.ones(3, 8, device='cuda')
    lab = torch.zeros(4, dtype=torch.long, device='cuda')
    l, rl, res = torch.zeros(4, 3, device='cuda'), torch.zeros(4, device='cuda'), torch.zeros(3, device='cuda')
    for kind, s, m in (('cosface', 0.0, 0.3), ('cosface', 30.0, 1.0), ('arcface', 30.0, 1.6), ('circle', 30.0, -0.1)):
        with pytest.raises(_lib.ReidHipError, match='reid_margin_ce_fwd'):
            ops.margin_ce_fwd(l, lab, None, kind, s, m, 0.1, rl, res)
    with pytest.raises(_lib.ReidHipError, match='smoothing'):
        ops.margin_ce_fwd(l, lab, None, 'cosine', 30.0, 0.0, 1.5, rl, res)
    with pytest.raises(_lib.ReidHipError, match='scale'):
        ops.cos_logits_fwd(x, W, -1.0, R.EPS, torch.zeros(4, device='cuda', dtype=torch.float64), torch.zeros(3, device='cuda', dtype=torch.float64), l)
    with pytest.raises(ValueError, match='rx'):
        ops.cos_logits_fwd(x, W, 30.0, R.EPS, torch.zeros(3, device='cuda', dtype=torch.float64), torch.zeros(3, device='cuda', dtype=torch.float64), l)
    with pytest.raises(ValueError, match='features'):
        losses.margin_cross_entropy(x, W[:, :4], lab)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.margin_cross_entropy(x.cpu(), W.cpu(), lab.cpu())


# ---- model level ---------------------------------------------------------------------------------------------------------------------
BASE_KEYS = {'total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt'}


def _inputs(batch):
    return ({m: t.cuda() for m, t in batch['images'].items()}, {m: t.cuda() for m, t in batch['modality_mask'].items()},
            batch['person_id'].cuda())


def test_default_config_is_the_linear_head_bit_for_bit():
    from prcv2025reid_amd.head import LinearF32Fn
    from prcv2025reid_amd.losses import CrossEntropyLSFn
    from test_triplet_gpu import _tiny
    meta, state, batch, make = _tiny()
    images, masks, labels = _inputs(batch)
    model = make()
    assert model.id_head == 'linear' and model.dropout_rate == 0.0
    out = model(images=images, texts=batch['texts'], modality_masks=masks)
    Ld = model.compute_loss(out, labels)
    assert set(Ld) == BASE_KEYS
    W = dict(model.named_parameters())['bn_neck.classifier.weight']
    logits = LinearF32Fn.apply(out['bn_features'].detach(), W.detach(), None)
    assert torch.equal(logits, out['logits'])
    valid = (torch.stack([t.cuda() for t in out['feature_masks'].values()], dim=0) > 0).any(dim=0).to(torch.uint8)
    ce, cnt = CrossEntropyLSFn.apply(logits, labels, valid, 0.1)
    assert torch.equal(ce, Ld['ce_loss'].detach()) and int(cnt) == int(Ld['ce_valid_cnt'])
    total = model.ce_weight * ce + model.contrastive_weight * Ld['sdm_loss'].detach()
    assert torch.equal(total, Ld['total_loss'].detach())


@pytest.mark.parametrize('kind', ['cosface', 'circle'])
def test_model_with_a_margin_head(kind):
    """The dict keeps its keys; logits are the margin-free s * cos in training and in eval; ce_loss and the gradients of
    bn_neck.classifier.weight and of the classifier's input hold the gate against the reference fed with the model's own classifier
    input (dropout is off in the tiny configuration: the input is bn_features); the gradient of the fused feature equals the
    BN-neck's own backward of the reference's dx to 1e-3 of its largest element (that backward is linear in its cotangent and tested
    per element elsewhere; 1e-3 is the tolerance the project holds fp32 head quantities to); state_dict() keeps its keys."""
    from test_triplet_gpu import _tiny
    meta, state, batch, make = _tiny()
    images, masks, labels = _inputs(batch)
    keys0 = set(make().state_dict())
    model = make(id_head=kind)
    s, m = F32(R.DEFAULTS[kind][0]), F32(R.DEFAULTS[kind][1])
    assert (model.id_head, F32(model.id_scale), F32(model.id_margin)) == (kind, s, m)
    assert set(model.state_dict()) == keys0
    out = model(images=images, texts=batch['texts'], modality_masks=masks)
    Ld = model.compute_loss(out, labels)
    assert set(Ld) == BASE_KEYS
    Wp = dict(model.named_parameters())['bn_neck.classifier.weight']
    x, W, lab = out['bn_features'].detach().cpu(), Wp.detach().cpu(), labels.cpu()
    valid = (torch.stack([t.cpu() for t in out['feature_masks'].values()], dim=0) > 0).any(dim=0).to(torch.uint8)
    l64, _, _ = R.cos_logits_plain(x.double(), W.double(), s)
    fl_l, _, _ = R.cos_logits_floor(x, W, s)
    lk = out['logits'].detach().cpu()
    loss64, scale64, _, ok = R.margin_ce_plain(lk.double(), lab, valid, F32(0.1), kind, s, m, 1.0)
    n = int(ok.sum())
    assert n > 0 and int(Ld['ce_valid_cnt']) == n
    gs = float(np.float32(model.ce_weight) / np.float32(n))
    d64 = R.margin_ce_plain(lk.double(), lab, valid, F32(0.1), kind, s, m, gs)[2]
    fl_loss, fl_d = R.margin_ce_floor(lk, lab, valid, F32(0.1), kind, s, m, gs)
    # the feature gradient the reference's dx gives through the BN-neck's own backward (before the graph is freed)
    _, dx64, dW64 = R.cos_logits_plain(x.double(), W.double(), s, d64)
    (gfeat_ref,) = torch.autograd.grad(out['bn_features'], out['features'], dx64.float().cuda(), retain_graph=True)
    out['features'].retain_grad(); out['bn_features'].retain_grad()          # (after the call above: it would have filled .grad)
    model.lora_arena.grad = None
    Ld['total_loss'].backward()
    dxk, dWk = out['bn_features'].grad.cpu(), Wp.grad.cpu()
    _, fl_dx, fl_dW = R.cos_logits_floor(x, W, s, fl_d)
    kernel = dict(logits=L.err_rows(lk, l64), ce_loss=L.err_sums([float(Ld['ce_loss'].detach())], [float(loss64.sum()) / n], [float(scale64.sum()) / n]),
                  dx=L.err_rows(dxk, dx64), dW=L.err_rows(dWk, dW64))
    floor = dict(logits=L.err_rows(fl_l, l64), ce_loss=L.err_sums([float(fl_loss.sum() / n)], [float(loss64.sum()) / n], [float(scale64.sum()) / n]),
                 dx=L.err_rows(fl_dx, dx64), dW=L.err_rows(fl_dW, dW64))
    report(f'model id_head={kind}', kernel, floor)
    gfeat = out['features'].grad
    assert float(gfeat_ref.abs().max()) > 0
    assert float((gfeat - gfeat_ref).abs().max()) <= 1e-3 * float(gfeat_ref.abs().max())
    # eval: the same margin-free logits from the running statistics
    model.eval()
    with torch.no_grad():
        oe = model(images=images, texts=batch['texts'], modality_masks=masks)
    xe = oe['bn_features'].cpu()
    le64, _, _ = R.cos_logits_plain(xe.double(), W.double(), s)
    report(f'model id_head={kind} eval', dict(logits=L.err_rows(oe['logits'].cpu(), le64)),
           dict(logits=L.err_rows(R.cos_logits_floor(xe, W, s)[0], le64)))
    assert float(oe['logits'].abs().max()) <= s * (1 + 1e-5)


def test_model_refuses_an_unknown_head():
    from test_triplet_gpu import _tiny
    meta, state, batch, make = _tiny()
    with pytest.raises(ValueError, match='id_head'):
        make(id_head='softmax')
    with pytest.raises(ValueError, match='margin'):
        make(id_head='cosface', id_margin=1.5)


@pytest.mark.parametrize('kind', ['cosface', 'circle'])
def test_graphed_step_with_a_margin_head_matches_eager(kind):
    """The shapes and warm-up of test_triplet_gpu.test_graphed_step_with_the_triplet_term_matches_eager, with the head on: nothing
    is read back to the host, so the capture is unchanged."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_triplet_gpu import _tiny
    meta, state, batch, build = _tiny(id_head=kind)
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
    assert float(Lb['ce_loss']) > 0 and int(Lb['ce_valid_cnt']) == int(La['ce_valid_cnt']) > 0
    for k in ('total_loss', 'ce_loss'):
        assert abs(float(La[k]) - float(Lb[k])) <= 2e-3 * max(1.0, abs(float(Lb[k]))), k


# ---- two ranks -----------------------------------------------------------------------------------------------------------------------
def _dp_build():
    import test_parallel_gpu as tp
    model = tp._build()
    model.id_head, model.id_scale, model.id_margin = 'cosface', 30.0, 0.35
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
    n = tp.P * tp.K // world
    sl = slice(rank * n, (rank + 1) * n)
    dp = DataParallel(model)
    out = dp.forward(images={m: t[sl].cuda() for m, t in b['images'].items()}, texts={k: v[sl].cuda() for k, v in tok.items()},
                     modality_masks={m: t[sl] for m, t in b['modality_mask'].items()})
    Ld = dp.compute_loss(out, b['person_id'][sl].cuda())
    Ld['total_loss'].backward()
    dp.reduce_grads()
    cls = dict(model.named_parameters())['bn_neck.classifier.weight'].grad.cpu()
    torch.save({'loss': float(Ld['total_loss'].detach()), 'ce': float(Ld['ce_loss'].detach()), 'n': int(Ld['ce_valid_cnt']), 'cls': cls,
                'rows': int(out['logits'].shape[0])}, os.path.join(tmp, f'm{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_run_the_head_on_the_global_batch(tmp_path):
    """Under parallel.DataParallel the head sees the gathered batch on every rank: the margin CE and the (averaged) classifier gradient
    of both ranks equal one process on the global batch; no collective was added."""
    import torch.multiprocessing as mp
    world = 2
    port = 33100 + (os.getpid() % 1500)
    ctx = mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=False)
    deadline = time.monotonic() + 300
    while not ctx.join(timeout=5):                              # raises as soon as a rank fails: nothing below runs then
        if time.monotonic() > deadline:
            for pr in ctx.processes:
                pr.kill()
            pytest.fail('the ranks did not finish within 300 s')
    model, tp = _dp_build()
    b, tok = tp._batch(model)
    out = model(images={m: t.cuda() for m, t in b['images'].items()}, texts={k: v.cuda() for k, v in tok.items()},
                modality_masks=b['modality_mask'])
    Ld = model.compute_loss(out, b['person_id'].cuda())
    Ld['total_loss'].backward()
    gr = dict(model.named_parameters())['bn_neck.classifier.weight'].grad.cpu()
    for r in range(world):
        o = torch.load(os.path.join(str(tmp_path), f'm{r}.pt'))
        assert o['rows'] == tp.P * tp.K and o['n'] == int(Ld['ce_valid_cnt']) > 0
        for k in ('ce', 'loss'):
            want = float(Ld['ce_loss' if k == 'ce' else 'total_loss'].detach())
            assert abs(o[k] - want) <= 2e-6 * max(1.0, abs(want)), (r, k, o[k], want)
        assert float((o['cls'] - gr).norm() / gr.norm().clamp_min(1e-20)) < 2e-3
