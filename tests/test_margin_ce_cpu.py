"""CPU: the references of the cosine-margin identity heads (margin_ce_ref.py) against an independent textbook formulation in torch
fp64 -- F.normalize, F.linear, torch.where, F.cross_entropy(label_smoothing=...), .detach() for circle's alphas, gradients by
autograd through the whole chain x, W -> loss -- plus the argument checks and the configuration default."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_refs as L
import margin_ce_ref as R

F32 = lambda v: float(np.float32(v))


def textbook(x, W, labels, valid, smoothing, kind, s, m, grad_scale):
    """(logits, row losses, used, dlogits, dx, dW) of grad_scale * sum of the used rows' losses, all by autograd in the dtype of x."""
    C = W.shape[0]
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    cos = F.linear(F.normalize(xr, dim=1, eps=R.EPS), F.normalize(Wr, dim=1, eps=R.EPS))
    logits = s * cos
    logits.retain_grad()
    cosl = logits / s
    ok = (labels >= 0) & (labels < C)
    if valid is not None:
        ok = ok & valid.bool()
    rl = torch.zeros(x.shape[0], dtype=x.dtype)
    if bool(ok.any()):
        c, y = cosl[ok], labels[ok]
        tgt = F.one_hot(y, C).bool()
        if kind == 'cosine':
            z = s * c
        elif kind == 'cosface':
            z = s * (c - m * tgt)
        elif kind == 'arcface':
            t = torch.clamp(c, -1 + 2.0 ** -23, 1 - 2.0 ** -23)
            theta = torch.acos(t)
            phi = torch.where(theta < math.pi - m, torch.cos(theta + m), t - m * math.sin(math.pi - m))     # cos(pi - m) < t <=> theta < pi - m
            z = s * torch.where(tgt, phi, c)
        else:
            ap = F.relu(1 + m - c.detach()); an = F.relu(c.detach() + m)
            z = s * torch.where(tgt, ap * (c - (1 - m)), an * (c - m))
        per = F.cross_entropy(z, y, label_smoothing=smoothing, reduction='none')
        (per.sum() * grad_scale).backward()
        rl[ok] = per.detach()
    zero = lambda t, like: t if t is not None else torch.zeros_like(like)
    return logits.detach(), rl, ok, zero(logits.grad, logits), zero(xr.grad, x), zero(Wr.grad, W)


def case(rows, C, D, seed, kind, mode):
    s, m = R.DEFAULTS[kind]
    s, m = F32(s), F32(m)
    x, W, lab = R.inputs(rows, C, D, seed, kind, m)
    g = torch.Generator().manual_seed(seed + 1)
    valid = None
    if mode == 'mixed':
        valid = (torch.rand(rows, generator=g) > 0.3).to(torch.uint8); valid[0] = 1
        if rows >= 16:
            valid[8:15] = 1
    elif mode == 'zero':
        valid = torch.zeros(rows, dtype=torch.uint8)
    return x, W, lab, valid, s, m


@pytest.mark.parametrize('smoothing', [0.0, 0.1])
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', [(1, 1, 4), (5, 7, 4), (21, 7, 96), (21, 65, 12), (5, 1, 8)])
def test_reference_equals_textbook_autograd(shape, kind, smoothing):
    rows, C, D = shape
    for i, mode in enumerate(('none', 'mixed', 'zero')):
        x, W, lab, valid, s, m = case(rows, C, D, 100 * rows + C + i, kind, mode)
        sm, gs = F32(smoothing), 0.37
        x, W = x.double(), W.double()
        l, rl, ok, dl, dx, dW = textbook(x, W, lab, valid, sm, kind, s, m, gs)
        l2, _, _ = R.cos_logits_plain(x, W, s)
        if kind == 'arcface' and bool(ok.any()):
            assert float((R.target_cosines(l2, lab, valid, s) - R.arc_threshold(m)).abs().min()) >= 1e-3
        loss2, scale2, dl2, ok2 = R.margin_ce_plain(l2, lab, valid, sm, kind, s, m, gs)
        _, dx2, dW2 = R.cos_logits_plain(x, W, s, dl2)
        assert torch.equal(ok, ok2)
        if mode == 'zero' or not bool(ok.any()):
            assert float(loss2.abs().max()) == 0 and float(dl2.abs().max()) == 0 and float(dx2.abs().max()) == 0 and float(dW2.abs().max()) == 0
        assert float(loss2[~ok].abs().sum()) == 0 and float(dl2[~ok].abs().sum()) == 0          # unused rows: exactly zero
        tol = 1e-9          # (acos / cos(theta + m) against the algebraic phi near |t| = 1: sqrt(1 - t^2) amplifies 1e-16 to ~1e-10)
        assert L.err_rows(l2, l) <= 1e-13
        assert L.err_sums(loss2, rl, scale2) <= tol
        # (where the clamp acts the gradient is 0 in both: torch.clamp.  p_y - 1 cancels in both: p = exp(z - lse) carries the rounding
        # of lse, 2^-53 |lse| <= 1e-14 absolutely, so a target with 1 - p_y = 1e-11 -- the constructed cos = 1 row -- agrees to 1e-5
        # of itself only: differences below 1e-13 gs are taken out before the row scale is applied)
        assert L.err_rows(torch.where((dl2 - dl).abs() <= 1e-13 * gs, dl, dl2), dl) <= tol
        for a, b in ((dx2, dx), (dW2, dW)):
            assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('smoothing', [0.0, 0.1])
def test_cosine_is_plain_ce_on_the_logits(smoothing):
    x, W, lab, valid, s, _ = case(21, 7, 12, 5, 'cosine', 'mixed')
    l, _, _ = R.cos_logits_plain(x.double(), W.double(), s)
    a = R.margin_ce_plain(l, lab, valid, F32(smoothing), 'cosine', s, 123.0, 0.7)          # the margin is ignored
    b = L.ce_plain(l, lab, valid, F32(smoothing), 0.7)
    for u, v in zip(a[:2] + a[3:], b[:2] + b[3:]):
        assert torch.equal(u, v)
    assert float((a[2] - b[2]).abs().max()) <= 1e-13 * 0.7      # the target's p_y - 1 is written without its cancellation: 2^-53 |lse| apart


def test_floor_is_the_same_function_in_fp32():
    for kind in R.KINDS:
        x, W, lab, valid, s, m = case(21, 65, 12, 9, kind, 'mixed')
        l64, _, _ = R.cos_logits_plain(x.double(), W.double(), s)
        l32, _, _ = R.cos_logits_floor(x, W, s)
        assert L.err_rows(l32, l64) <= 64 * L.U24
        loss64, scale64, d64, _ = R.margin_ce_plain(l32.double(), lab, valid, F32(0.1), kind, s, m, 0.5)
        loss32, d32 = R.margin_ce_floor(l32, lab, valid, F32(0.1), kind, s, m, 0.5)
        assert L.err_sums(loss32, loss64, scale64) <= 64 * L.U24
        _, dx64, dW64 = R.cos_logits_plain(x.double(), W.double(), s, d32.double())
        _, dx32, dW32 = R.cos_logits_floor(x, W, s, d32)
        assert L.err_rows(dx32, dx64) <= 1e-3 and L.err_rows(dW32, dW64) <= 1e-3


def test_argument_checks_raise():
    from prcv2025reid_amd import losses
    assert losses.MARGIN_DEFAULTS == R.DEFAULTS and losses.MARGIN_KINDS == R.KINDS and losses.EPS == R.EPS
    assert losses.margin_args('t', 'circle', None, None) == ('circle', 64.0, 0.35)
    assert losses.margin_args('t', 'cosine', None, 5.0) == ('cosine', 30.0, 0.0)              # ignored
    assert losses.margin_args('t', 'arcface', 16, 1.5) == ('arcface', 16.0, 1.5)
    x, W, lab = torch.zeros(4, 8), torch.zeros(3, 8), torch.zeros(4, dtype=torch.long)
    for kw in (dict(kind='softmax'), dict(scale=0.0), dict(scale=-1.0), dict(scale=float('inf')), dict(margin=-0.1),
               dict(kind='cosface', margin=1.0), dict(kind='circle', margin=1.0), dict(kind='arcface', margin=1.6), dict(smoothing=1.5)):
        with pytest.raises(ValueError):
            losses.margin_cross_entropy(x, W, lab, **kw)
    from prcv2025reid_amd import _lib
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.margin_cross_entropy(x, W, lab)


def test_config_defaults_to_the_linear_head():
    from prcv2025reid_amd.config import TrainingConfig
    c = TrainingConfig()
    assert c.id_head == 'linear' and c.id_scale is None and c.id_margin is None
