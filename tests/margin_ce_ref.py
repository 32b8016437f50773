"""References of the cosine-margin identity heads (csrc/margin_ce.hip; test_margin_ce_cpu.py checks them on the CPU against an
independent textbook formulation, test_margin_ce_gpu.py compares the kernels with them).

Two pieces, as the library has them, each written plainly in closed form (no autograd) in the dtype of its inputs -- fp64 on the
exact upcast of the fp32 inputs is the reference:
  cos_logits_plain   x [B, D], W [C, D] -> logits l = s cos, and for a cotangent g = dL/dl the gradients dx, dW
  margin_ce_plain    logits l -> margin logits z', per-row label-smoothed CE, its error scale, dl
and next to each the *fp32 floor*, the role loss_refs.ce_floor plays: the same formulas in plain CPU PyTorch fp32 with autograd
(cos_logits_floor, margin_ce_floor).  The definitions are those of include/reid_hip.h."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-12
KINDS = ('cosine', 'cosface', 'arcface', 'circle')
DEFAULTS = {'cosine': (30.0, 0.0), 'cosface': (30.0, 0.35), 'arcface': (30.0, 0.5), 'circle': (64.0, 0.35)}
ARC_LO, ARC_HI = -1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23


def arc_threshold(m):
    return math.cos(math.pi - m)


# ---- cosine logits -----------------------------------------------------------------------------------------------------------------
def cos_logits_plain(x, W, s, g=None, eps=EPS):
    """(logits, dx, dW) in the dtype of ``x``; dx = dW = None without a cotangent ``g``.  A row whose norm is below eps is divided by
    eps and has no projection term."""
    nx, nw = x.pow(2).sum(1).sqrt(), W.pow(2).sum(1).sqrt()
    rx, rw = 1.0 / nx.clamp_min(eps), 1.0 / nw.clamp_min(eps)
    l = s * ((x @ W.t()) * rx[:, None] * rw[None, :])
    if g is None:
        return l, None, None
    dz = s * g * rx[:, None] * rw[None, :]
    tb, tc = (g * l).sum(1), (g * l).sum(0)
    dx = dz @ W - x * (rx * rx * tb * (nx >= eps).to(x.dtype))[:, None]
    dW = dz.t() @ x - W * (rw * rw * tc * (nw >= eps).to(x.dtype))[:, None]
    return l, dx, dW


def cos_logits_floor(x, W, s, g=None):
    """fp32 floor: s * F.linear(F.normalize(x), F.normalize(W)) on the CPU, gradients by autograd."""
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    l = s * F.linear(F.normalize(xr, dim=1, eps=EPS), F.normalize(Wr, dim=1, eps=EPS))
    if g is None:
        return l.detach(), None, None
    l.backward(g)
    return l.detach(), xr.grad, Wr.grad


# ---- margin CE ---------------------------------------------------------------------------------------------------------------------
def _used(labels, valid, C):
    ok = (labels >= 0) & (labels < C)
    if valid is not None:
        ok = ok & (valid != 0)
    return ok, torch.where(ok, labels, torch.zeros_like(labels))


def margin_logits(l, lab, kind, s, m):
    """(z', dz'/dl) of logits ``l`` = s cos for the labels ``lab`` (all inside [0, C)), closed form, in the dtype of ``l``."""
    onehot = torch.zeros_like(l, dtype=torch.bool); onehot.scatter_(1, lab.view(-1, 1), True)
    one = torch.ones_like(l)
    if kind == 'cosine':
        return l, one
    if kind == 'cosface':
        return torch.where(onehot, l - s * m, l), one
    cs = l / s
    if kind == 'arcface':
        t = cs.clamp(ARC_LO, ARC_HI)
        sq = (1 - t * t).sqrt()
        first = t > arc_threshold(m)
        phi = torch.where(first, t * math.cos(m) - sq * math.sin(m), t - m * math.sin(math.pi - m))
        dphi = torch.where(first, math.cos(m) + t * math.sin(m) / sq, one)
        dphi = dphi * ((cs >= ARC_LO) & (cs <= ARC_HI)).to(l.dtype)                # the clamp passes 1 inside, 0 outside
        return torch.where(onehot, s * phi, l), torch.where(onehot, dphi, one)
    if kind == 'circle':
        ap, an = (1 + m - cs).clamp_min(0), (cs + m).clamp_min(0)                   # constants of the gradient
        return torch.where(onehot, s * ap * (cs - (1 - m)), s * an * (cs - m)), torch.where(onehot, ap, an)
    raise ValueError(kind)


def target_cosines(l, labels, valid, s):
    """cos_y of the used rows (what arcface's discontinuity is judged on)."""
    ok, lab = _used(labels, valid, l.shape[1])
    return (l.gather(1, lab.view(-1, 1)).squeeze(1) / s)[ok]


def margin_ce_plain(l, labels, valid, smoothing, kind, s, m, grad_scale):
    """(row loss, its scale, dl, used) in the dtype of ``l``: loss_refs.ce_plain on the margin logits, dl through dz'/dl.  Rows with
    valid == 0 or a label outside [0, C) are unused: loss 0, gradient 0."""
    rows, C = l.shape
    ok, lab = _used(labels, valid, C)
    z, dzdl = margin_logits(l, lab, kind, s, m)
    mx = z.amax(1); lse = mx + torch.log(torch.exp(z - mx[:, None]).sum(1))
    zy = z.gather(1, lab.view(-1, 1)).squeeze(1)
    loss = (1 - smoothing) * (lse - zy) + smoothing * (lse - z.sum(1) / C)
    scale = lse.abs() + (1 - smoothing) * zy.abs() + smoothing * z.abs().sum(1) / C
    p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z); onehot.scatter_(1, lab.view(-1, 1), 1.0)
    # p_y - smoothing / C - (1 - smoothing) on the target is written (smoothing - smoothing / C) - sum_{c != y} p_c: the same number,
    # without the cancellation of p_y - 1, which would leave a reference of this row with no correct digit once 1 - p_y < 2^-53
    off = (p * (1 - onehot)).sum(1, keepdim=True)
    d = grad_scale * torch.where(onehot > 0, (smoothing - smoothing / C) - off, p - smoothing / C) * dzdl
    okf = ok.to(l.dtype)
    return loss * okf, scale * okf, d * okf[:, None], ok


def margin_ce_floor(l, labels, valid, smoothing, kind, s, m, grad_scale):
    """fp32 floor: the margin logits by torch ops (circle's alphas detached), F.cross_entropy(label_smoothing=...) per row on the
    CPU, gradient by autograd."""
    rows, C = l.shape
    ok, lab = _used(labels, valid, C)
    lr = l.clone().requires_grad_(True)
    loss = torch.zeros(rows, dtype=l.dtype)
    if bool(ok.any()):
        lo, yo = lr[ok], lab[ok]
        onehot = torch.zeros_like(lo, dtype=torch.bool); onehot.scatter_(1, yo.view(-1, 1), True)
        cs = lo / s
        if kind == 'cosine':
            z = lo
        elif kind == 'cosface':
            z = torch.where(onehot, lo - s * m, lo)
        elif kind == 'arcface':
            t = cs.clamp(ARC_LO, ARC_HI)
            phi = torch.where(t > arc_threshold(m), t * math.cos(m) - (1 - t * t).sqrt() * math.sin(m), t - m * math.sin(math.pi - m))
            z = torch.where(onehot, s * phi, lo)
        else:
            ap, an = (1 + m - cs.detach()).clamp_min(0), (cs.detach() + m).clamp_min(0)
            z = torch.where(onehot, s * ap * (cs - (1 - m)), s * an * (cs - m))
        rl = F.cross_entropy(z, yo, label_smoothing=smoothing, reduction='none')
        (rl.sum() * grad_scale).backward()
        loss[ok] = rl.detach()
    d = lr.grad if lr.grad is not None else torch.zeros_like(l)
    return loss, d


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs(rows, C, D, seed, kind, m, constructed=True):
    """fp32 x [rows, D] (8 x a unit-scale row, the BN-neck's output scale, with a spread of norms), W [C, D] (rows of unequal
    norm), labels [rows].  rows >= 5: the labels 0, C - 1, -1 and C in rows 0..3.  rows >= 16, D >= 2, ``constructed``: rows 8..14
    are built -- x = W_y (cos = 1), x = -W_y, an all-zero row, target cosines 0.05 above and 0.05 below arcface's threshold
    cos(pi - m) (of ``m`` when the kind is arcface, else of 0.5), x = -W_c for a class c != y (a circle negative with cos < -m:
    alpha_n = 0; C >= 2), and a row of norm 1e-20 (below eps)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, D, generator=g) * 8.0 * torch.exp(0.5 * torch.randn(rows, 1, generator=g))).float()
    W = (torch.randn(C, D, generator=g) * torch.exp(0.7 * torch.randn(C, 1, generator=g)) * 0.05).float()
    lab = torch.randint(0, C, (rows,), generator=g)
    if rows >= 5:
        lab[0] = 0; lab[1] = C - 1; lab[2] = -1; lab[3] = C
    if constructed and rows >= 16 and D >= 2:
        Wd = W.double()
        for r in range(8, 15):
            lab[r] = (r * 5 + 3) % C
        x[8] = W[lab[8]]
        x[9] = -W[lab[9]]
        x[10] = 0.0
        thr = arc_threshold(m if kind == 'arcface' else 0.5)
        for r, c in ((11, thr + 0.05), (12, thr - 0.05)):
            w = Wd[lab[r]] / Wd[lab[r]].norm()
            u = torch.randn(D, generator=g).double()
            u = u - (u @ w) * w
            u = u / u.norm()
            x[r] = (8.0 * (c * w + math.sqrt(1 - c * c) * u)).float()
        if C >= 2:
            x[13] = -W[(int(lab[13]) + 1) % C] * 3.0
        x[14] = 0.0; x[14, 0] = 1e-20
    return x, W, lab
