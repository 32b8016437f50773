"""fp64 reference of the batch-hard triplet loss (include/reid_hip.h, reid_triplet_hard_*), written plainly in torch and sharing no
code with the package.

    d2(i,j) = sum_c (x_ic - x_jc)^2,  d = sqrt(max(d2, 1e-12)); where d2 <= 1e-12 that term has no gradient.
    hardest positive: valid j != i, same label, largest d2; hardest negative: valid j, other label, smallest d2; ties -> lowest index.
    active anchor: valid, has a positive and a negative; idx_p = idx_n = -1 and d_ap = d_an = row_loss = 0 otherwise.
    row loss: max(0, d_ap - d_an + margin) (margin >= 0) or softplus(d_ap - d_an) (margin None); loss = sum / max(1, n_active).
"""
import math

import torch

CLAMP = 1e-12


def pairwise_d2(x, chunk=64):
    """[B, B] fp64 squared distances in the difference form."""
    x = x.double()
    B = x.shape[0]
    out = torch.empty(B, B, dtype=torch.float64, device=x.device)
    for s in range(0, B, chunk):
        d = x[s:s + chunk, None, :] - x[None, :, :]
        out[s:s + chunk] = (d * d).sum(-1)
    return out


def row_loss_fn(z, margin):
    if margin is None:
        return z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    return (z + margin).clamp(min=0)


def row_dloss_fn(z, margin):
    if margin is None:
        return torch.sigmoid(z)
    return ((z + margin) > 0).double()


def _first_best(vals):
    """(best value, LOWEST index holding it, runner-up value) per row of ``vals`` (larger is better, -inf = no candidate)."""
    B = vals.shape[1]
    top = torch.topk(vals, min(2, B), dim=1).values
    best = top[:, 0]
    second = top[:, 1] if B > 1 else torch.full_like(best, -math.inf)
    ar = torch.arange(B, device=vals.device).expand_as(vals)
    idx = torch.where(vals == best[:, None], ar, torch.full_like(ar, B)).min(dim=1).values
    return best, idx, second


def mine(x, labels, valid=None):
    """d2 [B, B], idx_p, idx_n (int64, -1 = inactive), and the relative gap between the best and the runner-up candidate of each kind
    (inf when there is no runner-up)."""
    d2 = pairwise_d2(x)
    B = d2.shape[0]
    v = torch.ones(B, dtype=torch.bool, device=d2.device) if valid is None else valid.to(d2.device) != 0
    labels = labels.to(d2.device)
    same = labels[:, None] == labels[None, :]
    eye = torch.eye(B, dtype=torch.bool, device=d2.device)
    ninf = torch.full_like(d2, -math.inf)
    bp, ip, sp = _first_best(torch.where(same & ~eye & v[None, :], d2, ninf))
    bn, inn, sn = _first_best(torch.where(~same & v[None, :], -d2, ninf))
    active = v & torch.isfinite(bp) & torch.isfinite(bn)
    gap_p = torch.where(torch.isfinite(sp), (bp - sp) / bp.clamp(min=1e-300), torch.full_like(bp, math.inf))
    gap_n = torch.where(torch.isfinite(sn), (bn - sn) / (-bn).clamp(min=1e-300), torch.full_like(bn, math.inf))
    minus = torch.full_like(ip, -1)
    return d2, torch.where(active, ip, minus), torch.where(active, inn, minus), gap_p, gap_n


def evaluate(x, idx_p, idx_n, margin):
    """Distances, row losses, loss and n_active (all fp64) for a GIVEN selection."""
    x = x.double()
    idx_p, idx_n = idx_p.long().to(x.device), idx_n.long().to(x.device)
    active = idx_p >= 0
    a = torch.nonzero(active).flatten()
    B = x.shape[0]
    d_ap = torch.zeros(B, dtype=torch.float64, device=x.device); d_an = torch.zeros_like(d_ap); rl = torch.zeros_like(d_ap)
    d2p = ((x[a] - x[idx_p[a]]) ** 2).sum(-1); d2n = ((x[a] - x[idx_n[a]]) ** 2).sum(-1)
    d_ap[a] = d2p.clamp(min=CLAMP).sqrt(); d_an[a] = d2n.clamp(min=CLAMP).sqrt()
    rl[a] = row_loss_fn(d_ap[a] - d_an[a], margin)
    n = int(active.sum())
    return dict(d_ap=d_ap, d_an=d_an, row_loss=rl, loss=float(rl.sum() / max(1, n)), n_active=n, d2p=d2p, d2n=d2n, anchors=a)


def reference(x, labels, valid=None, margin=0.3):
    d2, ip, inn, gap_p, gap_n = mine(x, labels, valid)
    out = evaluate(x, ip, inn, margin)
    out.update(idx_p=ip, idx_n=inn, gap_p=gap_p, gap_n=gap_n)
    return out


def gradient(x, idx_p, idx_n, margin, dloss=1.0):
    """d (dloss * loss) / dx [B, D] fp64 for a GIVEN selection (the analytic formula of the header)."""
    x = x.double()
    e = evaluate(x, idx_p, idx_n, margin)
    a = e['anchors']
    p, n = idx_p.long().to(x.device)[a], idx_n.long().to(x.device)[a]
    c = dloss * row_dloss_fn(e['d_ap'][a] - e['d_an'][a], margin) / max(1, e['n_active'])
    sp = torch.where(e['d2p'] > CLAMP, c / e['d_ap'][a], torch.zeros_like(c))
    sn = torch.where(e['d2n'] > CLAMP, c / e['d_an'][a], torch.zeros_like(c))
    tp = sp[:, None] * (x[a] - x[p]); tn = sn[:, None] * (x[a] - x[n])
    dx = torch.zeros_like(x)
    dx.index_add_(0, a, tp - tn)
    dx.index_add_(0, p, -tp)
    dx.index_add_(0, n, tn)
    return dx


def loop_reference(x, labels, valid=None, margin=0.3):
    """The same definition with plain Python loops over lists (small inputs only)."""
    X = [[float(v) for v in row] for row in x.double().tolist()]
    L = [int(v) for v in labels.tolist()]
    V = [True] * len(X) if valid is None else [bool(v) for v in valid.tolist()]
    B = len(X)
    idx_p, idx_n, d_ap, d_an, rl = [-1] * B, [-1] * B, [0.0] * B, [0.0] * B, [0.0] * B
    for i in range(B):
        if not V[i]:
            continue
        bp, jp, bn, jn = -1.0, -1, math.inf, -1
        for j in range(B):
            if not V[j]:
                continue
            d2 = sum((a - b) ** 2 for a, b in zip(X[i], X[j]))
            if L[j] == L[i]:
                if j != i and d2 > bp:
                    bp, jp = d2, j
            elif d2 < bn:
                bn, jn = d2, j
        if jp < 0 or jn < 0:
            continue
        idx_p[i], idx_n[i] = jp, jn
        d_ap[i], d_an[i] = math.sqrt(max(bp, CLAMP)), math.sqrt(max(bn, CLAMP))
        z = d_ap[i] - d_an[i]
        rl[i] = max(0.0, z + margin) if margin is not None else max(z, 0.0) + math.log1p(math.exp(-abs(z)))
    n = sum(1 for j in idx_p if j >= 0)
    return dict(idx_p=idx_p, idx_n=idx_n, d_ap=d_ap, d_an=d_an, row_loss=rl, loss=sum(rl) / max(1, n), n_active=n)


def make_rows(P, K, D, ratio, seed, device='cpu'):
    """The generator of the issue: rows = common mean x ratio + class offset x 0.7 + N(0,1), P identities of K rows, as float32.
    The common mean has |m_c| in [0.5, 1.5) with a random sign, so |mean| / std per column is about ``ratio``."""
    g = torch.Generator().manual_seed(seed)
    m = (0.5 + torch.rand(D, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (D,), generator=g).double() * 2 - 1)
    off = torch.randn(P, D, generator=g, dtype=torch.float64)
    labels = torch.arange(P).repeat_interleave(K)
    x = m[None, :] * ratio + 0.7 * off[labels] + torch.randn(P * K, D, generator=g, dtype=torch.float64)
    return x.float().to(device), labels.to(device)
