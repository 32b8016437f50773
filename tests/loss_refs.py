"""Plain high-precision references, error scales and the gate of the neck / loss / metric kernel tests (test_loss_kernels_gpu.py,
checked on the CPU by test_loss_refs_cpu.py).

Every floating-point kernel is judged the same way: its error against the operation written plainly in fp64 on the exact upcast
of the fp32 inputs, next to the error of the plain PyTorch fp32 implementation on the CPU (the *fp32 floor*) on the same inputs,
both normalised by a scale that does not let a large element hide a small one.  The kernel may be at most GATE_FACTOR times worse
than max(floor, 2^-24)."""
import numpy as np
import torch

U24 = 2.0 ** -24          # fp32 unit roundoff
GATE_FACTOR = 4.0         # 2 (hardware rsqrt / exp / log: up to ~2 ulp where libm gives 1) x 2 (another summation order)


# ---- error scales ------------------------------------------------------------------------------------------------------------
def _d(t):
    if not torch.is_tensor(t):
        return torch.from_numpy(np.asarray(t, dtype=np.float64))
    return t.detach().cpu().double()


def err_rows(out, ref):
    """Worst |out - ref| / (max|ref| of the same row).  A row whose reference is exactly zero must be exactly zero (inf otherwise)."""
    out, ref = _d(out), _d(ref)
    if not bool(torch.isfinite(out).all()):
        return float('inf')
    scale = ref.abs().amax(dim=1, keepdim=True)
    diff = (out - ref).abs()
    zero = scale == 0
    if bool((diff[zero.expand_as(diff)] != 0).any()):
        return float('inf')
    e = diff / torch.where(zero, torch.ones_like(scale), scale)
    return float(e.max())


def err_elems(out, ref):
    """Worst |out - ref| / |ref| per element; where the reference is exactly zero the output must be (inf otherwise)."""
    out, ref = _d(out), _d(ref)
    if not bool(torch.isfinite(out).all()):
        return float('inf')
    diff = (out - ref).abs()
    zero = ref == 0
    if bool((diff[zero] != 0).any()):
        return float('inf')
    return float((diff / torch.where(zero, torch.ones_like(ref), ref.abs())).max()) if ref.numel() else 0.0


def err_sums(out, ref, abs_sum):
    """Worst |out - ref| / (sum of the absolute values of the summed terms, fp64): for reductions that may cancel."""
    out, ref, abs_sum = _d(out), _d(ref), _d(abs_sum)
    if not bool(torch.isfinite(out).all()):
        return float('inf')
    diff = (out - ref).abs()
    zero = abs_sum == 0
    if bool((diff[zero] != 0).any()):
        return float('inf')
    return float((diff / torch.where(zero, torch.ones_like(abs_sum), abs_sum)).max()) if ref.numel() else 0.0


def gate_limit(floor_err, factor=GATE_FACTOR):
    return factor * max(float(floor_err), U24)


def gate_ok(kernel_err, floor_err, factor=GATE_FACTOR):
    """The gate: worst normalised kernel error <= factor x max(worst normalised floor error on the same inputs, 2^-24)."""
    return float(kernel_err) <= gate_limit(floor_err, factor)


# ---- BN-neck -----------------------------------------------------------------------------------------------------------------
def bn_inputs(rows, D, ratios, seed, negative=False):
    """x = m_c + s_c n with |m_c| / s_c taken from `ratios` column by column (cyclically); fp32, CPU."""
    g = torch.Generator().manual_seed(seed)
    r = torch.tensor([ratios[c % len(ratios)] for c in range(D)], dtype=torch.float64)
    s = 0.5 + torch.rand(D, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0).double() if negative else torch.ones(D, dtype=torch.float64)
    x = (sign * r * s + s * torch.randn(rows, D, generator=g, dtype=torch.float64)).float()
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).float(); beta = (0.1 * torch.randn(D, generator=g)).float()
    rm = (0.1 * torch.randn(D, generator=g)).float(); rv = (1 + 0.1 * torch.rand(D, generator=g)).float()
    dy = torch.randn(rows, D, generator=g).float()
    return x, gamma, beta, rm, rv, dy


def bn_neck_plain(x, gamma, beta, rm, rv, dy, training, eps=1e-5, momentum=0.1, scale=8.0):
    """BN-neck forward and backward written plainly in the dtype of `x` (fp64 for the reference): two-pass batch statistics,
    running statistics with the unbiased variance, y = scale * z / max(||z||, 1e-12), and the pieces the kernels save or return."""
    rows = x.shape[0]
    if training:
        mean = x.mean(0); var = ((x - mean) ** 2).mean(0)
        rm_new = (1 - momentum) * rm + momentum * mean
        rv_new = (1 - momentum) * rv + momentum * var * (rows / max(rows - 1, 1))
    else:
        mean, var, rm_new, rv_new = rm, rv, rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * invstd
    z = xhat * gamma + beta
    rnorm = 1.0 / z.norm(dim=1).clamp_min(1e-12)
    u = z * rnorm[:, None]
    y = u * scale
    dz = scale * rnorm[:, None] * (dy - u * (u * dy).sum(1, keepdim=True))
    sum_dz = dz.sum(0); sum_dz_xhat = (dz * xhat).sum(0)
    v = dz
    if training:
        v = dz - sum_dz / rows - xhat * sum_dz_xhat / rows
    dx = gamma * invstd * v
    return dict(mean=mean, invstd=invstd, y=y, rnorm=rnorm, running_mean=rm_new, running_var=rv_new, dz=dz, sum_dz=sum_dz,
                sum_dz_xhat=sum_dz_xhat, abs_dz=dz.abs().sum(0), abs_dz_xhat=(dz * xhat).abs().sum(0), dx=dx)


def bn_neck_floor(x, gamma, beta, rm, rv, dy, training, eps=1e-5, momentum=0.1, scale=8.0):
    """The fp32 floor: F.batch_norm + F.normalize on the CPU and their autograd (torch.native_batch_norm is what F.batch_norm
    runs; it also returns the saved mean / invstd)."""
    x = x.clone().requires_grad_(True)
    rm2, rv2 = rm.clone(), rv.clone()
    z, smean, sinv = torch.native_batch_norm(x, gamma, beta, rm2, rv2, training, momentum, eps)
    if not training:
        smean, sinv = rm, 1.0 / torch.sqrt(rv + eps)
    z.retain_grad()
    y = torch.nn.functional.normalize(z, dim=1) * scale
    y.backward(dy)
    dz = z.grad
    xhat = (x.detach() - smean) * sinv
    return dict(mean=smean.detach(), invstd=sinv.detach(), y=y.detach(), rnorm=1.0 / z.detach().norm(dim=1).clamp_min(1e-12),
                running_mean=rm2, running_var=rv2, dz=dz, sum_dz=dz.sum(0), sum_dz_xhat=(dz * xhat).sum(0), dx=x.grad)


BN_SCALES = {'mean': 'elem', 'invstd': 'elem', 'running_mean': 'elem', 'running_var': 'elem', 'rnorm': 'elem', 'y': 'rows', 'dz': 'rows',
             'dx': 'rows', 'sum_dz': 'abs_dz', 'sum_dz_xhat': 'abs_dz_xhat'}


def bn_errors(got, ref):
    """Normalised error per BN-neck output of `got` (kernel or floor) against the fp64 `ref` of bn_neck_plain."""
    out = {}
    for k, kind in BN_SCALES.items():
        if k not in got:
            continue
        if kind == 'elem':
            out[k] = err_elems(got[k], ref[k])
        elif kind == 'rows':
            out[k] = err_rows(got[k], ref[k])
        else:
            out[k] = err_sums(got[k], ref[k], ref[kind])
    return out


def bn_stats_one_pass_f32(x):
    """numpy emulation of bn_stats_kernel + the one-pass finalize: fp32 sums of x and x^2 over four interleaved row lanes, then
    var = sqsum / n - mu^2 clamped at 0.  Returns (mean, var) in fp32."""
    x = np.asarray(x, dtype=np.float32)
    n, D = x.shape
    a = np.zeros((4, D), np.float32); b = np.zeros((4, D), np.float32)
    for r in range(n):
        a[r % 4] += x[r]; b[r % 4] += x[r] * x[r]
    s1 = ((a[0] + a[1]) + a[2]) + a[3]; s2 = ((b[0] + b[1]) + b[2]) + b[3]
    cnt = np.float32(n)
    mu = s1 / cnt
    return mu, np.maximum(s2 / cnt - mu * mu, np.float32(0))


def bn_stats_two_pass_f32(x):
    """Two passes, all in fp32: mu = sum / n, var = mean((x - mu)^2)."""
    x = np.asarray(x, dtype=np.float32)
    n, D = x.shape
    mu = bn_stats_one_pass_f32(x)[0]
    acc = np.zeros(D, np.float32)
    for r in range(n):
        d = x[r] - mu
        acc += d * d
    return mu, acc / np.float32(n)


def bn_stats_shifted_f64(x):
    """What the local form of reid_bnneck_fwd does: fp32 mu0 = sum / n, then delta = mean(x - mu0) and mean((x - mu0)^2) in fp64;
    mean = fp32(mu0 + delta), var = fp32(m2 - delta^2)."""
    x = np.asarray(x, dtype=np.float32)
    mu0 = bn_stats_one_pass_f32(x)[0].astype(np.float64)
    d = x.astype(np.float64) - mu0
    delta = d.mean(0)
    return (mu0 + delta).astype(np.float32), np.maximum((d * d).mean(0) - delta * delta, 0.0).astype(np.float32)


# ---- label-smoothed cross entropy ------------------------------------------------------------------------------------------------
def ce_plain(z, labels, valid, smoothing, grad_scale):
    """Per-row loss, its scale and dlogits in the dtype of `z`.  Rows with valid == 0 or a label outside [0, C) are unused: loss 0,
    gradient 0.  The scale of a row loss is the sum of the absolute values of the terms it adds up."""
    rows, C = z.shape
    ok = (labels >= 0) & (labels < C)
    if valid is not None:
        ok = ok & (valid != 0)
    lab = torch.where(ok, labels, torch.zeros_like(labels))
    mx = z.amax(1); lse = mx + torch.log(torch.exp(z - mx[:, None]).sum(1))
    zy = z.gather(1, lab.view(-1, 1)).squeeze(1)
    loss = (1 - smoothing) * (lse - zy) + smoothing * (lse - z.sum(1) / C)
    scale = lse.abs() + (1 - smoothing) * zy.abs() + smoothing * z.abs().sum(1) / C
    p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z); onehot.scatter_(1, lab.view(-1, 1), 1.0)
    d = grad_scale * (p - smoothing / C - (1 - smoothing) * onehot)
    okf = ok.to(z.dtype)
    return loss * okf, scale * okf, d * okf[:, None], ok


def ce_floor(z, labels, valid, smoothing, grad_scale):
    """fp32 floor: F.cross_entropy(label_smoothing=...) per row on the CPU, gradient by autograd."""
    rows, C = z.shape
    ok = (labels >= 0) & (labels < C)
    if valid is not None:
        ok = ok & (valid != 0)
    zr = z.clone().requires_grad_(True)
    loss = torch.zeros(rows, dtype=z.dtype)
    if bool(ok.any()):
        l = torch.nn.functional.cross_entropy(zr[ok], labels[ok], label_smoothing=smoothing, reduction='none')
        (l.sum() * grad_scale).backward()
        loss[ok] = l.detach()
    d = zr.grad if zr.grad is not None else torch.zeros_like(z)
    return loss, d


# ---- SDM ---------------------------------------------------------------------------------------------------------------------
def _sdm_side(S, y):
    """(mean CE over the rows with a positive, scale) of one direction: CE_i = lse_i - mean over positives of S_ij."""
    has = y.sum(1) > 0
    if not bool(has.any()):
        z = torch.zeros((), dtype=S.dtype)
        return z, z
    Sv = S[has].clamp(-20.0, 20.0); pos = y[has]
    w = pos / pos.sum(1, keepdim=True)
    lse = torch.logsumexp(Sv, dim=1)
    tgt = (w * Sv).sum(1)
    return (lse - tgt).mean(), (lse.abs() + (w * Sv.abs()).sum(1)).mean()


def sdm_plain(q, g, y, tau, eps=1e-8):
    """sdm_loss_stable written plainly in the dtype of q (no cast inside, unlike oracle.reid_oracle.sdm_loss): returns (loss, scale),
    scale = the sum of the absolute values of the terms the loss adds up."""
    t = max(0.15, min(0.5, tau))
    qn = q / q.norm(dim=1, keepdim=True).clamp_min(eps)
    gn = g / g.norm(dim=1, keepdim=True).clamp_min(eps)
    S = qn @ gn.t() / t
    y = y.to(q.dtype)
    if not bool((y.sum(1) > 0).any()):
        z = torch.zeros((), dtype=q.dtype)
        return z + 0.0 * (q.sum() + g.sum()), z
    a, sa = _sdm_side(S, y); b, sb = _sdm_side(S.t(), y.t())
    return 0.5 * (a + b), (0.5 * (sa + sb)).detach()


# ---- AP / CMC ----------------------------------------------------------------------------------------------------------------
MAX_POS = 8192


def rank_metrics_ref(scores, g_pid, q_pid, g_img=None, excl=None, has_slot=True):
    """(ap, rank1, npos) of one query by a walk of the stable descending argsort of its fp32 score row, in fp64.
    Gallery rows whose image id (>= 0) is one of `excl` are removed from the positives and, as non-positives, rank last (they
    precede no positive).  No positive: (0, 0, 0); more than 8192: (0, 0, -1); has_slot False = the pid has no gallery row."""
    s = np.asarray(scores, dtype=np.float32)
    g_pid = np.asarray(g_pid)
    dropped = np.zeros(s.shape[0], bool)
    if g_img is not None and excl is not None:
        ids = [int(e) for e in excl if int(e) >= 0]
        gi = np.asarray(g_img)
        if ids:
            dropped = (gi >= 0) & np.isin(gi, ids)
    pos = (g_pid == q_pid) & ~dropped
    if not has_slot:
        pos[:] = False
    npos = int(pos.sum())
    if npos == 0:
        return 0.0, 0, 0
    if npos > MAX_POS:
        return 0.0, 0, -1
    order = np.argsort(-s.astype(np.float64), kind='stable')       # score descending, index ascending on ties
    walk = order[~dropped[order]]
    ranks = np.nonzero(pos[walk])[0].astype(np.float64) + 1.0
    ap = float(np.sum(np.arange(1, npos + 1, dtype=np.float64) / ranks) / npos)
    return ap, int(ranks[0]), npos
