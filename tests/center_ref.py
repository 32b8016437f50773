"""Reference of the center loss (include/reid_hip.h, reid_center_*).  It shares no code with the package.

Two forms:
  (a) a float32 numpy LOOP over rows and classes that performs the operations of the definition in the stated order, every operation
      rounded to float32 on its own -- diff, the centres after an update and dx must equal the kernels' BIT FOR BIT (element-wise
      chains with a fixed order);
  (b) an fp64 torch form: loss = 0.5 * sum |x - c_y|^2 / n with its autograd gradient, Wen's update as a dense one-hot product.

Bounds against (b), u = 2^-24: d2 is a sum of D non-negative fp32 terms, each the rounded square of a rounded difference, so
|d2 - d2_64| <= (D + 3) u d2_64 whatever the summation order (2 u from the difference, 1 u from the square, D - 1 additions, and the
second-order terms); the loss adds the conversion of every d2 (exact), an fp64 sum, and the final rounding: (D + 5) u relative.
"""
import numpy as np
import torch

U = 2.0 ** -24
F = np.float32
# (S, N, D, C, pad): the smallest shapes that take each path -- one row, one class; one lane of the wave holds the whole row; a second
# 16-byte chunk in one lane only, with a padded leading dimension; the most sides, 297 rows: the update's 64-row ballots and the
# finalize kernel's 256-row pieces both take a second round; two full chunks per lane; the widest row (four chunks per lane), 40 classes
SHAPES = [(1, 1, 4, 1, 0), (1, 7, 4, 3, 0), (2, 5, 260, 4, 4), (9, 33, 64, 5, 0), (5, 16, 512, 6, 0), (1, 64, 1024, 40, 0)]
STEPS = 6


def d2_bound(D):
    return (D + 3) * U


def loss_bound(D):
    return (D + 5) * U


def make_case(S, N, D, C, seed):
    """(x [S, N, D] f32, labels [N] i64, valid [S, N] u8, centers [C, D] f32) on the CPU.  Labels repeat within a side (N > C) and, being
    shared, across the sides; from N = 5 on one label is -1 and one is C (out of range); validity bytes are 0, 1, 2 or 255."""
    g = torch.Generator().manual_seed(1000 + seed)
    labels = torch.arange(N)[torch.randperm(N, generator=g)] % C
    if N >= 5:
        labels[1] = -1; labels[3] = C
    means = torch.randn(C + 1, D, generator=g)
    x = (means[labels.clamp(0, C)][None] + 0.5 * torch.randn(S, N, D, generator=g)).float()
    valid = torch.tensor([1, 1, 1, 0, 255, 2], dtype=torch.uint8)[torch.randint(0, 6, (S, N), generator=g)]
    if N == 1:
        valid[:] = 1
    elif N >= 5:
        valid[0, 0] = 0; valid[-1, 2] = 255; valid[0, 4] = 1          # mixed whatever was drawn; row 4 of side 0 is always used
    centers = (means[:C] + 0.3 * torch.randn(C, D, generator=g)).float()
    return x, labels.long(), valid, centers


def stream_step(S, N, D, C, s):
    """Batch s of the stream: make_case with its own seed, labels rotated so that every batch misses some classes."""
    x, labels, valid, _ = make_case(S, N, D, C, 50 + s)
    if C > 2:
        labels = torch.where((labels >= 0) & (labels < C) & (labels % C == s % C), (labels + 1) % C, labels)     # class s % C is absent
    return x, labels, valid


def used_rows(labels, valid, S, C):
    """bool [S*N]: valid and 0 <= label < C."""
    lab = np.tile(np.asarray(labels, dtype=np.int64), S)
    ok = (lab >= 0) & (lab < C)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    return ok


# ------------------------------------------------------------------------------------------------------------ (a) float32 loop
def loop_forward(x, labels, valid, centers):
    """x [S, N, D]; returns dict(diff [S*N, D] f32, d2 [S*N] f32, used bool [S*N], loss f32, n_used int)."""
    x = np.asarray(x, dtype=F); c = np.asarray(centers, dtype=F)
    S, N, D = x.shape
    x = x.reshape(S * N, D)
    lab = np.asarray(labels, dtype=np.int64)
    used = used_rows(labels, valid, S, c.shape[0])
    diff = np.zeros((S * N, D), dtype=F); d2 = np.zeros(S * N, dtype=F)
    total, n = 0.0, 0
    with np.errstate(all='ignore'):
        for r in range(S * N):
            if not used[r]:
                continue
            diff[r] = x[r] - c[lab[r % N]]
            d2[r] = np.sum(diff[r] * diff[r], dtype=F)
            total += float(d2[r]); n += 1                             # ascending row order, fp64
        loss = F(0.5 * total / max(1, n))
    return dict(diff=diff, d2=d2, used=used, loss=loss, n_used=n)


def loop_update(diff, d2, labels, used, centers, alpha):
    """The centres after Wen's update, float32 operation by operation; rows of classes without a contributing row keep their bits."""
    c = np.array(centers, dtype=F, copy=True)
    lab = np.asarray(labels, dtype=np.int64)
    N, alpha = lab.shape[0], F(alpha)
    contributes = used & np.isfinite(d2)
    with np.errstate(all='ignore'):
        for j in range(c.shape[0]):
            rows = [r for r in range(diff.shape[0]) if contributes[r] and lab[r % N] == j]
            if not rows:
                continue
            acc = np.zeros(c.shape[1], dtype=F)
            for r in rows:
                acc = acc + (-diff[r])
            delta = acc / F(1 + len(rows))
            c[j] = c[j] - alpha * delta
    return c


def loop_backward(diff, used, n_used, dloss):
    coef = F(dloss) / max(F(1.0), F(n_used))
    with np.errstate(all='ignore'):
        dx = (coef * diff).astype(F)
    dx[~used] = 0
    return dx


# ------------------------------------------------------------------------------------------------------------ (b) fp64 torch
def ref64_loss(x, labels, valid, centers):
    """(loss, n_used, d2 [S*N]) in fp64; differentiable in x [S, N, D]."""
    S, N, D = x.shape
    C = centers.shape[0]
    used = torch.from_numpy(used_rows(labels.cpu(), None if valid is None else valid.cpu(), S, C)).to(x.device)
    lab = labels.repeat(S).clamp(0, C - 1)
    d = x.double().reshape(S * N, D) - centers.double()[lab]
    d2 = torch.where(used, (d * d).sum(1), torch.zeros((), dtype=torch.float64, device=x.device))
    n = int(used.sum())
    return 0.5 * d2.sum() / max(1, n), n, d2


def ref64_update(x, labels, valid, centers, alpha):
    """Wen's eq. 4 as a dense one-hot product in fp64; rows whose squared distance is not finite do not contribute."""
    S, N, D = x.shape
    C = centers.shape[0]
    c = centers.double()
    _, _, d2 = ref64_loss(x, labels, valid, centers)
    used = torch.from_numpy(used_rows(labels.cpu(), None if valid is None else valid.cpu(), S, C)).to(x.device) & torch.isfinite(d2)
    lab = labels.repeat(S).clamp(0, C - 1)
    onehot = torch.zeros(S * N, C, dtype=torch.float64, device=x.device)
    onehot[torch.arange(S * N, device=x.device), lab] = 1.0
    onehot = onehot * used[:, None]
    xs = torch.where(used[:, None], x.double().reshape(S * N, D), torch.zeros((), dtype=torch.float64, device=x.device))
    cnt = onehot.sum(0)                                               # n_j
    delta = (cnt[:, None] * c - onehot.t() @ xs) / (1.0 + cnt)[:, None]      # sum over the rows of class j of (c_j - x)
    return c - float(alpha) * delta


# ------------------------------------------------------------------------------------------------------------ argument checks
def violations(S=2, N=5, D=8, C=4):
    """(entry point, overrides of its good arguments, text its message must hold): one per violated requirement."""
    out = []
    for k, v, text in (('S', 0, 'S='), ('S', 10, 'S='), ('N', 0, 'N='), ('N', 8193, 'N='), ('D', 6, 'D='), ('D', 0, 'D='), ('D', 1028, 'D=')):
        out += [(e, {k: v}, text) for e in ('fwd', 'update', 'bwd', 'ws')]
    for e in ('fwd', 'update'):
        out += [(e, {'C': 0}, 'C='), (e, {'C': 2 ** 31 // D, 'D': D}, 'C * D')]
    out += [('fwd', {'ldx': D - 4}, 'ldx'), ('fwd', {'ldx': D + 2}, 'ldx'), ('bwd', {'lddx': D - 4}, 'lddx'), ('bwd', {'lddx': D + 1}, 'lddx'),
            ('fwd', {'S': 9, 'N': 8192, 'ldx': 2 ** 15}, '2^31'), ('bwd', {'S': 9, 'N': 8192, 'lddx': 2 ** 15}, '2^31'),
            ('update', {'alpha': float('nan')}, 'alpha'), ('update', {'alpha': float('inf')}, 'alpha'),
            ('fwd', {'x': 4}, 'aligned'), ('fwd', {'centers': 8}, 'aligned'), ('fwd', {'ws': 4}, 'aligned'), ('update', {'centers': 4}, 'aligned'),
            ('update', {'ws': 12}, 'aligned'), ('bwd', {'ws': 4}, 'aligned'), ('bwd', {'dx': 8}, 'aligned')]
    for e, names in (('fwd', ('x', 'labels', 'centers', 'ws', 'd2', 'result')), ('update', ('labels', 'd2', 'ws', 'centers')),
                     ('bwd', ('ws', 'result', 'dloss', 'dx'))):
        out += [(e, {n: None}, 'null') for n in names]
    return out


def call(h, entry, a):
    """Calls entry point ``entry`` of the bound library ``h`` with the argument dict ``a`` (pointers as integers or None)."""
    if entry == 'ws':
        return h.reid_center_ws_floats(a['S'], a['N'], a['D'])
    if entry == 'fwd':
        return h.reid_center_fwd(a['x'], a['ldx'], a['labels'], a['valid'], a['S'], a['N'], a['D'], a['centers'], a['C'], a['ws'], a['d2'],
                                 a['result'], a['stream'])
    if entry == 'update':
        return h.reid_center_update(a['labels'], a['valid'], a['S'], a['N'], a['D'], a['d2'], a['ws'], a['centers'], a['C'], a['alpha'], a['stream'])
    return h.reid_center_bwd(a['S'], a['N'], a['D'], a['ws'], a['result'], a['dloss'], a['dx'], a['lddx'], a['stream'])


def bad_arguments(good, over):
    """``good`` with the overrides; an integer override of a pointer is a byte offset from the good pointer (misalignment)."""
    a = dict(good)
    for k, v in over.items():
        a[k] = good[k] + v if k in ('x', 'centers', 'ws', 'dx') and v is not None else v
    return a
