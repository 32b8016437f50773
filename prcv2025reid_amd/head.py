"""Autograd boundaries of the head kernels: BN-neck, classifier, label-smoothed CE, SDM loss, batch-hard triplet loss, cross-modal
batch-hard triplet loss, cosine-margin identity heads, center loss.

Reference: BNNeck.forward models/model.py:208-224; compute_loss :512-659; sdm_loss_stable
models/sdm_loss.py:13-149.  All arithmetic is in libreid_hip.so (fp32); torch only carries the tensors.
"""
import math

import torch

from . import _lib, ops


class BNNeckFn(torch.autograd.Function):
    """y = 8 * normalize(BatchNorm1d(x)); batch statistics in training (running stats updated in place)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training: bool, momentum: float, eps: float):
        x = x.contiguous().float()
        B, D = x.shape
        dev = x.device
        s1 = torch.empty(D, device=dev); s2 = torch.empty(D, device=dev)
        y = torch.empty(B, D, device=dev)
        mean = torch.empty(D, device=dev); invstd = torch.empty(D, device=dev); rn = torch.empty(B, device=dev)
        if training:
            ops.bnneck_stats(x, s1, s2)
        ops.bnneck_fwd(x, gamma.detach(), beta.detach(), running_mean, running_var, s1, s2, float(B), training, y, None, mean,
                       invstd, rn, eps=eps, momentum=momentum, scale=8.0)
        ctx.save_for_backward(x, gamma.detach(), beta.detach(), mean, invstd, rn)
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd, rn = ctx.saved_tensors
        B, D = x.shape
        dev = x.device
        dy = dy.contiguous().float()
        dz = torch.empty(B, D, device=dev); a = torch.empty(D, device=dev); b = torch.empty(D, device=dev)
        dx = torch.empty(B, D, device=dev)
        ops.bnneck_bwd_p1(dy, x, gamma, beta, mean, invstd, rn, dz, a, b, scale=8.0)
        ops.bnneck_bwd_p2(dz, x, gamma, mean, invstd, a, b, float(B), ctx.training, dx)
        return dx, b, a, None, None, None, None, None


class LinearF32Fn(torch.autograd.Function):
    """y = x @ W.T (+ bias) in exact fp32 (vector-ALU GEMM); used for the identity classifier."""

    @staticmethod
    def forward(ctx, x, W, bias):
        x = x.contiguous().float()
        y = torch.empty(x.shape[0], W.shape[0], device=x.device)
        ops.sgemm(x, W.detach(), y, tb=True, bias=None if bias is None else bias.detach())
        ctx.save_for_backward(x, W.detach())
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous().float()
        dx = dW = db = None                                   # only what autograd asks for (frozen weights cost nothing)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ops.sgemm(dy, W, dx)                              # [B,C] @ [C,D]
        if ctx.needs_input_grad[1]:
            dW = torch.empty_like(W)
            ops.sgemm(dy, x, dW, ta=True)                     # [C,B] @ [B,D]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dW, db


class CrossEntropyLSFn(torch.autograd.Function):
    """Mean over valid rows of label-smoothed CE; returns (loss, count) with count a float tensor."""

    @staticmethod
    def forward(ctx, logits, labels, valid, smoothing: float):
        logits = logits.contiguous().float()
        acc = torch.zeros(2, device=logits.device)
        ops.ce_ls_fwd(logits, labels, valid, None, acc, smoothing)
        cnt = acc[1]
        loss = acc[0] / cnt.clamp_min(1.0)
        ctx.save_for_backward(logits, labels, valid, cnt)
        ctx.smoothing = smoothing
        ctx.mark_non_differentiable(cnt)
        return loss, cnt

    @staticmethod
    def backward(ctx, dloss, _dcnt):
        logits, labels, valid, cnt = ctx.saved_tensors
        gs = (dloss / cnt.clamp_min(1.0)).reshape(1).float().contiguous()
        dl = torch.empty_like(logits)
        ops.ce_ls_bwd(logits, labels, valid, gs, dl, ctx.smoothing)
        return dl, None, None, None


class SDMFn(torch.autograd.Function):
    """(losses [P], contributes [P]) of sdm_loss_stable between P stacked modality feature sets q [P, N, D] and the vis features
    g [Mg, D] -- the fused kernel of csrc/sdm.hip: all pairs in one launch, no [N, Mg] matrix in memory."""

    @staticmethod
    def forward(ctx, q, g, q_label, g_label, q_valid, g_valid, tau: float):
        P, N, D = q.shape
        q2 = q.reshape(P * N, D).contiguous().float(); g = g.contiguous().float()
        ws = torch.empty(ops.sdm_ws_floats(P, N, g.shape[0], D), device=q.device)
        res = torch.zeros(2 * P, device=q.device)
        qv = None if q_valid is None else q_valid.reshape(P * N).contiguous()
        ops.sdm_fwd(q2, g, q_label, g_label, qv, g_valid, tau, ws, res, P=P)
        ctx.save_for_backward(q2, g, q_label, g_label, qv, g_valid, ws)
        ctx.tau, ctx.P = tau, P
        res = res.view(P, 2)
        loss, flag = res[:, 0].contiguous(), res[:, 1].contiguous()
        ctx.mark_non_differentiable(flag)
        return loss, flag

    @staticmethod
    def backward(ctx, dloss, _dflag):
        q2, g, ql, gl, qv, gv, ws = ctx.saved_tensors
        P = ctx.P
        dq = torch.zeros_like(q2); dg = torch.zeros_like(g)
        ops.sdm_bwd(q2, g, ql, gl, qv, gv, ctx.tau, ws, dloss.reshape(P).float().contiguous(), dq, dg, P=P)
        return dq.view(P, q2.shape[0] // P, q2.shape[1]), dg, None, None, None, None, None


EPS = 1e-12                                                   # of the triplet losses' unit rows: F.normalize's default


def _margin_arg(fn, margin):
    """The kernels' margin: None (the soft-margin form) -> -1.0."""
    if margin is not None and float(margin) < 0:
        raise ValueError(f'{fn.__name__}: margin must be >= 0, or None for the soft-margin form')
    return -1.0 if margin is None else float(margin)


def _two_sided_prepare(q, g, q_valid):
    """q [P, N, D], g [Mg, D], q_valid [P, N] or None as the two-sided kernels take them: (q2 [P*N, D], g, qv [P*N], res [P, 4])."""
    P, N, D = q.shape
    q2 = q.reshape(P * N, D).contiguous().float()
    return q2, g.contiguous().float(), None if q_valid is None else q_valid.reshape(P * N).contiguous(), torch.empty(P, 4, device=q.device)


def _two_sided_results(ctx, res):
    """(loss, flag, n_active) of res [P, 4]; only the loss is differentiable."""
    loss, flag, n_active = res[:, 0].contiguous(), res[:, 1].contiguous(), res[:, 2:].contiguous()
    ctx.mark_non_differentiable(flag, n_active)
    return loss, flag, n_active


def _gscale(dloss, P):                                        # (a copy: the cotangent of L.sum() is an expanded scalar with stride 0)
    return torch.empty(P, device=dloss.device).copy_(dloss.reshape(P))


def _two_sided_args(who, q, g, q_labels, g_labels, q_valid, g_valid):
    """The public two-sided functions' argument checks; returns q as [P, N, D] and the validity vectors as the kernels take them."""
    tensors = (q, g, q_labels, g_labels) + tuple(t for t in (q_valid, g_valid) if t is not None)
    if not all(t.is_cuda for t in tensors):
        raise _lib.ReidHipError(f'{who} needs device tensors (there is no CPU path)')
    if q.dim() == 2:
        q = q.unsqueeze(0)
    if q.dim() != 3 or g.dim() != 2 or g.shape[1] != q.shape[2] or q_labels.shape != q.shape[1:2] or g_labels.shape != g.shape[:1]:
        raise ValueError(f'{who}: q [P, N, D] or [N, D], g [Mg, D], q_labels [N], g_labels [Mg]')
    return (q, None if q_valid is None else q_valid.to(torch.uint8).reshape(q.shape[0], q.shape[1]).contiguous(),
            None if g_valid is None else g_valid.to(torch.uint8).contiguous())


class TripletHardFn(torch.autograd.Function):
    """(loss, n_active) of the batch-hard triplet loss of x [B, D] (csrc/triplet.hip; the reference has no such loss).  ``margin`` None:
    the soft-margin form softplus(d_ap - d_an).  n_active is a float tensor; nothing is read back to the host.  ``rows_out``: an optional
    trailing dict that receives COPIES of the per-row arrays ``d_ap``, ``d_an``, ``idx_p``, ``idx_n`` (batch_hard_triplet); the call the
    model makes is ``apply(x, labels, valid, margin)``."""

    @staticmethod
    def forward(ctx, x, labels, valid, margin, rows_out=None):
        m = _margin_arg(TripletHardFn, margin)
        x = x.contiguous().float()
        B, dev = x.shape[0], x.device
        fl = torch.empty(3, B, device=dev); ix = torch.empty(2, B, dtype=torch.int32, device=dev)      # d_ap | d_an | row_loss, idx_p | idx_n
        res = torch.empty(2, device=dev)
        labels = labels.contiguous()
        ops.triplet_hard_fwd(x, labels, valid, m, fl[0], fl[1], ix[0], ix[1], fl[2], res)
        ctx.save_for_backward(x, fl, ix, res)
        ctx.margin = m
        loss, n_active = res[0], res[1]
        ctx.mark_non_differentiable(n_active)
        if rows_out is not None:
            flc, ixc = fl[:2].clone(), ix.clone()          # copies: the saved arrays belong to the backward
            rows_out.update(d_ap=flc[0], d_an=flc[1], idx_p=ixc[0], idx_n=ixc[1])
        return loss, n_active

    @staticmethod
    def backward(ctx, dloss, _dn):
        x, fl, ix, res = ctx.saved_tensors
        dx = torch.empty_like(x)
        ops.triplet_hard_bwd(x, ctx.margin, fl[0], fl[1], ix[0], ix[1], res, dloss.reshape(1).float().contiguous(), dx)
        return dx, None, None, None, None


def batch_hard_triplet(features, labels, valid=None, margin=0.3):
    """Batch-hard triplet loss of ``features`` [B, D] for users with their own loop: hardest positive / negative per anchor by the
    Euclidean distance (difference form, fp32), mean over the active anchors.  ``valid``: optional bool / uint8 [B], rows that take part;
    ``margin`` None: soft margin.  The features are NOT L2-normalised here.  Returns (loss, LazyCount(n_active), {'d_ap', 'd_an',
    'idx_p', 'idx_n'}); the loss carries the gradient to ``features``."""
    from .model import LazyCount
    if not (features.is_cuda and labels.is_cuda and (valid is None or valid.is_cuda)):
        raise _lib.ReidHipError('batch_hard_triplet needs device tensors (there is no CPU path)')
    if features.dim() != 2 or labels.shape != features.shape[:1]:
        raise ValueError('batch_hard_triplet: features [B, D], labels [B]')
    if valid is not None:
        valid = valid.to(torch.uint8).contiguous()
    rows = {}
    loss, n_active = TripletHardFn.apply(features, labels.long(), valid, margin, rows)
    return loss, LazyCount(n_active), rows


class CrossTripletFn(torch.autograd.Function):
    """(loss [P], flag [P], n_active [P, 2]) of the cross-modal batch-hard triplet loss between P stacked modality feature sets
    q [P, N, D] and the vis features g [Mg, D] (csrc/cross_triplet.hip; the reference has no such loss): unit rows, difference-form
    distances, hardest positive / negative in both directions, L_p the mean of the two directions' means.  ``margin`` None: the
    soft-margin form.  n_active = (q->g, g->q) active anchors as floats; nothing is read back to the host.  ``rows_out``: an optional
    trailing dict that receives COPIES of the saved arrays (cross_modal_triplet); the call the model makes is
    ``apply(q, g, q_label, g_label, q_valid, g_valid, margin, normalize)``."""
    @staticmethod
    def forward(ctx, q, g, q_label, g_label, q_valid, g_valid, margin, normalize: bool, rows_out=None):
        m = _margin_arg(CrossTripletFn, margin)
        (P, N, D), Mg, dev = q.shape, g.shape[0], q.device
        q2, g, qv, res = _two_sided_prepare(q, g, q_valid)
        ws = torch.empty(ops.cross_triplet_ws_floats(P, N, Mg, D), device=dev)
        qd = torch.empty(2, P * N, device=dev); qi = torch.empty(2, P * N, dtype=torch.int32, device=dev)
        gd = torch.empty(2, P * Mg, device=dev); gi = torch.empty(2, P * Mg, dtype=torch.int32, device=dev)
        ops.cross_triplet_fwd(q2, g, q_label.contiguous(), g_label.contiguous(), qv, g_valid, m, normalize, EPS, qd, qi, gd, gi, ws, res, P=P)
        ctx.save_for_backward(q2, g, qv, g_valid, qd, qi, gd, gi, ws, res)
        ctx.margin, ctx.normalize, ctx.P = m, bool(normalize), P
        loss, flag, n_active = _two_sided_results(ctx, res)
        if rows_out is not None:                              # copies: the saved arrays belong to the backward
            rows_out.update(q_d_ap=qd[0].view(P, N).clone(), q_d_an=qd[1].view(P, N).clone(), q_idx_p=qi[0].view(P, N).clone(),
                            q_idx_n=qi[1].view(P, N).clone(), g_d_ap=gd[0].view(P, Mg).clone(), g_d_an=gd[1].view(P, Mg).clone(),
                            g_idx_p=gi[0].view(P, Mg).clone(), g_idx_n=gi[1].view(P, Mg).clone())
        return loss, flag, n_active

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):
        q2, g, qv, gv, qd, qi, gd, gi, ws, res = ctx.saved_tensors
        P = ctx.P
        dq = torch.empty_like(q2); dg = torch.empty_like(g)
        ops.cross_triplet_bwd(q2, g, qv, gv, ctx.margin, ctx.normalize, EPS, qd, qi, gd, gi, ws, res, _gscale(dloss, P), dq, dg, P=P)
        return dq.view(P, q2.shape[0] // P, q2.shape[1]), dg, None, None, None, None, None, None, None


def cross_modal_triplet(q, g, q_labels, g_labels, q_valid=None, g_valid=None, margin=0.3, normalize=True):
    """Cross-modal batch-hard triplet loss for users with their own loop: ``q`` [P, N, D] (P query modalities stacked; [N, D] = one)
    against the vis features ``g`` [Mg, D].  Per pair, every valid q row mines its hardest positive / negative among the g rows and
    every valid g row among the pair's q rows (Euclidean distance of the unit rows, difference form, fp32; no self-exclusion);
    L_p = 0.5 * (mean over the active q anchors + mean over the active g anchors).  ``q_valid`` [P, N] / ``g_valid`` [Mg]: optional
    bool / uint8, rows that take part; ``margin`` None: soft margin; ``normalize`` False: the rows are used as they are.  Returns
    (losses [P], flags [P], rows): flag 1 where the pair has an active anchor, rows = {'q_d_ap', 'q_d_an', 'q_idx_p', 'q_idx_n'} [P, N]
    and {'g_d_ap', 'g_d_an', 'g_idx_p', 'g_idx_n'} [P, Mg] (g indices into 0..N-1) plus 'n_active' [P, 2]; the losses carry the
    gradient to ``q`` and ``g``."""
    q, q_valid, g_valid = _two_sided_args('cross_modal_triplet', q, g, q_labels, g_labels, q_valid, g_valid)
    rows = {}
    loss, flag, n_active = CrossTripletFn.apply(q, g, q_labels.long(), g_labels.long(), q_valid, g_valid, margin, bool(normalize), rows)
    rows['n_active'] = n_active
    return loss, flag, rows


class HcTripletFn(torch.autograd.Function):
    """(loss [P], flag [P], n_active [P, 2]) of the hetero-center triplet loss between P stacked modality feature sets q [P, N, D] and
    the vis features g [Mg, D] (csrc/hc_triplet.hip; the reference has no such loss): unit rows, per-identity centres of every side,
    the triplet on the centres of [pair p's q centres | g centres].  ``margin`` None: the soft-margin form.  n_active = active anchors
    among the (q, g) centres as floats; nothing is read back to the host.  ``rows_out``: an optional trailing dict that receives COPIES
    of the saved arrays (hetero_center_triplet); the call the model makes is
    ``apply(q, g, q_label, g_label, q_valid, g_valid, margin, normalize)``."""
    @staticmethod
    def forward(ctx, q, g, q_label, g_label, q_valid, g_valid, margin, normalize: bool, rows_out=None):
        m = _margin_arg(HcTripletFn, margin)
        (P, N, D), Mg, dev = q.shape, g.shape[0], q.device
        q2, g, qv, res = _two_sided_prepare(q, g, q_valid)
        R, U = P * N + Mg, N + Mg
        ws = torch.empty(ops.hc_triplet_ws_floats(P, N, Mg, D), device=dev)
        ints = torch.empty(2, R, dtype=torch.int32, device=dev)                                  # lead | count
        clabel = torch.empty(R, dtype=torch.int64, device=dev)
        d = torch.empty(2, P, U, device=dev); idx = torch.empty(2, P, U, dtype=torch.int32, device=dev)
        ops.hc_triplet_fwd(q2, g, q_label.contiguous(), g_label.contiguous(), qv, g_valid, m, normalize, EPS,
                           ints[0], ints[1], clabel, d, idx, ws, res, P=P)
        ctx.save_for_backward(q2, g, ints, ws, res)
        ctx.margin, ctx.normalize, ctx.P = m, bool(normalize), P
        loss, flag, n_active = _two_sided_results(ctx, res)
        if rows_out is not None:                              # copies: the saved arrays belong to the backward
            for side, rows, slots in (('q', slice(0, P * N), slice(0, N)), ('g', slice(P * N, R), slice(N, U))):
                shape = (P, N) if side == 'q' else (Mg,)
                rows_out.update({f'{side}_lead': ints[0, rows].reshape(shape).clone(), f'{side}_count': ints[1, rows].reshape(shape).clone(),
                                 f'{side}_label': clabel[rows].reshape(shape).clone(),
                                 f'{side}_d_ap': d[0, :, slots].clone(), f'{side}_d_an': d[1, :, slots].clone(),
                                 f'{side}_idx_p': idx[0, :, slots].clone(), f'{side}_idx_n': idx[1, :, slots].clone()})
        return loss, flag, n_active

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):
        q2, g, ints, ws, res = ctx.saved_tensors
        P = ctx.P
        dq = torch.empty_like(q2); dg = torch.empty_like(g)
        ops.hc_triplet_bwd(q2, g, ctx.margin, ctx.normalize, EPS, ints[0], ints[1], ws, res, _gscale(dloss, P), dq, dg, P=P)
        return dq.view(P, q2.shape[0] // P, q2.shape[1]), dg, None, None, None, None, None, None, None


def hetero_center_triplet(q, g, q_labels, g_labels, q_valid=None, g_valid=None, margin=0.3, normalize=True):
    """Hetero-center triplet loss (Zhu et al. 2020; Liu et al. 2020) for users with their own loop: ``q`` [P, N, D] (P query modalities
    stacked; [N, D] = one) against the vis features ``g`` [Mg, D].  On every side the valid rows of one label are averaged into a centre
    (of the unit rows; ``normalize`` False: of the rows as they are); per pair, every centre of [q centres | g centres] is an anchor, its
    positive the centre of the other side with its label, its negative the nearest centre of another label from either side
    (difference form, fp32, ties to the lowest index); L_p = mean over the active anchors.  ``q_valid`` [P, N] / ``g_valid`` [Mg]:
    optional bool / uint8, rows that take part; ``margin`` None: soft margin.  Returns (losses [P], flags [P], rows): flag 1 where the
    pair has an active anchor; rows = {'q_lead' [P, N], 'g_lead' [Mg]} (the centre slot of a row, -1: invalid), {'q_count', 'q_label'
    [P, N], 'g_count', 'g_label' [Mg]} per centre slot (count 0 behind the side's centres), {'q_d_ap', 'q_d_an', 'q_idx_p', 'q_idx_n'}
    [P, N] and {'g_d_ap', 'g_d_an', 'g_idx_p', 'g_idx_n'} [P, Mg] per centre slot, indices in 0..N+Mg-1 (q centre s = s, g centre t =
    N + t), plus 'n_active' [P, 2]; the losses carry the gradient to ``q`` and ``g``."""
    q, q_valid, g_valid = _two_sided_args('hetero_center_triplet', q, g, q_labels, g_labels, q_valid, g_valid)
    rows = {}
    loss, flag, n_active = HcTripletFn.apply(q, g, q_labels.long(), g_labels.long(), q_valid, g_valid, margin, bool(normalize), rows)
    rows['n_active'] = n_active
    return loss, flag, rows


class CrossBatchMemory:
    """The ring of xbm_cross_triplet (Wang et al., "Cross-Batch Memory for Embedding Learning", CVPR 2020; csrc/xbm.hip): the rows of
    the last ``capacity`` instances of every side (side 0 = vis, 1 .. sides-1 = the non-vis modalities), their labels and validity
    bytes, and a DEVICE-side cursor (next slot, rows ever written) that the enqueue kernels read and advance -- no host-side counter
    takes part, so a captured graph keeps filing rows where its last replay stopped.  Plain tensors, not parameters or buffers: a
    memory is not part of a state_dict, a resumed run refills it."""

    def __init__(self, capacity, sides, dim, device='cuda'):
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.ReidHipError('CrossBatchMemory needs device tensors (there is no CPU path)')
        if not (1 <= capacity <= 8192 and 2 <= sides <= 9 and dim % 4 == 0 and 4 <= dim <= 1024):
            raise ValueError('CrossBatchMemory: capacity 1..8192, sides 2..9 (vis + 1..8 modalities), dim a multiple of 4 in 4..1024')
        self.capacity, self.sides, self.dim = int(capacity), int(sides), int(dim)
        self.rows = torch.zeros(sides, capacity, dim, device=device)
        self.labels = torch.zeros(capacity, dtype=torch.int64, device=device)
        self.valid = torch.zeros(sides, capacity, dtype=torch.uint8, device=device)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=device)

    def reset(self):
        """Empties the memory (device fills only)."""
        for t in (self.rows, self.labels, self.valid, self.cursor):
            t.zero_()

    @property
    def rows_written(self):
        """Rows ever enqueued per side, read from the device when someone looks at it."""
        from .model import LazyCount
        return LazyCount(self.cursor[1])

    @property
    def filled(self):
        """Slots that hold a row (valid or not), read from the device when someone looks at it."""
        from .model import LazyCount
        return LazyCount(self.cursor[1].clamp(max=self.capacity))


class XbmTripletFn(torch.autograd.Function):
    """(loss [P], flag [P], n_active [P, 2]) of the cross-modal batch-hard triplet loss with a cross-batch memory (csrc/xbm.hip; the
    reference has no such loss): with ``enqueue`` the batch q [P, N, D], g [N, D] is first filed into ``memory`` (unit rows when
    ``normalize``), then every valid q row of pair p mines the slots of memory side 0 and every valid g row the slots of side p + 1 by
    the rules of CrossTripletFn; indices are slot numbers.  The memory's rows are constants: the gradient reaches the anchors only, from
    copies of the kept rows the forward puts into its workspace (the ring may be overwritten before the backward runs).  ``rows_out``:
    an optional trailing dict that receives COPIES of the saved arrays (xbm_cross_triplet); the call the model makes is
    ``apply(q, g, labels, q_valid, g_valid, memory, margin, normalize, enqueue)``."""
    @staticmethod
    def forward(ctx, q, g, labels, q_valid, g_valid, memory, margin, normalize: bool, enqueue: bool, rows_out=None):
        m = _margin_arg(XbmTripletFn, margin)
        (P, N, D), dev = q.shape, q.device
        if g.shape[0] != N or P + 1 != memory.sides:
            raise ValueError(f'XbmTripletFn: q [P, N, D] and g [N, D] with P + 1 = {memory.sides} sides of the memory')
        if N > memory.capacity:
            raise ValueError(f'XbmTripletFn: a batch of N={N} rows does not fit a memory of {memory.capacity} slots')
        if D != memory.dim:
            raise _lib.ReidHipError(f'XbmTripletFn: the memory holds rows of D={memory.dim}, the batch has D={D}')
        q2, g, qv, res = _two_sided_prepare(q, g, q_valid)
        labels = labels.contiguous()
        mem = (memory.rows, memory.labels, memory.valid)
        if enqueue:
            ops.xbm_enqueue(q2, g, labels, qv, g_valid, normalize, EPS, *mem, memory.cursor, P=P)
        ws = torch.empty(ops.xbm_ws_floats(P, N, memory.capacity, D), device=dev)
        qd = torch.empty(2, P * N, device=dev); qi = torch.empty(2, P * N, dtype=torch.int32, device=dev)
        gd = torch.empty(2, P * N, device=dev); gi = torch.empty(2, P * N, dtype=torch.int32, device=dev)
        ops.xbm_triplet_fwd(q2, g, labels, qv, g_valid, m, normalize, EPS, *mem, qd, qi, gd, gi, ws, res, P=P)
        ctx.save_for_backward(q2, g, qv, g_valid, qd, qi, gd, gi, ws, res)
        ctx.margin, ctx.normalize, ctx.P = m, bool(normalize), P
        loss, flag, n_active = _two_sided_results(ctx, res)
        if rows_out is not None:                              # copies: the saved arrays belong to the backward
            for side, d, ix in (('q', qd, qi), ('g', gd, gi)):
                rows_out.update({f'{side}_d_ap': d[0].view(P, N).clone(), f'{side}_d_an': d[1].view(P, N).clone(),
                                 f'{side}_idx_p': ix[0].view(P, N).clone(), f'{side}_idx_n': ix[1].view(P, N).clone()})
        return loss, flag, n_active

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):
        q2, g, qv, gv, qd, qi, gd, gi, ws, res = ctx.saved_tensors
        P = ctx.P
        dq = torch.empty_like(q2); dg = torch.empty_like(g)
        ops.xbm_triplet_bwd(q2, g, qv, gv, ctx.margin, ctx.normalize, EPS, qd, qi, gd, gi, ws, res, _gscale(dloss, P), dq, dg, P=P)
        return dq.view(P, q2.shape[0] // P, q2.shape[1]), dg, None, None, None, None, None, None, None, None


def xbm_cross_triplet(q, g, labels, memory, q_valid=None, g_valid=None, margin=0.3, normalize=True, enqueue=True):
    """Cross-modal batch-hard triplet loss with a cross-batch memory, for users with their own loop: ``q`` [P, N, D] (P query
    modalities stacked; [N, D] = one) and the vis features ``g`` [N, D] of the SAME N instances, ``labels`` [N], ``memory`` a
    CrossBatchMemory(capacity >= N, P + 1, D).  With ``enqueue`` the batch is first filed into the memory at its cursor (the oldest
    rows are overwritten), so it is part of what is mined; ``enqueue=False`` mines the memory as it stands and leaves it untouched.
    Per pair, every valid q row mines its hardest positive / negative among the valid slots of memory side 0 (vis) and every valid g
    row among those of side p + 1 (Euclidean distance of the unit rows, difference form, fp32; ties to the lowest slot);
    L_p = 0.5 * (mean over the active q anchors + mean over the active g anchors).  The memory's rows are constants.  ``q_valid``
    [P, N] / ``g_valid`` [N]: optional bool / uint8; ``margin`` None: soft margin; ``normalize`` False: the rows are used and stored
    as they are.  Returns (losses [P], flags [P], rows): rows = {'q_d_ap', 'q_d_an', 'q_idx_p', 'q_idx_n', 'g_d_ap', 'g_d_an',
    'g_idx_p', 'g_idx_n'} [P, N] (indices are slot numbers, -1 = inactive) plus 'n_active' [P, 2]; the losses carry the gradient to
    ``q`` and ``g``."""
    q, q_valid, g_valid = _two_sided_args('xbm_cross_triplet', q, g, labels, labels, q_valid, g_valid)
    if not isinstance(memory, CrossBatchMemory):
        raise TypeError('xbm_cross_triplet: memory must be a CrossBatchMemory')
    rows = {}
    loss, flag, n_active = XbmTripletFn.apply(q, g, labels.long(), q_valid, g_valid, memory, margin, bool(normalize), bool(enqueue), rows)
    rows['n_active'] = n_active
    return loss, flag, rows


class ClassCenters:
    """The table of center_loss (Wen et al., ECCV 2016; csrc/center.hip): one centre per identity, ``centers`` f32 [num_classes, dim],
    zero at the start and moved by the update kernel only -- not by the optimizer.  A plain tensor, not a parameter or buffer: the
    table is not part of a state_dict; ``state()`` / ``load_state()`` carry it through a checkpoint (``center_state_dict``).  It may be
    constructed on the CPU for that; the kernels need the device."""

    def __init__(self, num_classes, dim, device='cuda'):
        if not (num_classes >= 1 and dim % 4 == 0 and 4 <= dim <= 1024 and num_classes * dim < 2 ** 31):
            raise ValueError('ClassCenters: num_classes >= 1, dim a multiple of 4 in 4..1024, num_classes * dim < 2^31')
        self.num_classes, self.dim = int(num_classes), int(dim)
        self.centers = torch.zeros(self.num_classes, self.dim, dtype=torch.float32, device=torch.device(device))

    def reset(self):
        """Zeroes the table in place (a device fill: a captured graph that holds it stays valid)."""
        self.centers.zero_()

    def state(self):
        return {'centers': self.centers.detach().cpu().clone()}

    def load_state(self, state):
        """Copies ``state['centers']`` into the table in place; a table of another shape is refused."""
        c = state['centers']
        if tuple(c.shape) != (self.num_classes, self.dim):
            raise ValueError(f'ClassCenters: the state holds centres {tuple(c.shape)}, this table is [{self.num_classes}, {self.dim}]')
        self.centers.copy_(c.to(torch.float32))


class CenterLossFn(torch.autograd.Function):
    """(loss, n_used) of the center loss of x [S, N, D] (S sides stacked, ``labels`` [N] shared) against the table ``centers``
    (csrc/center.hip; the reference has no such loss): loss = 0.5 * mean over the used rows of |x - c_y|^2, a row used when it is valid
    and its label lies in the table.  With ``update`` the centres the forward used are then moved by Wen's rule with step ``alpha``.
    The centres are constants of the loss: the gradient reaches x only, from the differences the forward left in its workspace (the
    table may have moved before the backward runs).  n_used is a float tensor; nothing is read back to the host.  ``rows_out``: an
    optional trailing dict that receives a COPY of ``d2`` (center_loss); the call the model makes is
    ``apply(x, labels, valid, centers, alpha, update)``."""
    @staticmethod
    def forward(ctx, x, labels, valid, centers, alpha: float, update: bool, rows_out=None):
        (S, N, D), dev = x.shape, x.device
        if D != centers.dim:
            raise _lib.ReidHipError(f'CenterLossFn: the table holds centres of D={centers.dim}, the batch has D={D}')
        x2 = x.reshape(S * N, D).contiguous().float()
        labels = labels.contiguous()
        vv = None if valid is None else valid.reshape(S * N).contiguous()
        ws = torch.empty(ops.center_ws_floats(S, N, D), device=dev)
        d2 = torch.empty(S * N, device=dev); res = torch.empty(2, device=dev)
        ops.center_fwd(x2, labels, vv, centers.centers, ws, d2, res, S=S)
        if update:
            ops.center_update(labels, vv, d2, ws, centers.centers, alpha, S=S)
        ctx.save_for_backward(ws, res)
        ctx.shape = (S, N, D)
        loss, n_used = res[0], res[1]
        ctx.mark_non_differentiable(n_used)
        if rows_out is not None:
            rows_out.update(d2=d2.view(S, N).clone())
        return loss, n_used

    @staticmethod
    def backward(ctx, dloss, _dn):
        ws, res = ctx.saved_tensors
        S, N, D = ctx.shape
        dx = torch.empty(S * N, D, device=ws.device)
        ops.center_bwd(ws, res, dloss.reshape(1).float().contiguous(), dx, S=S)
        return dx.view(S, N, D), None, None, None, None, None, None


def center_loss(x, labels, centers, valid=None, alpha=0.5, update=True):
    """Center loss (Wen et al., ECCV 2016) for users with their own loop: ``x`` [S, N, D] (S sides stacked, e.g. the raw features of
    every modality; [N, D] = one side) of the N instances with ``labels`` [N], ``centers`` a ClassCenters(C, D).  A row is used when it
    is valid (``valid`` [S, N] or [N] for one side: optional bool / uint8) and its label lies in 0..C-1; loss = 0.5 * mean over the used
    rows of |x - c_y|^2 (fp32 differences, the mean in fp64).  With ``update`` the centres of the classes in the batch then move:
    c_j -= alpha * sum over its rows of (c_j - x) / (1 + n_j), rows with a non-finite distance left out; ``update=False`` leaves the
    table as it is.  Returns (loss, LazyCount(n_used), rows) with rows = {'d2' [S, N]} (a copy); the loss carries the gradient to ``x``."""
    from .model import LazyCount
    if not (x.is_cuda and labels.is_cuda and (valid is None or valid.is_cuda)):
        raise _lib.ReidHipError('center_loss needs device tensors (there is no CPU path)')
    if not isinstance(centers, ClassCenters):
        raise TypeError('center_loss: centers must be a ClassCenters')
    if not centers.centers.is_cuda:
        raise _lib.ReidHipError('center_loss needs the table on the device (there is no CPU path)')
    flat = x.dim() == 2
    if flat:
        x = x.unsqueeze(0)
    if x.dim() != 3 or labels.shape != x.shape[1:2]:
        raise ValueError('center_loss: x [S, N, D] or [N, D], labels [N]')
    if valid is not None:
        valid = valid.to(torch.uint8).reshape(x.shape[0], x.shape[1]).contiguous()
    if not math.isfinite(float(alpha)):
        raise ValueError(f'center_loss: alpha must be finite, not {alpha}')
    rows = {}
    loss, n_used = CenterLossFn.apply(x, labels.long(), valid, centers, float(alpha), bool(update), rows)
    if flat:
        rows['d2'] = rows['d2'][0]
    return loss, LazyCount(n_used), rows


MARGIN_KINDS = ('cosine', 'cosface', 'arcface', 'circle')
# (scale, margin) a kind takes when the caller leaves them open (TrainingConfig.id_scale / id_margin = None)
MARGIN_DEFAULTS = {'cosine': (30.0, 0.0), 'cosface': (30.0, 0.35), 'arcface': (30.0, 0.5), 'circle': (64.0, 0.35)}


def margin_args(who, kind, scale, margin):
    """The checked (kind, scale, margin) of a cosine-margin head; None for scale or margin = the kind's default."""
    if kind not in MARGIN_KINDS:
        raise ValueError(f'{who}: kind must be one of {MARGIN_KINDS}, not {kind!r}')
    scale = MARGIN_DEFAULTS[kind][0] if scale is None else float(scale)
    margin = MARGIN_DEFAULTS[kind][1] if margin is None else float(margin)
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError(f'{who}: scale must be > 0 and finite, not {scale}')
    if kind == 'cosine':
        return kind, scale, 0.0                               # the margin is ignored
    limit, text = (math.pi / 2, 'pi/2 for arcface') if kind == 'arcface' else (1.0, f'1 for {kind}')
    if not 0 <= margin < limit:
        raise ValueError(f'{who}: margin must be in [0, {text}), not {margin}')
    return kind, scale, margin


class CosineLinearFn(torch.autograd.Function):
    """logits [B, C] = scale * cos(x_b, W_c) of x [B, D] (not assumed unit) and W [C, D] (csrc/margin_ce.hip; the reference has no
    such head): rows divided by max(|row|, EPS) as F.normalize does.  The margin-free logits of the cosine-margin heads."""

    @staticmethod
    def forward(ctx, x, W, scale: float):
        x = x.contiguous().float(); W = W.detach().contiguous().float()
        (B, D), C, dev = x.shape, W.shape[0], x.device
        rx = torch.empty(B, device=dev, dtype=torch.float64); rw = torch.empty(C, device=dev, dtype=torch.float64)
        logits = torch.empty(B, C, device=dev)
        ops.cos_logits_fwd(x, W, float(scale), EPS, rx, rw, logits)
        ctx.save_for_backward(x, W, rx, rw)
        ctx.scale = float(scale)
        return logits

    @staticmethod
    def backward(ctx, g):
        x, W, rx, rw = ctx.saved_tensors
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_w):                            # only what autograd asks for, as LinearF32Fn
            return None, None, None
        g = g.contiguous().float()
        dev = x.device
        G = torch.empty(x.shape, device=dev, dtype=torch.float64) if want_x else None          # fp64 products, rounded once in the fix
        H = torch.empty(W.shape, device=dev, dtype=torch.float64) if want_w else None
        ops.cos_logits_bwd_prep(g, x, W, rx, rw, G, H)
        dx = torch.empty_like(x) if want_x else None
        dW = torch.empty_like(W) if want_w else None
        ops.cos_logits_bwd_fix(x, rx, G, dx, W, rw, H, dW, ctx.scale, EPS)
        return dx, dW, None


class MarginCEFn(torch.autograd.Function):
    """(loss, count) of the label-smoothed CE of the margin logits of ``kind`` (cosine | cosface | arcface | circle; include/reid_hip.h
    has the definitions) of logits = scale * cos (CosineLinearFn's): the mean over the rows with valid != 0 and a label in [0, C).
    count is a float tensor; nothing is read back to the host."""

    @staticmethod
    def forward(ctx, logits, labels, valid, smoothing: float, kind: str, scale: float, margin: float):
        kind, scale, margin = margin_args('MarginCEFn', kind, scale, margin)
        logits = logits.contiguous().float()
        labels = labels.contiguous()
        row_loss = torch.empty(logits.shape[0], device=logits.device)
        res = torch.empty(3, device=logits.device)
        ops.margin_ce_fwd(logits, labels, valid, kind, scale, margin, float(smoothing), row_loss, res)
        ctx.save_for_backward(logits, labels, valid, res)
        ctx.args = (kind, scale, margin, float(smoothing))
        loss, cnt = res[2], res[1]
        ctx.mark_non_differentiable(cnt)
        return loss, cnt

    @staticmethod
    def backward(ctx, dloss, _dcnt):
        logits, labels, valid, res = ctx.saved_tensors
        dl = torch.empty_like(logits)
        ops.margin_ce_bwd(logits, labels, valid, *ctx.args, res, dloss.reshape(1).float().contiguous(), dl)
        return dl, None, None, None, None, None, None


def margin_cross_entropy(features, weight, labels, valid=None, kind='cosface', scale=30.0, margin=0.35, smoothing=0.1):
    """Cosine-margin identity loss for users with their own loop: ``features`` [B, D] (not assumed unit) against the class weights
    ``weight`` [C, D], both L2-normalised inside; logits = scale * cos; ``kind`` 'cosine' (NormFace, margin ignored), 'cosface'
    (cos_y - m), 'arcface' (cos(theta_y + m) with the hard fallback below cos(pi - m)) or 'circle' (Sun et al. 2020, self-paced
    weights that carry no gradient); label-smoothed CE of the margin logits, mean over the rows that take part.  ``valid``: optional
    bool / uint8 [B]; rows with a label outside [0, C) take no part either.  Returns (loss, LazyCount(count), logits): the loss
    carries the gradient to ``features`` and ``weight``, logits are the margin-free scale * cos."""
    from .model import LazyCount
    kind, scale, margin = margin_args('margin_cross_entropy', kind, scale, margin)
    if not 0 <= smoothing <= 1:
        raise ValueError(f'margin_cross_entropy: smoothing must be in [0, 1], not {smoothing}')
    if not (features.is_cuda and weight.is_cuda and labels.is_cuda and (valid is None or valid.is_cuda)):
        raise _lib.ReidHipError('margin_cross_entropy needs device tensors (there is no CPU path)')
    if features.dim() != 2 or weight.dim() != 2 or weight.shape[1] != features.shape[1] or labels.shape != features.shape[:1] \
            or (valid is not None and valid.shape != labels.shape):
        raise ValueError('margin_cross_entropy: features [B, D], weight [C, D], labels [B], valid [B]')
    if valid is not None:
        valid = valid.to(torch.uint8).contiguous()
    logits = CosineLinearFn.apply(features, weight, scale)
    loss, cnt = MarginCEFn.apply(logits, labels.long(), valid, float(smoothing), kind, scale, margin)
    return loss, LazyCount(cnt), logits


# ----------------------------------------------------------------------------------------------------------------
# Small fp32 pieces of SemanticDisentanglementModule (models/model.py:57-77) and FeatureFusion (:113-183)
class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.eltwise('add', a.contiguous().float(), b.contiguous().float())

    @staticmethod
    def backward(ctx, g):
        return g, g


class MulFn(torch.autograd.Function):
    """y = x * m with a constant multiplier tensor m (dropout masks 0 or 1/keep): nn.Dropout / DropPath-style scaling."""

    @staticmethod
    def forward(ctx, x, m):
        m = m.contiguous().float()
        ctx.save_for_backward(m)
        return ops.eltwise('mul', x.contiguous().float(), m)

    @staticmethod
    def backward(ctx, g):
        (m,) = ctx.saved_tensors
        return ops.eltwise('mul', g.contiguous().float(), m), None


class ActFn(torch.autograd.Function):
    """relu / gelu (exact erf form) with the matching derivative kernels."""

    @staticmethod
    def forward(ctx, x, kind: str):
        x = x.contiguous().float()
        ctx.save_for_backward(x)
        ctx.kind = kind
        return ops.eltwise(kind, x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.eltwise(ctx.kind + '_bwd', x, g.contiguous().float()), None


class NanToNumFn(torch.autograd.Function):
    """torch.nan_to_num(x, nan=0, posinf=1e4, neginf=-1e4) (model.py:165); the gradient passes where x is finite."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous().float()
        ctx.save_for_backward(x)
        return ops.eltwise('nan_to_num', x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.isfinite(x)


class LayerNormF32Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps: float):
        shp = x.shape
        x2 = x.contiguous().float().view(-1, shp[-1])
        y = torch.empty_like(x2)
        mean = torch.empty(x2.shape[0], device=x2.device); rstd = torch.empty_like(mean)
        ops.layernorm_fwd(x2, w.detach(), b.detach(), y_f32=y, mean=mean, rstd=rstd, eps=eps)
        ctx.save_for_backward(x2, w.detach(), mean, rstd)
        ctx.shp = shp
        return y.view(shp)

    @staticmethod
    def backward(ctx, g):
        x2, w, mean, rstd = ctx.saved_tensors
        g2 = g.contiguous().float().view(x2.shape)
        dx = torch.empty_like(x2)
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw = torch.zeros_like(w) if want else None; db = torch.zeros_like(w) if want else None
        ops.layernorm_bwd(g2, x2, w, mean, rstd, dx, dgamma=dw, dbeta=db)
        return dx.view(ctx.shp), dw, db, None


class LinearNdF32Fn(torch.autograd.Function):
    """y = x @ W.T + b for x of any leading shape, exact fp32 (vector-ALU GEMM)."""

    @staticmethod
    def forward(ctx, x, W, b):
        shp = x.shape
        x2 = x.contiguous().float().view(-1, shp[-1])
        W = W.detach().contiguous()
        y = torch.empty(x2.shape[0], W.shape[0], device=x2.device)
        ops.sgemm(x2, W, y, tb=True, bias=None if b is None else b.detach().contiguous())
        ctx.save_for_backward(x2, W)
        ctx.shp = shp; ctx.has_bias = b is not None
        return y.view(shp[:-1] + (W.shape[0],))

    @staticmethod
    def backward(ctx, g):
        x2, W = ctx.saved_tensors
        g2 = g.contiguous().float().view(x2.shape[0], W.shape[0])
        dx = dW = None                                        # only what autograd asks for: the SDM module and the fusion block
        if ctx.needs_input_grad[0]:                           # are frozen under the reference's default rule (train.py:1418-1425)
            dx = torch.empty_like(x2)
            ops.sgemm(g2, W, dx)
        if ctx.needs_input_grad[1]:
            dW = torch.empty_like(W)
            ops.sgemm(g2, x2, dW, ta=True)
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            ones = torch.ones(1, g2.shape[0], device=g2.device)
            db = torch.empty(1, W.shape[0], device=g2.device)
            ops.sgemm(ones, g2, db)
            db = db.view(-1)
        return (None if dx is None else dx.view(ctx.shp)), dW, db


class SmallAttnFn(torch.autograd.Function):
    """softmax(q k^T / 8 + key padding) v over S <= 8 tokens (nn.MultiheadAttention core, head_dim 64), fp32."""

    @staticmethod
    def forward(ctx, qkv, key_mask, n_seq: int, S: int, heads: int, drop=None):
        """``drop``: optional f32 [n_seq, heads, 8, 8] attention-dropout multipliers (0 or 1/keep)."""
        qkv = qkv.contiguous().float()
        d = heads * 64
        out = torch.empty(n_seq * S, d, device=qkv.device)
        probs = torch.zeros(n_seq * heads * 64, device=qkv.device)
        drop = None if drop is None else drop.contiguous().float()
        ops.small_attn_fwd(qkv, key_mask, out, probs, n_seq, S, heads, drop=drop)
        ctx.save_for_backward(qkv, probs, drop)
        ctx.dims = (n_seq, S, heads)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, probs, drop = ctx.saved_tensors
        n_seq, S, heads = ctx.dims
        dqkv = torch.empty_like(qkv)
        ops.small_attn_bwd(qkv, probs, g.contiguous().float(), dqkv, n_seq, S, heads, drop=drop)
        return dqkv, None, None, None, None, None


class MaskedMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        B, M, D = x.shape
        x = x.contiguous().float(); mask = mask.contiguous().float()
        out = torch.empty(B, D, device=x.device)
        ops.masked_mean(x, mask, out, B, M, D)
        ctx.save_for_backward(mask)
        ctx.dims = (B, M, D)
        return out

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        B, M, D = ctx.dims
        dx = torch.empty(B, M, D, device=g.device)
        ops.masked_mean(g.contiguous().float(), mask, dx, B, M, D, backward=True)
        return dx, None
