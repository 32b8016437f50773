"""Autograd boundaries and public functions of the loss kernels: label-smoothed CE, SDM loss, batch-hard triplet loss, cross-modal
batch-hard triplet loss, hetero-center triplet loss, cross-batch memory (XBM), cross-modal Smooth-AP (in the batch or over a ring), center
loss, cluster-contrast memory loss, hybrid (instance + cluster) memory loss, margin CE of the cosine-margin heads.

Reference: compute_loss models/model.py:512-659; sdm_loss_stable models/sdm_loss.py:13-149 (the reference has CE and SDM only).  All
arithmetic is in libreid_hip.so (fp32); torch only carries the tensors.  The two-sided losses (one stack of query modalities against
vis) share one forward prologue / epilogue and one backward; a class states its saved arrays, its two ``ops`` calls and its rows.
"""
import math

import torch

from . import _lib, ops


class LazyCount:
    """Integer that lives on the device until someone looks at it (keeps compute_loss free of host syncs)."""

    def __init__(self, t):
        self._t = t

    def __int__(self):
        return int(self._t.item())

    __index__ = __int__

    def __eq__(self, o):
        return int(self) == o

    def __gt__(self, o):
        return int(self) > o

    def __repr__(self):
        return str(int(self))


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


def _need_device(who, *tensors):
    if not all(t.is_cuda for t in tensors if t is not None):
        raise _lib.ReidHipError(f'{who} needs device tensors (there is no CPU path)')


def _margin_arg(fn, margin):
    """The kernels' margin: None (the soft-margin form) -> -1.0."""
    if margin is not None and float(margin) < 0:
        raise ValueError(f'{fn.__name__}: margin must be >= 0, or None for the soft-margin form')
    return -1.0 if margin is None else float(margin)


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
    _need_device('batch_hard_triplet', features, labels, valid)
    if features.dim() != 2 or labels.shape != features.shape[:1]:
        raise ValueError('batch_hard_triplet: features [B, D], labels [B]')
    if valid is not None:
        valid = valid.to(torch.uint8).contiguous()
    rows = {}
    loss, n_active = TripletHardFn.apply(features, labels.long(), valid, margin, rows)
    return loss, LazyCount(n_active), rows


# ----------------------------------------------------------------------------------------------------------------
# The two-sided losses: P stacked query modalities q [P, N, D] against the vis features g; result [P, 4] = (L_p, flag_p, two counts)
def _two_sided_prepare(fn, q, g, q_valid, margin):
    """The kernels' margin and q [P, N, D], g [Mg, D], q_valid [P, N] or None as the two-sided kernels take them:
    (m, q2 [P*N, D], g, qv [P*N], res [P, 4])."""
    m = _margin_arg(fn, margin)
    P, N, D = q.shape
    q2 = q.reshape(P * N, D).contiguous().float()
    return m, q2, g.contiguous().float(), None if q_valid is None else q_valid.reshape(P * N).contiguous(), torch.empty(P, 4, device=q.device)


def _two_sided_finish(ctx, saved, m, normalize, res):
    """Keeps ``saved`` (q2, g, then the loss's own tensors, res last) for _two_sided_backward; returns (loss, flag, n_active) of
    res [P, 4], of which only the loss is differentiable."""
    ctx.save_for_backward(*saved)
    ctx.margin, ctx.normalize, ctx.P = m, bool(normalize), res.shape[0]
    loss, flag, n_active = res[:, 0].contiguous(), res[:, 1].contiguous(), res[:, 2:].contiguous()
    ctx.mark_non_differentiable(flag, n_active)
    return loss, flag, n_active


def _gscale(dloss, P):                                        # (a copy: the cotangent of L.sum() is an expanded scalar with stride 0)
    return torch.empty(P, device=dloss.device).copy_(dloss.reshape(P))


def _two_sided_backward(ctx, dloss, n_inputs, bwd):
    """The backward of every two-sided loss.  ``bwd(saved, consts, outs)`` is the loss's one ``ops`` call, from the saved tensors, consts
    = (margin, normalize, EPS) and outs = (gscale [P], dq, dg); ``n_inputs``: the arguments of the forward, of which q and g get one."""
    saved, P = ctx.saved_tensors, ctx.P
    q2, g = saved[:2]
    dq = torch.empty_like(q2); dg = torch.empty_like(g)
    bwd(saved, (ctx.margin, ctx.normalize, EPS), (_gscale(dloss, P), dq, dg))
    return (dq.view(P, q2.shape[0] // P, q2.shape[1]), dg) + (None,) * (n_inputs - 2)


def _mined(n, dev):
    """A side's (d_ap | d_an) f32 [2, n] and (idx_p | idx_n) i32 [2, n]."""
    return torch.empty(2, n, device=dev), torch.empty(2, n, dtype=torch.int32, device=dev)


def _mined_rows(side, d, ix, shape):
    """rows_out's entries of a side's _mined arrays.  Copies: the saved arrays belong to the backward."""
    return {f'{side}_d_ap': d[0].view(shape).clone(), f'{side}_d_an': d[1].view(shape).clone(),
            f'{side}_idx_p': ix[0].view(shape).clone(), f'{side}_idx_n': ix[1].view(shape).clone()}


def _two_sided_loss(who, fn, q, g, labels, q_valid, g_valid, *extra):
    """The body of the three public two-sided functions: the argument checks, q as [P, N, D] and the validity vectors as the kernels
    take them, then ``fn.apply``.  ``labels`` = (q_labels, g_labels), or (labels,) where both sides share them."""
    _need_device(who, q, g, *labels, q_valid, g_valid)
    if q.dim() == 2:
        q = q.unsqueeze(0)
    if q.dim() != 3 or g.dim() != 2 or g.shape[1] != q.shape[2] or labels[0].shape != q.shape[1:2] or labels[-1].shape != g.shape[:1]:
        raise ValueError(f'{who}: q [P, N, D] or [N, D], g [Mg, D], q_labels [N], g_labels [Mg]')
    if fn is XbmTripletFn and not isinstance(extra[0], CrossBatchMemory):
        raise TypeError(f'{who}: memory must be a CrossBatchMemory')
    if q_valid is not None:
        q_valid = q_valid.to(torch.uint8).reshape(q.shape[0], q.shape[1]).contiguous()
    if g_valid is not None:
        g_valid = g_valid.to(torch.uint8).contiguous()
    rows = {}
    loss, flag, n_active = fn.apply(q, g, *[t.long() for t in labels], q_valid, g_valid, *extra, rows)
    rows['n_active'] = n_active
    return loss, flag, rows


class CrossTripletFn(torch.autograd.Function):
    """(loss [P], flag [P], n_active [P, 2]) of the cross-modal batch-hard triplet loss between P stacked modality feature sets
    q [P, N, D] and the vis features g [Mg, D] (csrc/cross_triplet.hip; the reference has no such loss): unit rows, difference-form
    distances, hardest positive / negative in both directions, L_p the mean of the two directions' means.  ``margin`` None: the
    soft-margin form.  n_active = (q->g, g->q) active anchors as floats; nothing is read back to the host.  ``rows_out``: an optional
    trailing dict that receives COPIES of the saved arrays (cross_modal_triplet); the call the model makes is
    ``apply(q, g, q_label, g_label, q_valid, g_valid, margin, normalize)``."""
    @staticmethod
    def forward(ctx, q, g, q_label, g_label, q_valid, g_valid, margin, normalize: bool, rows_out=None):
        (P, N, D), Mg, dev = q.shape, g.shape[0], q.device
        m, q2, g, qv, res = _two_sided_prepare(CrossTripletFn, q, g, q_valid, margin)
        ws = torch.empty(ops.cross_triplet_ws_floats(P, N, Mg, D), device=dev)
        (qd, qi), (gd, gi) = _mined(P * N, dev), _mined(P * Mg, dev)
        ops.cross_triplet_fwd(q2, g, q_label.contiguous(), g_label.contiguous(), qv, g_valid, m, normalize, EPS, qd, qi, gd, gi, ws, res, P=P)
        if rows_out is not None:
            rows_out.update(**_mined_rows('q', qd, qi, (P, N)), **_mined_rows('g', gd, gi, (P, Mg)))
        return _two_sided_finish(ctx, (q2, g, qv, g_valid, qd, qi, gd, gi, ws, res), m, normalize, res)

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):            # saved: q2, g, qv, gv | qd, qi, gd, gi, ws, res
        return _two_sided_backward(ctx, dloss, 9, lambda s, consts, outs: ops.cross_triplet_bwd(*s[:4], *consts, *s[4:], *outs, P=ctx.P))


def cross_modal_triplet(q, g, q_labels, g_labels, q_valid=None, g_valid=None, margin=0.3, normalize=True):
    """Cross-modal batch-hard triplet loss for users with their own loop: ``q`` [P, N, D] (P query modalities stacked; [N, D] = one)
    against the vis features ``g`` [Mg, D].  Per pair, every valid q row mines its hardest positive / negative among the g rows and
    every valid g row among the pair's q rows (Euclidean distance of the unit rows, difference form, fp32; no self-exclusion);
    L_p = 0.5 * (mean over the active q anchors + mean over the active g anchors).  ``q_valid`` [P, N] / ``g_valid`` [Mg]: optional
    bool / uint8, rows that take part; ``margin`` None: soft margin; ``normalize`` False: the rows are used as they are.  Returns
    (losses [P], flags [P], rows): flag 1 where the pair has an active anchor, rows = {'q_d_ap', 'q_d_an', 'q_idx_p', 'q_idx_n'} [P, N]
    and {'g_d_ap', 'g_d_an', 'g_idx_p', 'g_idx_n'} [P, Mg] (g indices into 0..N-1) plus 'n_active' [P, 2]; the losses carry the
    gradient to ``q`` and ``g``."""
    return _two_sided_loss('cross_modal_triplet', CrossTripletFn, q, g, (q_labels, g_labels), q_valid, g_valid, margin, bool(normalize))


class HcTripletFn(torch.autograd.Function):
    """(loss [P], flag [P], n_active [P, 2]) of the hetero-center triplet loss between P stacked modality feature sets q [P, N, D] and
    the vis features g [Mg, D] (csrc/hc_triplet.hip; the reference has no such loss): unit rows, per-identity centres of every side,
    the triplet on the centres of [pair p's q centres | g centres].  ``margin`` None: the soft-margin form.  n_active = active anchors
    among the (q, g) centres as floats; nothing is read back to the host.  ``rows_out``: an optional trailing dict that receives COPIES
    of the saved arrays (hetero_center_triplet); the call the model makes is
    ``apply(q, g, q_label, g_label, q_valid, g_valid, margin, normalize)``."""
    @staticmethod
    def forward(ctx, q, g, q_label, g_label, q_valid, g_valid, margin, normalize: bool, rows_out=None):
        (P, N, D), Mg, dev = q.shape, g.shape[0], q.device
        m, q2, g, qv, res = _two_sided_prepare(HcTripletFn, q, g, q_valid, margin)
        R, U = P * N + Mg, N + Mg
        ws = torch.empty(ops.hc_triplet_ws_floats(P, N, Mg, D), device=dev)
        ints = torch.empty(2, R, dtype=torch.int32, device=dev)                                  # lead | count
        clabel = torch.empty(R, dtype=torch.int64, device=dev)
        d = torch.empty(2, P, U, device=dev); idx = torch.empty(2, P, U, dtype=torch.int32, device=dev)
        ops.hc_triplet_fwd(q2, g, q_label.contiguous(), g_label.contiguous(), qv, g_valid, m, normalize, EPS,
                           ints[0], ints[1], clabel, d, idx, ws, res, P=P)
        if rows_out is not None:                              # copies: the saved arrays belong to the backward
            for side, rows, slots in (('q', slice(0, P * N), slice(0, N)), ('g', slice(P * N, R), slice(N, U))):
                shape = (P, N) if side == 'q' else (Mg,)
                rows_out.update({f'{side}_lead': ints[0, rows].reshape(shape).clone(), f'{side}_count': ints[1, rows].reshape(shape).clone(),
                                 f'{side}_label': clabel[rows].reshape(shape).clone(),
                                 f'{side}_d_ap': d[0, :, slots].clone(), f'{side}_d_an': d[1, :, slots].clone(),
                                 f'{side}_idx_p': idx[0, :, slots].clone(), f'{side}_idx_n': idx[1, :, slots].clone()})
        return _two_sided_finish(ctx, (q2, g, ints, ws, res), m, normalize, res)

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):            # saved: q2, g | ints = (lead | count), ws, res
        return _two_sided_backward(ctx, dloss, 9, lambda s, consts, outs: ops.hc_triplet_bwd(*s[:2], *consts, s[2][0], s[2][1], *s[3:], *outs, P=ctx.P))


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
    return _two_sided_loss('hetero_center_triplet', HcTripletFn, q, g, (q_labels, g_labels), q_valid, g_valid, margin, bool(normalize))


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
        return LazyCount(self.cursor[1])

    @property
    def filled(self):
        """Slots that hold a row (valid or not), read from the device when someone looks at it."""
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
        (P, N, D), dev = q.shape, q.device
        m, q2, g, qv, res = _two_sided_prepare(XbmTripletFn, q, g, q_valid, margin)
        if g.shape[0] != N or P + 1 != memory.sides:
            raise ValueError(f'XbmTripletFn: q [P, N, D] and g [N, D] with P + 1 = {memory.sides} sides of the memory')
        if N > memory.capacity:
            raise ValueError(f'XbmTripletFn: a batch of N={N} rows does not fit a memory of {memory.capacity} slots')
        if D != memory.dim:
            raise _lib.ReidHipError(f'XbmTripletFn: the memory holds rows of D={memory.dim}, the batch has D={D}')
        labels = labels.contiguous()
        mem = (memory.rows, memory.labels, memory.valid)
        if enqueue:
            ops.xbm_enqueue(q2, g, labels, qv, g_valid, normalize, EPS, *mem, memory.cursor, P=P)
        ws = torch.empty(ops.xbm_ws_floats(P, N, memory.capacity, D), device=dev)
        (qd, qi), (gd, gi) = _mined(P * N, dev), _mined(P * N, dev)
        ops.xbm_triplet_fwd(q2, g, labels, qv, g_valid, m, normalize, EPS, *mem, qd, qi, gd, gi, ws, res, P=P)
        if rows_out is not None:
            rows_out.update(**_mined_rows('q', qd, qi, (P, N)), **_mined_rows('g', gd, gi, (P, N)))
        return _two_sided_finish(ctx, (q2, g, qv, g_valid, qd, qi, gd, gi, ws, res), m, normalize, res)

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):            # saved: q2, g, qv, gv | qd, qi, gd, gi, ws, res
        return _two_sided_backward(ctx, dloss, 10, lambda s, consts, outs: ops.xbm_triplet_bwd(*s[:4], *consts, *s[4:], *outs, P=ctx.P))


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
    return _two_sided_loss('xbm_cross_triplet', XbmTripletFn, q, g, (labels,), q_valid, g_valid, memory, margin, bool(normalize), bool(enqueue))


def smooth_ap_temperature(who, temperature):
    """The checked temperature of the Smooth-AP loss."""
    temperature = float(temperature)
    if not (temperature > 0 and math.isfinite(temperature)):
        raise ValueError(f'{who}: temperature must be > 0 and finite, not {temperature}')
    return temperature


def _check_ring(who, memory, P, N, Mg, D, enqueue):
    """A CrossBatchMemory against the batch q [P, N, D], g [Mg, D] of the ring forms."""
    if Mg != N or P + 1 != memory.sides:
        raise ValueError(f'{who}: q [P, N, D] and g [N, D] with P + 1 = {memory.sides} sides of the memory')
    if enqueue and N > memory.capacity:
        raise ValueError(f'{who}: a batch of N={N} rows does not fit a memory of {memory.capacity} slots')
    if D != memory.dim:
        raise _lib.ReidHipError(f'{who}: the memory holds rows of D={memory.dim}, the batch has D={D}')


class SmoothAPFn(torch.autograd.Function):
    """(loss [P], flag [P], n_active [P, 2]) of the cross-modal Smooth-AP ranking loss between P stacked modality feature sets
    q [P, N, D] and the vis features g [Mg, D] (csrc/smooth_ap.hip; the reference has no such loss): every valid
    q row of pair p ranks a gallery by cosine and so does every valid g row; L_p = 0.5 * (mean of 1 - AP over the active q anchors +
    the same over the active g anchors), AP in Brown et al.'s sigmoid form at temperature ``tau``.  ``memory`` None: the galleries are
    g and pair p's q rows and receive a gradient.  ``memory`` a CrossBatchMemory: with ``enqueue`` the batch is first filed into it
    (reid_xbm_enqueue, unchanged), then the q rows rank the valid slots of side 0 and the g rows those of side p + 1; the slots are
    constants, and the forward leaves the finished gradients in its workspace, so later enqueues cannot change a pending backward.
    ``with_grad`` False (or no input that requires a gradient): the gradient part of the forward is skipped.  n_active = (q->g, g->q)
    active anchors as floats; nothing is read back to the host.  ``rows_out``: an optional trailing dict that receives COPIES of
    ``q_ap``, ``g_ap`` (-1 = inactive), ``q_npos``, ``g_npos``; the call the model makes is
    ``apply(q, g, q_label, g_label, q_valid, g_valid, memory, tau, normalize, enqueue, with_grad)``."""
    @staticmethod
    def forward(ctx, q, g, q_label, g_label, q_valid, g_valid, memory, tau: float, normalize: bool, enqueue: bool, with_grad: bool, rows_out=None):
        (P, N, D), Mg, dev = q.shape, g.shape[0], q.device
        _, q2, g, qv, res = _two_sided_prepare(SmoothAPFn, q, g, q_valid, 0.0)
        with_grad = bool(with_grad and any(ctx.needs_input_grad[:2]))
        q_label, g_label = q_label.contiguous(), g_label.contiguous()
        ring = None
        if memory is not None:
            _check_ring('SmoothAPFn', memory, P, N, Mg, D, enqueue)
            ring = (memory.rows, memory.labels, memory.valid)
            if enqueue:
                ops.xbm_enqueue(q2, g, g_label, qv, g_valid, normalize, EPS, *ring, memory.cursor, P=P)
        G = (Mg, N) if memory is None else (memory.capacity, memory.capacity)
        ws = torch.empty(ops.smooth_ap_ws_floats(P, N, Mg, D, *G, with_grad), device=dev)
        ap = torch.empty(P * (N + Mg), device=dev); npos = torch.empty(P * (N + Mg), dtype=torch.int32, device=dev)      # q anchors | g anchors
        ops.smooth_ap_fwd(q2, g, q_label, g_label, qv, g_valid, tau, normalize, EPS, with_grad, ap[:P * N], npos[:P * N], ap[P * N:],
                          npos[P * N:], ws, res, P=P, ring=ring)
        if rows_out is not None:
            rows_out.update(q_ap=ap[:P * N].view(P, N).clone(), g_ap=ap[P * N:].view(P, Mg).clone(),
                            q_npos=npos[:P * N].view(P, N).clone(), g_npos=npos[P * N:].view(P, Mg).clone())
        ctx.with_grad = with_grad
        return _two_sided_finish(ctx, (q2, g, qv, g_valid, ws, res), 0.0, normalize, res)

    @staticmethod
    def backward(ctx, dloss, _dflag, _dn):            # saved: q2, g (their shapes only), qv, gv | ws, res
        if not ctx.with_grad:
            raise _lib.ReidHipError('SmoothAPFn: this forward ran without its gradient part (with_grad=False)')
        return _two_sided_backward(ctx, dloss, 12, lambda s, consts, outs: ops.smooth_ap_bwd(s[2], s[3], s[4], *outs, P=ctx.P))


def _smooth_ap_with_grad(q, g):
    return bool(torch.is_grad_enabled() and (q.requires_grad or g.requires_grad))


def smooth_ap(q, g, q_labels, g_labels, q_valid=None, g_valid=None, temperature=0.01, normalize=True):
    """Cross-modal Smooth-AP ranking loss (Brown et al., ECCV 2020) for users with their own loop: ``q`` [P, N, D] (P query modalities
    stacked; [N, D] = one) against the vis features ``g`` [Mg, D].  Per pair, every valid q row ranks the valid g rows by cosine and
    every valid g row the pair's valid q rows (no self-exclusion); with sigma_ij = sigmoid((s_j - s_i) / temperature), R_i = 1 +
    sum_{j != i} sigma_ij over the gallery and R+_i the same over the anchor's positives, AP = mean over the positives of R+_i / R_i;
    an anchor is active when it has a positive and a negative; L_p = 0.5 * (mean of 1 - AP over the active q anchors + the same over
    the active g anchors).  As temperature -> 0 this is 1 - the AP evaluate.rank_and_metrics reports.  Cosines are formed in fp64 and
    rounded once, the rest is fp32 in a fixed order: two runs give the same bits.  ``q_valid`` [P, N] / ``g_valid`` [Mg]: optional
    bool / uint8, rows that take part; ``normalize`` False: the rows are used as they are.  At most 8192 rows per side.  Returns
    (losses [P], flags [P], rows): flag 1 where the pair has an active anchor, rows = {'q_ap', 'q_npos'} [P, N], {'g_ap', 'g_npos'}
    [P, Mg] (copies; AP -1 = inactive) plus 'n_active' [P, 2]; the losses carry the gradient to ``q`` and ``g``.  Without gradients
    (no_grad, or neither input requires one) the gradient part of the forward is skipped."""
    tau = smooth_ap_temperature('smooth_ap', temperature)
    _need_device('smooth_ap', q, g)
    return _two_sided_loss('smooth_ap', SmoothAPFn, q, g, (q_labels, g_labels), q_valid, g_valid, None, tau, bool(normalize), False,
                           _smooth_ap_with_grad(q, g))


def smooth_ap_xbm(q, g, labels, memory, q_valid=None, g_valid=None, temperature=0.01, normalize=True, enqueue=True):
    """Smooth-AP over a ring, for users with their own loop: ``q`` [P, N, D] and the vis features ``g`` [N, D] of the SAME N instances,
    ``labels`` [N], ``memory`` a CrossBatchMemory(capacity, P + 1, D) of this loss alone.  With ``enqueue`` the batch is first filed
    into the memory at its cursor (capacity >= N), so it is part of what is ranked; ``enqueue=False`` ranks the memory as it stands and
    leaves it untouched.  Per pair, every valid q row ranks the valid slots of memory side 0 (vis) and every valid g row those of side
    p + 1, by the rules of ``smooth_ap``; a list of thousands of rows is what the soft rank wants.  The memory's rows are constants:
    the gradient reaches ``q`` and ``g`` only, and it is finished inside the forward, so later enqueues cannot change a pending
    backward.  Returns (losses [P], flags [P], rows) as ``smooth_ap`` with every array [P, N]."""
    tau = smooth_ap_temperature('smooth_ap_xbm', temperature)
    _need_device('smooth_ap_xbm', q, g)
    if not isinstance(memory, CrossBatchMemory):
        raise TypeError('smooth_ap_xbm: memory must be a CrossBatchMemory')
    return _two_sided_loss('smooth_ap_xbm', SmoothAPFn, q, g, (labels, labels), q_valid, g_valid, memory, tau, bool(normalize), bool(enqueue),
                           _smooth_ap_with_grad(q, g))


# ----------------------------------------------------------------------------------------------------------------
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
    _need_device('center_loss', x, labels, valid)
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


# ----------------------------------------------------------------------------------------------------------------
CLUSTER_NCE_MODES = ('mean', 'hard')


def cluster_nce_args(who, temperature, momentum, mode):
    """The checked (temperature, momentum, mode) of the cluster-contrast loss."""
    if mode not in CLUSTER_NCE_MODES:
        raise ValueError(f"{who}: mode must be 'mean' or 'hard', not {mode!r}")
    temperature, momentum = float(temperature), float(momentum)
    if not (temperature > 0 and math.isfinite(temperature)):
        raise ValueError(f'{who}: temperature must be > 0 and finite, not {temperature}')
    if not 0 <= momentum <= 1:
        raise ValueError(f'{who}: momentum must be in [0, 1], not {momentum}')
    return temperature, momentum, mode


class ClusterMemory:
    """The memory of cluster_nce (SpCL's cluster-level memory, Ge et al. 2020; Cluster-Contrast, Dai et al. 2021; csrc/cluster_nce.hip):
    one unit centroid per cluster of a pseudo-labelled set, ``centroids`` f32 [num_clusters, dim], moved by the momentum update only --
    not by the optimizer.  A plain tensor, not a parameter or buffer: ``state()`` / ``load_state()`` carry it through a checkpoint
    (``cluster_memory_state_dict``).  Cluster numbers change at every re-clustering: build a new memory from the features with
    ``from_labels`` / ``from_clustering``.  It may be constructed on the CPU to carry a state; the kernels need the device."""

    def __init__(self, num_clusters, dim, device='cuda'):
        if not (num_clusters >= 1 and dim % 32 == 0 and 32 <= dim <= 1024 and num_clusters * dim < 2 ** 31):
            raise ValueError('ClusterMemory: num_clusters >= 1, dim a multiple of 32 in 32..1024, num_clusters * dim < 2^31')
        self.num_clusters, self.dim = int(num_clusters), int(dim)
        self.centroids = torch.zeros(self.num_clusters, self.dim, dtype=torch.float32, device=torch.device(device))

    @classmethod
    def from_labels(cls, feats, labels):
        """The memory of the pseudo-labelled rows ``feats`` [n, D] (device, fp32): K = max label + 1, centroid k = the normalised fp32
        mean of the rows with label k, summed in ascending row index (grouped by a stable sort here, one wave per cluster on the
        device).  Labels of -1 (DBSCAN noise) are skipped; a cluster number without a row raises."""
        _need_device('ClusterMemory.from_labels', feats, labels)
        if feats.dim() != 2 or labels.shape != feats.shape[:1]:
            raise ValueError('ClusterMemory.from_labels: feats [n, D], labels [n]')
        labels = labels.long()
        if labels.numel() == 0 or int(labels.max()) < 0:
            raise ValueError('ClusterMemory.from_labels: no row has a cluster')
        if int(labels.min()) < -1:
            raise ValueError('ClusterMemory.from_labels: labels are cluster numbers >= 0, or -1 for a row without one')
        K = int(labels.max()) + 1
        counts = torch.bincount(labels[labels >= 0], minlength=K)
        if bool((counts == 0).any()):
            raise ValueError(f'ClusterMemory.from_labels: cluster {int((counts == 0).nonzero()[0])} has no row (cluster numbers must be 0..K-1 without gaps)')
        mem = cls(K, feats.shape[1], feats.device)
        order = torch.sort(labels, stable=True).indices[int((labels < 0).sum()):].contiguous()
        offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).contiguous()
        feats = feats.float()
        if feats.stride(1) != 1 or feats.stride(0) % 4 or feats.data_ptr() % 16:
            feats = feats.contiguous()
        ops.cluster_centroids(feats, order, offsets, mem.centroids)
        return mem

    @classmethod
    def from_clustering(cls, feats, clustering):
        """The memory of a ``cluster.Clustering`` of the rows ``feats`` (jaccard_dbscan's result): its noise rows are skipped."""
        return cls.from_labels(feats, clustering.labels.to(feats.device))

    def reset(self):
        """Zeroes the table in place (a device fill: a captured graph that holds it stays valid)."""
        self.centroids.zero_()

    def state(self):
        return {'centroids': self.centroids.detach().cpu().clone()}

    def load_state(self, state):
        """Copies ``state['centroids']`` into the table in place; a table of another shape is refused."""
        c = state['centroids']
        if tuple(c.shape) != (self.num_clusters, self.dim):
            raise ValueError(f'ClusterMemory: the state holds centroids {tuple(c.shape)}, this memory is [{self.num_clusters}, {self.dim}]')
        self.centroids.copy_(c.to(torch.float32))


class ClusterNCEFn(torch.autograd.Function):
    """(loss, n_used) of the cluster-contrast loss of x [S, N, D] (S sides stacked, ``labels`` [N] shared) against ``memory``
    (csrc/cluster_nce.hip; the reference has no such loss): the mean over the used rows of lse_c(x^ . C_c / tau) - x^ . C_y / tau, a row
    used when it is valid and its label lies in the memory.  With ``update`` the centroids the forward used are then moved by momentum
    (``mode`` 'mean' | 'hard').  The centroids are constants of the loss: the gradient reaches x only, from what the forward left in
    its workspace (the memory may have moved before the backward runs).  Without gradients the table is streamed once and nothing is
    kept.  n_used is a float tensor; nothing is read back to the host.  ``rows_out``: an optional trailing dict that receives COPIES of
    ``row_loss`` and ``target_cos`` (cluster_nce); the call the model makes is ``apply(x, labels, valid, memory, tau, momentum, mode,
    update)``."""
    @staticmethod
    def forward(ctx, x, labels, valid, memory, tau: float, momentum: float, mode: str, update: bool, rows_out=None):
        (S, N, D), dev = x.shape, x.device
        if D != memory.dim:
            raise _lib.ReidHipError(f'ClusterNCEFn: the memory holds centroids of D={memory.dim}, the batch has D={D}')
        with_grad = bool(ctx.needs_input_grad[0])
        x2 = x.reshape(S * N, D).contiguous().float()
        labels = labels.contiguous()
        vv = None if valid is None else valid.reshape(S * N).contiguous()
        ws = torch.empty(ops.cluster_nce_ws_floats(S, N, D, memory.num_clusters), device=dev)
        row_loss = torch.empty(S * N, device=dev); tcos = torch.empty(S * N, device=dev); res = torch.empty(2, device=dev)
        ops.cluster_nce_fwd(x2, labels, vv, memory.centroids, tau, with_grad, ws, row_loss, tcos, res, S=S)
        if update:
            ops.cluster_nce_update(labels, vv, row_loss, tcos, ws, memory.centroids, momentum, mode, S=S)
        ctx.save_for_backward(ws, res)
        ctx.shape, ctx.with_grad = (S, N, D), with_grad
        loss, n_used = res[0], res[1]
        ctx.mark_non_differentiable(n_used)
        if rows_out is not None:
            rows_out.update(row_loss=row_loss.view(S, N).clone(), target_cos=tcos.view(S, N).clone())
        return loss, n_used

    @staticmethod
    def backward(ctx, dloss, _dn):
        ws, res = ctx.saved_tensors
        S, N, D = ctx.shape
        dx = torch.empty(S * N, D, device=ws.device)
        ops.cluster_nce_bwd(ws, res, dloss.reshape(1).float().contiguous(), dx, S=S)
        return dx.view(S, N, D), None, None, None, None, None, None, None, None


def cluster_nce(x, labels, memory, valid=None, temperature=0.05, momentum=0.1, mode='mean', update=True):
    """Cluster-contrast loss (ClusterNCE) for users with their own loop: ``x`` [S, N, D] (S sides stacked; [N, D] = one side) of the N
    instances with pseudo-labels ``labels`` [N], ``memory`` a ClusterMemory(K, D).  A row is used when it is valid (``valid`` [S, N] or
    [N] for one side: optional bool / uint8) and its label lies in 0..K-1 -- a DBSCAN noise label of -1 is simply unused;
    loss = mean over the used rows of lse_c(x^ . C_c / temperature) - x^ . C_y / temperature, 0 when no row is used.  With ``update``
    (and gradients enabled) the centroids of the labels in the batch then move: 'mean' blends c <- m c + (1 - m) x^, renormalised, over
    the label's rows in ascending row order; 'hard' blends once with the row of the smallest x^ . C_y; rows with a non-finite loss
    are left out; ``update=False`` leaves the memory as it is.  Returns (loss, LazyCount(n_used), rows) with rows = {'row_loss',
    'target_cos'} [S, N] (copies); the loss carries the gradient to ``x``."""
    _need_device('cluster_nce', x, labels, valid)
    if not isinstance(memory, ClusterMemory):
        raise TypeError('cluster_nce: memory must be a ClusterMemory')
    if not memory.centroids.is_cuda:
        raise _lib.ReidHipError('cluster_nce needs the memory on the device (there is no CPU path)')
    flat = x.dim() == 2
    if flat:
        x = x.unsqueeze(0)
    if x.dim() != 3 or labels.shape != x.shape[1:2]:
        raise ValueError('cluster_nce: x [S, N, D] or [N, D], labels [N]')
    if valid is not None:
        valid = valid.to(torch.uint8).reshape(x.shape[0], x.shape[1]).contiguous()
    temperature, momentum, mode = cluster_nce_args('cluster_nce', temperature, momentum, mode)
    rows = {}
    loss, n_used = ClusterNCEFn.apply(x, labels.long(), valid, memory, temperature, momentum, mode,
                                      bool(update and torch.is_grad_enabled()), rows)
    if flat:
        rows = {k: v[0] for k, v in rows.items()}
    return loss, LazyCount(n_used), rows


# ----------------------------------------------------------------------------------------------------------------
def hybrid_nce_args(who, temperature, momentum):
    """The checked (temperature, momentum) of the hybrid memory loss."""
    return cluster_nce_args(who, temperature, momentum, 'mean')[:2]


class HybridMemory:
    """The hybrid memory of hybrid_nce (SpCL, Ge et al. 2020, sections 3.1-3.2; csrc/hybrid_nce.hip): one unit
    entry per training INSTANCE, ``instances`` f32 [num_instances, dim], which persists across re-clusterings and is only re-labelled
    (``set_labels``); ``labels`` i64 [num_instances] the class of every instance in 0..num_classes-1 -- a cluster, or a class of its
    own for an un-clustered instance (``Clustering.hybrid_labels()``); ``table`` f32 [num_classes, dim] the class vectors = the fp32
    mean of the members' entries added in ascending instance index, NOT renormalised, kept exact after every update; ``counts`` i64
    [num_classes].  Plain tensors moved by the momentum update only, not by the optimizer; ``state()`` / ``load_state()`` carry entries
    and labels through a checkpoint (``hybrid_memory_state_dict``).  A new memory holds zero entries, all in class 0.  It may be
    constructed on the CPU to carry a state (its table then stays zero); the kernels need the device."""

    def __init__(self, num_instances, dim, device='cuda'):
        if not (num_instances >= 1 and dim % 32 == 0 and 32 <= dim <= 1024):
            raise ValueError('HybridMemory: num_instances >= 1, dim a multiple of 32 in 32..1024')
        self.num_instances, self.dim = int(num_instances), int(dim)
        self.instances = torch.zeros(self.num_instances, self.dim, dtype=torch.float32, device=torch.device(device))
        self._relabel(torch.zeros(self.num_instances, dtype=torch.int64, device=self.instances.device), 1)

    def _relabel(self, labels, C):
        """Installs checked labels: members grouped by class (a stable sort: ascending instance index inside a class), counts, and
        the table from the entries as they stand."""
        if C * self.dim >= 2 ** 31:
            raise ValueError(f'HybridMemory: num_classes * dim = {C} * {self.dim} must stay below 2^31')
        self.labels, self.num_classes = labels.contiguous(), int(C)
        self.counts = torch.bincount(self.labels, minlength=self.num_classes)
        self.order = torch.sort(self.labels, stable=True).indices.contiguous()
        self.offsets = torch.cat([self.counts.new_zeros(1), self.counts.cumsum(0)]).contiguous()
        self.table = torch.zeros(self.num_classes, self.dim, dtype=torch.float32, device=self.instances.device)
        if self.instances.is_cuda:
            ops.class_means(self.instances, self.order, self.offsets, self.table)

    def set_labels(self, labels):
        """Re-labels the memory after a re-clustering: the entries stay as they are; the members, the counts and the table (the number
        of classes may change) are rebuilt.  ``labels`` [num_instances]: classes 0..C-1 without gaps (Clustering.hybrid_labels()).
        A captured graph holds the old table: capture again."""
        if labels.shape != (self.num_instances,):
            raise ValueError(f'HybridMemory.set_labels: labels [{self.num_instances}], one per instance')
        labels = labels.to(self.instances.device).long()
        if int(labels.min()) < 0:
            raise ValueError('HybridMemory.set_labels: every instance needs a class >= 0; a -1 (DBSCAN noise) becomes a class of its '
                             'own with Clustering.hybrid_labels()')
        C = int(labels.max()) + 1
        counts = torch.bincount(labels, minlength=C)
        if bool((counts == 0).any()):
            raise ValueError(f'HybridMemory.set_labels: class {int((counts == 0).nonzero()[0])} has no instance (classes must be 0..C-1 without gaps)')
        self._relabel(labels.clone(), C)

    @classmethod
    def from_labels(cls, feats, labels):
        """The memory of the rows ``feats`` [M, D] (device): entries = l2_normalize(feats), classes ``labels`` [M] >= 0 without gaps."""
        _need_device('HybridMemory.from_labels', feats, labels)
        if feats.dim() != 2 or labels.shape != feats.shape[:1]:
            raise ValueError('HybridMemory.from_labels: feats [M, D], labels [M]')
        mem = cls(feats.shape[0], feats.shape[1], feats.device)
        ops.l2norm_rows(feats.float().contiguous(), y=mem.instances, eps=EPS)
        mem.set_labels(labels)
        return mem

    @classmethod
    def from_clustering(cls, feats, clustering):
        """The memory of a ``cluster.Clustering`` of the rows ``feats`` (jaccard_dbscan's result): every noise row is a class of its own."""
        return cls.from_labels(feats, clustering.hybrid_labels()[0].to(feats.device))

    def classes_of(self, index):
        """The classes of the dataset rows ``index`` (i64, on the memory's device), -1 for an index outside the memory; no host read."""
        ok = (index >= 0) & (index < self.num_instances)
        return torch.where(ok, self.labels[index.clamp(0, self.num_instances - 1)], torch.full_like(index, -1))

    def state(self):
        return {'instances': self.instances.detach().cpu().clone(), 'labels': self.labels.detach().cpu().clone()}

    def load_state(self, state):
        """Copies ``state['instances']`` into the entries in place and re-labels with ``state['labels']``; another shape is refused."""
        v = state['instances']
        if tuple(v.shape) != (self.num_instances, self.dim):
            raise ValueError(f'HybridMemory: the state holds instances {tuple(v.shape)}, this memory is [{self.num_instances}, {self.dim}]')
        self.instances.copy_(v.to(torch.float32))
        self.set_labels(state['labels'])


class HybridNCEFn(torch.autograd.Function):
    """(loss, n_used) of the hybrid memory loss of x [S, N, D] (S sides stacked, ``index`` [N] shared: the dataset row of each instance)
    against ``memory`` (csrc/hybrid_nce.hip): ClusterNCEFn's forward against the memory's table of class means with the labels
    memory.labels[index] -- a row is used when it is valid and its index lies in the memory.  With ``update`` the entries of the
    contributing instances are then moved by momentum and the class means of their classes re-formed from the moved entries, two
    kernels in stream order.  Entries and table are constants of the loss: the gradient reaches x only, from what the forward left in
    its workspace.  n_used is a float tensor; nothing is read back to the host.  ``rows_out``: an optional trailing dict that receives
    COPIES of ``row_loss``, ``target_cos`` and ``labels``; the call the model makes is ``apply(x, index, valid, memory, tau, momentum,
    update)``."""
    @staticmethod
    def forward(ctx, x, index, valid, memory, tau: float, momentum: float, update: bool, rows_out=None):
        (S, N, D), dev = x.shape, x.device
        if D != memory.dim:
            raise _lib.ReidHipError(f'HybridNCEFn: the memory holds entries of D={memory.dim}, the batch has D={D}')
        with_grad = bool(ctx.needs_input_grad[0])
        x2 = x.reshape(S * N, D).contiguous().float()
        index = index.contiguous()
        labels = memory.classes_of(index).contiguous()
        vv = None if valid is None else valid.reshape(S * N).contiguous()
        ws = torch.empty(ops.cluster_nce_ws_floats(S, N, D, memory.num_classes), device=dev)
        row_loss = torch.empty(S * N, device=dev); tcos = torch.empty(S * N, device=dev); res = torch.empty(2, device=dev)
        ops.cluster_nce_fwd(x2, labels, vv, memory.table, tau, with_grad, ws, row_loss, tcos, res, S=S)
        if update:
            ops.hybrid_update_instances(index, vv, row_loss, ws, memory.instances, momentum, S=S)
            ops.hybrid_refresh_classes(labels, vv, row_loss, memory.instances, memory.order, memory.offsets, memory.table, S=S)
        ctx.save_for_backward(ws, res)
        ctx.shape = (S, N, D)
        loss, n_used = res[0], res[1]
        ctx.mark_non_differentiable(n_used)
        if rows_out is not None:
            rows_out.update(row_loss=row_loss.view(S, N).clone(), target_cos=tcos.view(S, N).clone(), labels=labels.clone())
        return loss, n_used

    @staticmethod
    def backward(ctx, dloss, _dn):
        ws, res = ctx.saved_tensors
        S, N, D = ctx.shape
        dx = torch.empty(S * N, D, device=ws.device)
        ops.cluster_nce_bwd(ws, res, dloss.reshape(1).float().contiguous(), dx, S=S)
        return dx.view(S, N, D), None, None, None, None, None, None, None


def hybrid_nce(x, index, memory, valid=None, temperature=0.05, momentum=0.2, update=True):
    """Hybrid memory loss (SpCL) for users with their own loop: ``x`` [S, N, D] (S sides stacked; [N, D] = one side) of the N instances
    whose dataset rows are ``index`` [N], ``memory`` a HybridMemory(M, D).  A row is used when it is valid (``valid`` [S, N] or [N] for
    one side: optional bool / uint8) and 0 <= index < M; its label is memory.labels[index];
    loss = mean over the used rows of lse_c(x^ . T_c / temperature) - x^ . T_y / temperature against the class means T, 0 when no row
    is used.  With ``update`` (and gradients enabled) the entries of the batch's instances then move, v <- m v + (1 - m) x^,
    renormalised, over an instance's rows in ascending row order, and the means of their classes are re-formed; rows with a
    non-finite loss are left out; ``update=False`` leaves the memory as it is.  Returns (loss, LazyCount(n_used), rows) with rows =
    {'row_loss', 'target_cos'} [S, N] and 'labels' [N] (copies); the loss carries the gradient to ``x``."""
    _need_device('hybrid_nce', x, index, valid)
    if not isinstance(memory, HybridMemory):
        raise TypeError('hybrid_nce: memory must be a HybridMemory')
    if not memory.instances.is_cuda:
        raise _lib.ReidHipError('hybrid_nce needs the memory on the device (there is no CPU path)')
    flat = x.dim() == 2
    if flat:
        x = x.unsqueeze(0)
    if x.dim() != 3 or index.shape != x.shape[1:2]:
        raise ValueError('hybrid_nce: x [S, N, D] or [N, D], index [N]')
    if valid is not None:
        valid = valid.to(torch.uint8).reshape(x.shape[0], x.shape[1]).contiguous()
    temperature, momentum = hybrid_nce_args('hybrid_nce', temperature, momentum)
    rows = {}
    loss, n_used = HybridNCEFn.apply(x, index.long(), valid, memory, temperature, momentum, bool(update and torch.is_grad_enabled()), rows)
    if flat:
        rows = {k: (v if k == 'labels' else v[0]) for k, v in rows.items()}
    return loss, LazyCount(n_used), rows


# ----------------------------------------------------------------------------------------------------------------
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


class MarginCEFn(torch.autograd.Function):
    """(loss, count) of the label-smoothed CE of the margin logits of ``kind`` (cosine | cosface | arcface | circle; include/reid_hip.h
    has the definitions) of logits = scale * cos (head.CosineLinearFn's): the mean over the rows with valid != 0 and a label in [0, C).
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
    from .head import CosineLinearFn
    kind, scale, margin = margin_args('margin_cross_entropy', kind, scale, margin)
    if not 0 <= smoothing <= 1:
        raise ValueError(f'margin_cross_entropy: smoothing must be in [0, 1], not {smoothing}')
    _need_device('margin_cross_entropy', features, weight, labels, valid)
    if features.dim() != 2 or weight.dim() != 2 or weight.shape[1] != features.shape[1] or labels.shape != features.shape[:1] \
            or (valid is not None and valid.shape != labels.shape):
        raise ValueError('margin_cross_entropy: features [B, D], weight [C, D], labels [B], valid [B]')
    if valid is not None:
        valid = valid.to(torch.uint8).contiguous()
    logits = CosineLinearFn.apply(features, weight, scale)
    loss, cnt = MarginCEFn.apply(logits, labels.long(), valid, float(smoothing), kind, scale, margin)
    return loss, LazyCount(cnt), logits
