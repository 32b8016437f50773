"""fp64 reference of the cross-modal triplet loss with a cross-batch memory (include/reid_hip.h, reid_xbm_*), written plainly in torch
and sharing no code with the package (helpers of cross_triplet_ref.py only).

    sides: 0 = vis, 1 .. P = the non-vis modalities.  The memory of capacity M: rows [P+1, M, D], labels [M], valid [P+1, M], cursor =
    (next slot, rows ever written).  The shadow ring here holds the RAW fp32 rows; the unit rows x / max(|x|, eps) are formed in fp64
    where they are used.
    enqueue: row i of every side -> slot (cursor + i) mod M; labels and validity alongside; the cursor advances by N (FIFO).
    mining (after the enqueue: the batch is part of the memory): pair p, q->mem: every valid row of q[p] against the valid slots of
    side 0; g->mem: every valid row of g against the valid slots of side p + 1.  Hardest positive: same label, largest d2; hardest
    negative: other label, smallest d2; ties -> lowest slot; no self-exclusion.  Indices are slots, -1 = inactive.
    row loss max(0, d_ap - d_an + margin) or softplus (margin None); L_p = 0.5 (mean over the active q anchors + mean over the active g
    anchors); flag_p = [any active].
    gradient: the memory is constant -- an anchor gets c l' ((x^ - m_p) / d_ap - (x^ - m_n) / d_an), a term dropped where its d2 was
    clamped; a vis row adds its terms over the pairs; then back through the normalisation.
"""
import math

import torch

import cross_triplet_ref as R

CLAMP, EPS, U = R.CLAMP, R.EPS, R.U


class Ring:
    """The shadow ring: raw fp32 rows."""

    def __init__(self, P, M, D, device='cpu'):
        self.P, self.M, self.D = P, M, D
        self.rows = torch.zeros(P + 1, M, D, dtype=torch.float32, device=device)
        self.labels = torch.zeros(M, dtype=torch.int64, device=device)
        self.valid = torch.zeros(P + 1, M, dtype=torch.bool, device=device)
        self.cursor, self.written = 0, 0

    def slots(self, N):
        """The slots the NEXT batch of N rows goes to."""
        return (self.cursor + torch.arange(N, device=self.rows.device)) % self.M

    def enqueue(self, q, g, labels, q_valid=None, g_valid=None):
        P, N, _ = q.shape
        assert P == self.P and g.shape[0] == N <= self.M
        s = self.slots(N)
        self.rows[0, s] = g.float()
        self.rows[1:, s] = q.float()
        self.labels[s] = labels.to(self.labels.device)
        self.valid[0, s] = R._valid(g_valid, (N,), self.rows.device)
        self.valid[1:, s] = R._valid(q_valid, (P, N), self.rows.device)
        self.cursor, self.written = (self.cursor + N) % self.M, self.written + N
        return s

    def clone(self):
        c = Ring(self.P, self.M, self.D, self.rows.device)
        c.rows, c.labels, c.valid, c.cursor, c.written = self.rows.clone(), self.labels.clone(), self.valid.clone(), self.cursor, self.written
        return c


def mine(ring, q, g, labels, q_valid=None, g_valid=None, normalize=True, eps=EPS):
    """The selection of every pair and direction against the ring as it stands: q_idx_p / q_idx_n / q_gap_p / q_gap_n and g_* [P, N]."""
    P, N, _ = q.shape
    dev = q.device
    qh, _ = R.unit_rows(q, normalize, eps); gh, _ = R.unit_rows(g, normalize, eps)
    mh, _ = R.unit_rows(ring.rows, normalize, eps)
    qv, gv = R._valid(q_valid, (P, N), dev), R._valid(g_valid, (N,), dev)
    lab = labels.to(dev)
    out = {k: [] for k in ('q_idx_p', 'q_idx_n', 'q_gap_p', 'q_gap_n', 'g_idx_p', 'g_idx_n', 'g_gap_p', 'g_gap_n')}
    for p in range(P):
        for side, vals in (('q', R.mine_direction(R.pairwise_d2(qh[p], mh[0]), lab, ring.labels, qv[p], ring.valid[0])),
                           ('g', R.mine_direction(R.pairwise_d2(gh, mh[p + 1]), lab, ring.labels, gv, ring.valid[p + 1]))):
            for k, v in zip(('idx_p', 'idx_n', 'gap_p', 'gap_n'), vals):
                out[f'{side}_{k}'].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def evaluate(ring, q, g, sel, margin, normalize=True, eps=EPS):
    """Distances, row losses, L [P], flag [P], n_q / n_g [P] (all fp64) for a GIVEN selection of slots."""
    P = q.shape[0]
    qh, _ = R.unit_rows(q, normalize, eps); gh, _ = R.unit_rows(g, normalize, eps)
    mh, _ = R.unit_rows(ring.rows, normalize, eps)
    out = {k: [] for k in ('q_d_ap', 'q_d_an', 'q_row_loss', 'q_d2p', 'q_d2n', 'g_d_ap', 'g_d_an', 'g_row_loss', 'g_d2p', 'g_d2n')}
    L, n_q, n_g = [], [], []
    for p in range(P):
        sums = []
        for side, A, C in (('q', qh[p], mh[0]), ('g', gh, mh[p + 1])):
            ip, inn = sel[f'{side}_idx_p'][p].long().to(A.device), sel[f'{side}_idx_n'][p].long().to(A.device)
            act = ip >= 0
            a = torch.nonzero(act).flatten()
            z = torch.zeros(A.shape[0], dtype=torch.float64, device=A.device)
            d2p, d2n, d_ap, d_an, rl = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
            d2p[a] = ((A[a] - C[ip[a]]) ** 2).sum(-1); d2n[a] = ((A[a] - C[inn[a]]) ** 2).sum(-1)
            d_ap[a] = d2p[a].clamp(min=CLAMP).sqrt(); d_an[a] = d2n[a].clamp(min=CLAMP).sqrt()
            rl[a] = R.row_loss_fn(d_ap[a] - d_an[a], margin)
            n = int(act.sum())
            sums.append(float(rl.sum()) / max(1, n))
            (n_q if side == 'q' else n_g).append(n)
            for k, v in (('d_ap', d_ap), ('d_an', d_an), ('row_loss', rl), ('d2p', d2p), ('d2n', d2n)):
                out[f'{side}_{k}'].append(v)
        L.append(0.5 * (sums[0] + sums[1]) if n_q[-1] + n_g[-1] > 0 else 0.0)
    res = {k: torch.stack(v) for k, v in out.items()}
    res.update(L=L, flag=[1.0 if a + b > 0 else 0.0 for a, b in zip(n_q, n_g)], n_q=n_q, n_g=n_g)
    return res


def reference(ring, q, g, labels, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    sel = mine(ring, q, g, labels, q_valid, g_valid, normalize, eps)
    out = evaluate(ring, q, g, sel, margin, normalize, eps)
    out.update(sel)
    return out


def gradient(ring, q, g, margin, normalize, sel, gscale=None, eps=EPS):
    """(dq [P, N, D], dg [N, D]) fp64 of sum_p gscale[p] L_p at a GIVEN selection, the memory constant: only the anchors' own terms,
    through the normalisation (dx = (G - x^ (x^ . G)) / |x| where |x| >= eps, G / eps below)."""
    P = q.shape[0]
    e = evaluate(ring, q, g, sel, margin, normalize, eps)
    qh, qn = R.unit_rows(q, normalize, eps); gh, gn = R.unit_rows(g, normalize, eps)
    mh, _ = R.unit_rows(ring.rows, normalize, eps)
    gs = [1.0] * P if gscale is None else [float(v) for v in gscale]
    Gq, Gg = torch.zeros_like(qh), torch.zeros_like(gh)
    for p in range(P):
        for side, A, C, GA, n in (('q', qh[p], mh[0], Gq[p], e['n_q'][p]), ('g', gh, mh[p + 1], Gg, e['n_g'][p])):
            ip, inn = sel[f'{side}_idx_p'][p].long().to(A.device), sel[f'{side}_idx_n'][p].long().to(A.device)
            a = torch.nonzero(ip >= 0).flatten()
            dp, dn = e[f'{side}_d_ap'][p][a], e[f'{side}_d_an'][p][a]
            c = gs[p] * 0.5 * R.row_dloss_fn(dp - dn, margin) / max(1, n)
            sp = torch.where(e[f'{side}_d2p'][p][a] > CLAMP, c / dp, torch.zeros_like(c))
            sn = torch.where(e[f'{side}_d2n'][p][a] > CLAMP, c / dn, torch.zeros_like(c))
            GA.index_add_(0, a, sp[:, None] * (A[a] - C[ip[a]]) - sn[:, None] * (A[a] - C[inn[a]]))
    if not normalize:
        return Gq, Gg

    def project(G, xh, n):
        proj = (G - xh * (xh * G).sum(-1, keepdim=True)) / n.clamp(min=eps)[..., None]
        return torch.where((n >= eps)[..., None], proj, G / eps)
    return project(Gq, qh, qn), project(Gg, gh, gn)


class LoopRing:
    """The second implementation: the ring as plain Python lists, filled row by row."""

    def __init__(self, P, M, D):
        self.P, self.M = P, M
        self.rows = [[[0.0] * D for _ in range(M)] for _ in range(P + 1)]
        self.labels = [0] * M
        self.valid = [[False] * M for _ in range(P + 1)]
        self.cursor, self.written = 0, 0

    def enqueue(self, q, g, labels, q_valid=None, g_valid=None):
        P, N = q.shape[0], q.shape[1]
        for i in range(N):
            s = (self.cursor + i) % self.M
            self.labels[s] = int(labels[i])
            for side in range(P + 1):
                x = g[i] if side == 0 else q[side - 1, i]
                v = g_valid if side == 0 else (None if q_valid is None else q_valid.reshape(P, N)[side - 1])
                self.rows[side][s] = [float(t) for t in x.double().tolist()]
                self.valid[side][s] = True if v is None else bool(v[i])
        self.cursor, self.written = (self.cursor + N) % self.M, self.written + N


def loop_reference(ring, q, g, labels, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    """The same definition with plain Python loops over lists, against a LoopRing (small inputs only)."""
    def unit(r):
        return [v / max(math.sqrt(sum(c * c for c in r)), eps) for v in r] if normalize else list(r)

    P, N = q.shape[0], q.shape[1]
    LAB = [int(v) for v in labels.tolist()]
    QV = [[True] * N for _ in range(P)] if q_valid is None else [[bool(v) for v in r] for r in q_valid.reshape(P, N).tolist()]
    GV = [True] * N if g_valid is None else [bool(v) for v in g_valid.tolist()]
    MEM = [[unit(r) for r in side] for side in ring.rows]

    def direction(A, AV, C, CV):
        idx_p, idx_n, d_ap, d_an, rl = [-1] * N, [-1] * N, [0.0] * N, [0.0] * N, [0.0] * N
        for i in range(N):
            if not AV[i]:
                continue
            bp, jp, bn, jn = -1.0, -1, math.inf, -1
            for j in range(ring.M):
                if not CV[j]:
                    continue
                d2 = sum((a - b) ** 2 for a, b in zip(A[i], C[j]))
                if ring.labels[j] == LAB[i]:
                    if d2 > bp:
                        bp, jp = d2, j
                elif d2 < bn:
                    bn, jn = d2, j
            if jp < 0 or jn < 0:
                continue
            idx_p[i], idx_n[i] = jp, jn
            d_ap[i], d_an[i] = math.sqrt(max(bp, CLAMP)), math.sqrt(max(bn, CLAMP))
            z = d_ap[i] - d_an[i]
            rl[i] = max(0.0, z + margin) if margin is not None else max(z, 0.0) + math.log1p(math.exp(-abs(z)))
        return idx_p, idx_n, d_ap, d_an, rl

    out = {k: [] for k in ('q_idx_p', 'q_idx_n', 'q_d_ap', 'q_d_an', 'q_row_loss', 'g_idx_p', 'g_idx_n', 'g_d_ap', 'g_d_an', 'g_row_loss',
                           'L', 'flag', 'n_q', 'n_g')}
    G = [unit([float(t) for t in r]) for r in g.double().tolist()]
    for p in range(P):
        Q = [unit([float(t) for t in r]) for r in q[p].double().tolist()]
        sums, counts = [], []
        for side, vals in (('q', direction(Q, QV[p], MEM[0], ring.valid[0])), ('g', direction(G, GV, MEM[p + 1], ring.valid[p + 1]))):
            for k, v in zip(('idx_p', 'idx_n', 'd_ap', 'd_an', 'row_loss'), vals):
                out[f'{side}_{k}'].append(v)
            n = sum(1 for j in vals[0] if j >= 0)
            counts.append(n); sums.append(sum(vals[4]) / max(1, n))
        out['n_q'].append(counts[0]); out['n_g'].append(counts[1])
        out['flag'].append(1.0 if sum(counts) > 0 else 0.0)
        out['L'].append(0.5 * (sums[0] + sums[1]) if sum(counts) > 0 else 0.0)
    return out


# ---- the stream of the tests
STEPS = 5
# (P, N, D, M, pad) of the GPU tests: one row; a batch that wraps from the fourth step on; a batch that wraps mid-way (M = 160, N = 64); a
# ring that wraps at every step (M = 8, N = 6)
SHAPES = [(1, 1, 4, 1, 0), (2, 16, 96, 48, 8), (4, 64, 512, 160, 0), (1, 6, 1024, 8, 0)]


def stream_step(P, N, D, ratio, s, device='cpu'):
    """Batch s = 1, 2, ... of the stream: cross_triplet_ref.make_case(P, N, N, D, ratio, 100 + s) with the labels shifted by 2 (s mod
    2), so that the identities of consecutive batches overlap.  Returns q [P, N, D], g [N, D], labels [N]."""
    q, g, ql, _ = R.make_case(P, N, N, D, ratio, 100 + s, device=device)
    return q, g, ql + 2 * (s % 2)
