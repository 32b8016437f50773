"""fp64 numpy restatement of the cross-modal Smooth-AP loss (csrc/smooth_ap.hip): the loss, the per-anchor AP, the
gradient by the closed form, the ring form, and the error bounds of the fp32 kernels.

The bounds are running error bounds: every term is (a count of roundings) * u times the magnitude it applies to, propagated through the
reference's own fp64 intermediates of the case -- no constant is taken from a run of the code under test.  u = 2^-24.  The chain:
  score      one rounding of the fp64 cosine to fp32, plus the fp64 work itself:  es = u |s| + (D + 8) 2^-53 |x^| |g^|
  d          fl(fl(s_j - s_i) * fl(1 / tau)): three roundings:  ed = (es_i + es_j) / tau + 3 u |d|
  sigma      e = exp(-|d|) (<= 1 ulp = 2 u), 1 + e, the division, and for d < 0 the product e r:  <= 6 u relative;
             through d:  sigma' ed + M2 ed^2 / 2  with M2 = max |sigma''| = 1 / (6 sqrt 3)
  t          t = sigma (1 - sigma) = (e r) r:  <= 10 u relative;  through d:  |t'| ed + M3 ed^2 / 2,  M3 = max |sigma'''| = 1 / 8
  sums over j   per-lane chains of ceil(G / 64) terms, 6 butterfly levels (and the "1 +"):  (ceil(G / 64) + 7) u of the (positive) sum
  quotients  R+ / R, 1 / R, (R+ / R) (1 / R): one rounding each on top of the propagated errors
  AP_a       an fp64 mean, rounded once;  L_dir an fp64 mean;  L_p rounded once
  ds         the fma chain over the |P| positives, ka = fl(fl(1 / tau) / |P|) (2 u), the product (1 u), the positive's own term
             ka (v A - u B) with A, B sums over j as above
  gathers    weights c * ds (c = 0.5 / n: 1 u, the product 1 u), fma chains of ceil(n / 4) + 4 terms per column, unit rows of the batch
             off by E_UNIT relative (ring rows are exact: they ARE what the kernel reads)
  projection dot = x^ . G (4 ceil(D / 256) + 6 terms), G - x^ dot, the scaling by 1 / max(|x|, eps);  then gscale (fma chain over p)
"""
import math

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-12))
E_SIG, E_T = 6, 10                                   # roundings (in u) of sigma and of t = sigma (1 - sigma) as the kernel forms them
M2, M3 = 1 / (6 * math.sqrt(3)), 1 / 8               # max |sigma''|, max |sigma'''|


def tau32(tau):
    """The temperature the kernel sees: the fp32 value of ``tau``."""
    return float(np.float32(tau))


def e_unit(D):
    """Relative error of a component of an fp32 unit row (triplet::unit_row): the sum of squares (4 ceil(D / 256) products and additions
    per lane, 6 butterfly levels) enters halved through the square root; the root, the reciprocal, the product: one rounding each."""
    return ((8 * math.ceil(D / 256) + 6) / 2 + 3) * U


def n_sum(G):
    return math.ceil(G / 64) + 7


def unit_rows(x, normalize=True, eps=EPS):
    """(x^ fp64, 1 / max(|x|, eps), |x|) of the rows of x [..., D]; normalize False: (x, 1, |x|)."""
    x = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x * x).sum(-1))
    if not normalize:
        return x, np.ones_like(n), n
    inv = 1.0 / np.maximum(n, eps)
    return x * inv[..., None], inv, n


def _sig_parts(d):
    e = np.exp(-np.abs(d))
    r = 1.0 / (1.0 + e)
    return np.where(d >= 0, r, e * r), e * r * r


def rank_anchor(s, es, pos, valid, tau, D, with_bounds=True):
    """One anchor: scores s [G] (fp64), their error bounds es [G], positives pos [G] bool, valid [G] bool (pos is a subset), tau.
    Returns dict(ap, ds [G], e_ap, e_ds [G]) -- the closed form of the issue, and the running error bounds of the kernel's arithmetic."""
    G = s.shape[0]
    idx = np.flatnonzero(pos)
    n_p = idx.size
    d = (s[None, :] - s[idx][:, None]) / tau                         # [|P|, G]: row i, column j
    live = np.broadcast_to(valid[None, :], d.shape).copy()
    live[np.arange(n_p), idx] = False                                # j != i
    d = np.where(live, d, 0.0)
    sig, t = _sig_parts(d)
    sig, t = np.where(live, sig, 0.0), np.where(live, t, 0.0)
    R, Rp = 1 + sig.sum(1), 1 + sig[:, pos].sum(1)
    ratio = Rp / R
    ap = ratio.mean()
    coef = (pos[None, :] * R[:, None] - Rp[:, None]) / (R * R)[:, None]
    w = t / tau * coef
    ds = -w.sum(0) / n_p
    ds[idx] += w.sum(1) / n_p
    out = dict(ap=ap, ds=ds, npos=n_p)
    if not with_bounds:
        return out
    ed = np.where(live, (es[None, :] + es[idx][:, None]) / tau + 3 * U * np.abs(d), 0.0)
    dsig = t * ed + 0.5 * M2 * ed * ed + E_SIG * U * sig
    ns = n_sum(G) * U
    dR, dRp = dsig.sum(1) + ns * R, dsig[:, pos].sum(1) + ns * Rp
    assert (dR < 0.5 * R).all(), 'the rank bound is void: scores too close for this tau'
    dratio = (dRp + ratio * dR) / (R - dR) + U * ratio
    out['e_ap'] = dratio.mean() + U * ap
    # the gradient
    dt = np.abs(t * (1 - 2 * sig)) * ed + 0.5 * M3 * ed * ed + E_T * U * t
    v, u_ = 1 / R, ratio / R
    dv = dR / (R * (R - dR)) + U * v
    du = dratio * v + ratio * dv + dratio * dv + U * u_
    cp, cn = v - u_, -u_                                             # the coefficient of a positive / a negative column
    dcp, dcn = dv + du + U * np.abs(cp), du
    c_abs = np.where(pos[None, :], np.abs(cp)[:, None], np.abs(cn)[:, None])
    dc = np.where(pos[None, :], dcp[:, None], dcn[:, None])
    acc_abs = (t * c_abs).sum(0)
    dacc = (dt * c_abs + t * dc + dt * dc).sum(0) + n_p * U * acc_abs
    ka = 1 / (tau * n_p)
    e_ds = ka * dacc + 3 * U * ka * acc_abs
    A, B = t[:, pos].sum(1), t.sum(1)
    nt = (n_sum(G) - 1) * U
    dA, dB = dt[:, pos].sum(1) + nt * A, dt.sum(1) + nt * B
    dvA = dv * A + v * dA + dv * dA + U * v * A
    duB = du * B + u_ * dB + du * dB + U * u_ * B
    diag = ka * (v * A - u_ * B)
    ddiag = ka * (dvA + duB + U * np.abs(v * A - u_ * B)) + 3 * U * np.abs(diag)
    e_ds[idx] += ddiag + U * np.abs(ds[idx])
    out['e_ds'] = e_ds
    return out


def direction(a_hat, a_norm, a_lab, a_valid, c_hat, c_norm, c_lab, c_valid, tau, with_bounds=True):
    """The ranking problems of one direction of one pair: anchors a_hat [A, D] (rows in score space, their norms a_norm) against the
    gallery c_hat [G, D].  Returns dict(ap [A] (-1: inactive), npos [A], ds [A, G], e_ap [A], e_ds [A, G], s [A, G])."""
    A, D = a_hat.shape
    G = c_hat.shape[0]
    a_on = np.ones(A, bool) if a_valid is None else np.asarray(a_valid) != 0
    c_on = np.ones(G, bool) if c_valid is None else np.asarray(c_valid) != 0
    ah, ch = np.where(a_on[:, None], a_hat, 0.0), np.where(c_on[:, None], c_hat, 0.0)      # (invalid rows may hold anything)
    s = ah @ ch.T
    es = U * np.abs(s) + (D + 8) * 2.0 ** -53 * np.where(a_on, a_norm, 0.0)[:, None] * np.where(c_on, c_norm, 0.0)[None, :]
    ap, npos = np.full(A, -1.0), np.zeros(A, np.int64)
    ds, e_ds, e_ap = np.zeros((A, G)), np.zeros((A, G)), np.zeros(A)
    for a in range(A):
        if not a_on[a]:
            continue
        pos = c_on & (np.asarray(c_lab) == a_lab[a])
        npos[a] = pos.sum()
        if npos[a] == 0 or npos[a] == c_on.sum():
            continue
        r = rank_anchor(s[a], es[a], pos, c_on, tau, D, with_bounds)
        ap[a], ds[a] = r['ap'], r['ds']
        if with_bounds:
            e_ap[a], e_ds[a] = r['e_ap'], r['e_ds']
    return dict(ap=ap, npos=npos, ds=ds, e_ap=e_ap, e_ds=e_ds, s=s, c_on=c_on, a_on=a_on)


def _project(G, EG, xhat, inv, norm, normalize, eps, D, eu):
    """(dx, its bound) of the unit-space gradient G [rows, D] with bound EG through x^ = x / max(|x|, eps)."""
    if not normalize:
        return G, EG
    dot = (xhat * G).sum(-1, keepdims=True)
    big = (norm >= eps)[:, None]
    out = np.where(big, (G - xhat * dot) * inv[:, None], G / eps)
    xa = np.abs(xhat)
    ddot = (xa * EG + eu * xa * np.abs(G)).sum(-1, keepdims=True) + (4 * math.ceil(D / 256) + 6) * U * (xa * np.abs(G)).sum(-1, keepdims=True)
    e_big = inv[:, None] * (EG + xa * ddot + eu * xa * np.abs(dot) + 2 * U * (np.abs(G) + xa * np.abs(dot))) + (eu + U) * np.abs(out)
    return out, np.where(big, e_big, EG / eps + U * np.abs(out))


def forward(q, g, q_lab, g_lab, q_valid=None, g_valid=None, tau=0.01, normalize=True, ring=None, gscale=None, with_bounds=True, eps=EPS):
    """The whole loss.  q [P, N, D], g [Mg, D] (fp32 or fp64 values), labels, optional validity [P, N] / [Mg]; ``ring`` = (rows
    [P + 1, M, D] as the kernel reads them, labels [M], valid [P + 1, M]) selects the ring form (then g_lab = q_lab, Mg = N).  gscale [P]:
    the cotangent of the losses (default ones).  Returns loss / flag [P], n_active [P, 2], q_ap / q_npos [P, N], g_ap / g_npos [P, Mg],
    dq [P, N, D], dg [Mg, D], the per-direction dicts ``dirs[p] = (q->g, g->q)``, and the bounds e_loss [P], e_q_ap, e_g_ap, e_dq
    [P, N, D], e_dg [Mg, D] (element-wise)."""
    tau = tau32(tau)
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    P, N, D = q.shape
    Mg = g.shape[0]
    gscale = np.ones(P) if gscale is None else np.asarray(gscale, np.float64)
    qh, qinv, qn = unit_rows(q, normalize, eps)
    gh, ginv, gn = unit_rows(g, normalize, eps)
    qv = np.ones((P, N), bool) if q_valid is None else np.asarray(q_valid).reshape(P, N) != 0
    gv = np.ones(Mg, bool) if g_valid is None else np.asarray(g_valid) != 0
    eu = e_unit(D) if normalize else 0.0
    out = dict(loss=np.zeros(P), flag=np.zeros(P), n_active=np.zeros((P, 2)), q_ap=np.zeros((P, N)), g_ap=np.zeros((P, Mg)),
               q_npos=np.zeros((P, N), np.int64), g_npos=np.zeros((P, Mg), np.int64), dq=np.zeros((P, N, D)), dg=np.zeros((Mg, D)),
               e_loss=np.zeros(P), e_q_ap=np.zeros((P, N)), e_g_ap=np.zeros((P, Mg)), e_dq=np.zeros((P, N, D)), e_dg=np.zeros((Mg, D)), dirs=[])
    e_dg_abs = np.zeros((Mg, D))
    for p in range(P):
        if ring is None:
            A = (gh, np.sqrt((gh * gh).sum(-1)), g_lab, gv, eu)
            B = (qh[p], np.sqrt((qh[p] * qh[p]).sum(-1)), q_lab, qv[p], eu)
        else:
            rows, rl, rv = ring
            rows = np.asarray(rows, np.float64)
            A = (rows[0], np.sqrt((rows[0] ** 2).sum(-1)), rl, np.asarray(rv)[0], 0.0)
            B = (rows[p + 1], np.sqrt((rows[p + 1] ** 2).sum(-1)), rl, np.asarray(rv)[p + 1], 0.0)
        d0 = direction(qh[p], np.sqrt((qh[p] ** 2).sum(-1)), q_lab, qv[p], A[0], A[1], A[2], A[3], tau, with_bounds)
        d1 = direction(gh, np.sqrt((gh ** 2).sum(-1)), g_lab, gv, B[0], B[1], B[2], B[3], tau, with_bounds)
        out['dirs'].append((d0, d1))
        act0, act1 = d0['ap'] >= 0, d1['ap'] >= 0
        n0, n1 = int(act0.sum()), int(act1.sum())
        L0 = (1 - d0['ap'][act0]).mean() if n0 else 0.0
        L1 = (1 - d1['ap'][act1]).mean() if n1 else 0.0
        out['loss'][p] = 0.5 * (L0 + L1) if n0 + n1 else 0.0
        out['flag'][p] = 1.0 if n0 + n1 else 0.0
        out['n_active'][p] = (n0, n1)
        out['q_ap'][p], out['g_ap'][p], out['q_npos'][p], out['g_npos'][p] = d0['ap'], d1['ap'], d0['npos'], d1['npos']
        out['e_q_ap'][p], out['e_g_ap'][p] = d0['e_ap'], d1['e_ap']
        out['e_loss'][p] = 0.5 * ((d0['e_ap'][act0].mean() if n0 else 0.0) + (d1['e_ap'][act1].mean() if n1 else 0.0)) + U * out['loss'][p]
        # unit-space gradients: as anchors against the gallery, and (batch form) as gallery rows of the other direction
        c0, c1 = 0.5 / max(n0, 1), 0.5 / max(n1, 1)
        XA, XB = np.where(d0['c_on'][:, None], A[0], 0.0), np.where(d1['c_on'][:, None], B[0], 0.0)

        def term(c, ds, e_ds, X, ex):
            n = ds.shape[1]
            k = (ex + 2 * U + (math.ceil(n / 4) + 4) * U)
            return c * ds @ X, c * (e_ds + k * np.abs(ds)) @ np.abs(X)

        Gq, EGq = term(c0, d0['ds'], d0['e_ds'], XA, A[4])
        Gg, EGg = term(c1, d1['ds'], d1['e_ds'], XB, B[4])
        if ring is None:
            qa, ga = np.where(d0['a_on'][:, None], qh[p], 0.0), np.where(d1['a_on'][:, None], gh, 0.0)
            t2 = term(c1, d1['ds'].T, d1['e_ds'].T, ga, eu)
            Gq, EGq = Gq + t2[0], EGq + t2[1] + U * np.abs(t2[0])
            t2 = term(c0, d0['ds'].T, d0['e_ds'].T, qa, eu)
            Gg, EGg = Gg + t2[0], EGg + t2[1] + U * np.abs(t2[0])
        Hq, EHq = _project(Gq, EGq, np.where(qv[p][:, None], qh[p], 0.0), qinv[p], qn[p], normalize, eps, D, eu)
        Hg, EHg = _project(Gg, EGg, np.where(gv[:, None], gh, 0.0), ginv, gn, normalize, eps, D, eu)
        Hq, EHq = np.where(qv[p][:, None], Hq, 0.0), np.where(qv[p][:, None], EHq, 0.0)
        Hg, EHg = np.where(gv[:, None], Hg, 0.0), np.where(gv[:, None], EHg, 0.0)
        out['dq'][p] = gscale[p] * Hq
        out['e_dq'][p] = abs(gscale[p]) * EHq + U * np.abs(out['dq'][p])
        out['dg'] += gscale[p] * Hg
        out['e_dg'] += abs(gscale[p]) * EHg
        e_dg_abs += np.abs(gscale[p] * Hg)
    out['e_dg'] += P * U * e_dg_abs
    return out


def naive_loss_torch(q, g, q_lab, g_lab, q_valid, g_valid, tau, normalize=True, ring=None, eps=EPS):
    """The definition written naively on torch fp64 tensors (q, g may require a gradient): the losses [P]."""
    import torch
    tau = tau32(tau)
    P, N, D = q.shape

    def hat(x):
        return x / x.norm(dim=-1, keepdim=True).clamp_min(eps) if normalize else x

    def one_dir(a, a_lab, a_on, c, c_lab, c_on):
        total, n = 0.0, 0
        s = a @ c.T
        for i_a in range(a.shape[0]):
            if not a_on[i_a]:
                continue
            cols = [j for j in range(c.shape[0]) if c_on[j]]
            pos = [j for j in cols if c_lab[j] == a_lab[i_a]]
            if not pos or len(pos) == len(cols):
                continue
            ap = 0.0
            for i in pos:
                R = 1.0 + sum(torch.sigmoid((s[i_a, j] - s[i_a, i]) / tau) for j in cols if j != i)
                Rp = 1.0 + sum(torch.sigmoid((s[i_a, j] - s[i_a, i]) / tau) for j in pos if j != i)
                ap = ap + Rp / R
            total, n = total + (1.0 - ap / len(pos)), n + 1
        return total / n if n else 0.0

    qh, gh = hat(q), hat(g)
    qv = np.ones((P, N), bool) if q_valid is None else np.asarray(q_valid).reshape(P, N) != 0
    gv = np.ones(g.shape[0], bool) if g_valid is None else np.asarray(g_valid) != 0
    losses = []
    for p in range(P):
        if ring is None:
            L0 = one_dir(qh[p], q_lab, qv[p], gh, g_lab, gv)
            L1 = one_dir(gh, g_lab, gv, qh[p], q_lab, qv[p])
        else:
            rows, rl, rv = ring
            rows = torch.as_tensor(np.asarray(rows, np.float64))
            L0 = one_dir(qh[p], q_lab, qv[p], rows[0], rl, np.asarray(rv)[0] != 0)
            L1 = one_dir(gh, g_lab, gv, rows[p + 1], rl, np.asarray(rv)[p + 1] != 0)
        losses.append(torch.zeros((), dtype=torch.float64) + 0.5 * (L0 + L1))
    return torch.stack(losses)


class Ring:
    """The cross-batch memory as reid_xbm_enqueue files it, in fp64: rows [sides, M, D], labels [M], valid [sides, M], the cursor."""

    def __init__(self, capacity, sides, D):
        self.M, self.rows = capacity, np.zeros((sides, capacity, D))
        self.labels, self.valid = np.zeros(capacity, np.int64), np.zeros((sides, capacity), np.uint8)
        self.cursor, self.written = 0, 0

    def enqueue(self, q, g, labels, q_valid=None, g_valid=None, normalize=True):
        P, N, D = q.shape
        slots = (self.cursor + np.arange(N)) % self.M
        sides = [np.asarray(g, np.float64)] + [np.asarray(q[p], np.float64) for p in range(P)]
        valids = [g_valid] + [None if q_valid is None else np.asarray(q_valid).reshape(P, N)[p] for p in range(P)]
        for s, (x, v) in enumerate(zip(sides, valids)):
            self.rows[s, slots] = unit_rows(x, normalize)[0]
            self.valid[s, slots] = 1 if v is None else (np.asarray(v) != 0)
        self.labels[slots] = labels
        self.cursor, self.written = (self.cursor + N) % self.M, self.written + N


def exact_ap(s, pos, valid):
    """The AP of the stable descending ranking of the valid scores s [G] with positives pos: the evaluator's AP with K >= G."""
    idx = np.flatnonzero(valid)
    order = idx[np.argsort(-s[idx], kind='stable')]
    hits = pos[order]
    ranks = np.flatnonzero(hits) + 1
    return float((np.arange(1, ranks.size + 1) / ranks).mean())


def make_case(P, N, Mg, D, ids, seed, invalid=0.0, dtype=np.float32):
    """Random directions: q [P, N, D], g [Mg, D] standard normal rows scaled by random norms in [0.5, 2], labels in [0, ids), optional
    invalid rows (a share ``invalid`` of each side)."""
    r = np.random.default_rng(seed)
    q = r.standard_normal((P, N, D)) * r.uniform(0.5, 2.0, (P, N, 1))
    g = r.standard_normal((Mg, D)) * r.uniform(0.5, 2.0, (Mg, 1))
    q_lab, g_lab = r.integers(0, ids, N), r.integers(0, ids, Mg)
    qv = gv = None
    if invalid > 0:
        qv, gv = (r.random((P, N)) >= invalid).astype(np.uint8), (r.random(Mg) >= invalid).astype(np.uint8)
    return q.astype(dtype), g.astype(dtype), q_lab.astype(np.int64), g_lab.astype(np.int64), qv, gv
