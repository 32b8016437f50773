"""fp64 reference of the cross-modal batch-hard triplet loss (include/reid_hip.h, reid_cross_triplet_*), written plainly in torch and
sharing no code with the package.

    q [P, N, D] = P query sides, g [Mg, D] = the vis side, q_label [N] shared by the pairs, g_label [Mg]; q_valid [P, N], g_valid [Mg].
    unit rows (normalize): x / max(|x|, eps);  d2(a, b) = sum_c (a_c - b_c)^2,  d = sqrt(max(d2, 1e-12)); where d2 <= 1e-12 that term
    has no gradient.
    per pair p, q->g: every valid q row is an anchor against the valid g rows; g->q: every valid g row against the valid q rows of pair
    p (indices pair-local).  hardest positive: same label, largest d2; hardest negative: other label, smallest d2; ties -> lowest
    index; NO self-exclusion.  active anchor: valid, has a positive and a negative; indices -1 and distances / row loss 0 otherwise.
    row loss: max(0, d_ap - d_an + margin) (margin >= 0) or softplus(d_ap - d_an) (margin None);
    L_p = 0.5 (sum_q / max(1, n_qg) + sum_g / max(1, n_gq)), flag_p = [n_qg + n_gq > 0].
"""
import functools
import math

import torch

CLAMP = 1e-12
EPS = 1e-12
U = 2.0 ** -24


def unit_rows(x, normalize, eps=EPS):
    """(rows used for the distances, |x|) in fp64."""
    x = x.double()
    n = (x * x).sum(-1).sqrt()
    return (x / n.clamp(min=eps)[..., None] if normalize else x), n


def pairwise_d2(a, b):
    """[nA, nB] fp64 squared distances in the difference form."""
    a, b = a.double(), b.double()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float64, device=a.device)
    chunk = max(1, (1 << 24) // max(1, b.shape[0] * b.shape[1]))
    for s in range(0, a.shape[0], chunk):
        d = a[s:s + chunk, None, :] - b[None, :, :]
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


def dist_bound(D, d, normalize):
    """The fp32 kernels' allowance on a distance d (the issue's bounds, u = 2^-24)."""
    return (D + 6) * U + 0.5 * D * U * d if normalize else 0.5 * D * U * d


def _first_best(vals):
    """(best value, LOWEST index holding it, runner-up value) per row of ``vals`` (larger is better, -inf = no candidate)."""
    n = vals.shape[1]
    top = torch.topk(vals, min(2, n), dim=1).values
    best = top[:, 0]
    second = top[:, 1] if n > 1 else torch.full_like(best, -math.inf)
    ar = torch.arange(n, device=vals.device).expand_as(vals)
    idx = torch.where(vals == best[:, None], ar, torch.full_like(ar, n)).min(dim=1).values
    return best, idx, second


def mine_direction(d2, a_label, c_label, a_valid, c_valid):
    """idx_p, idx_n (int64, -1 = inactive) of the anchors (rows of d2) among the candidates (columns), and the fp64 gap in DISTANCE
    between the best and the runner-up candidate of each kind (inf when there is no runner-up)."""
    same = a_label[:, None] == c_label[None, :]
    ninf = torch.full_like(d2, -math.inf)
    bp, ip, sp = _first_best(torch.where(same & c_valid[None, :], d2, ninf))
    bn, inn, sn = _first_best(torch.where(~same & c_valid[None, :], -d2, ninf))
    active = a_valid & torch.isfinite(bp) & torch.isfinite(bn)
    dist = lambda v: v.clamp(min=CLAMP).sqrt()
    inf = torch.full_like(bp, math.inf)
    gap_p = torch.where(torch.isfinite(sp), dist(bp) - dist(sp.clamp(min=0)), inf)
    gap_n = torch.where(torch.isfinite(sn), dist((-sn).clamp(min=0)) - dist(-bn), inf)
    minus = torch.full_like(ip, -1)
    return torch.where(active, ip, minus), torch.where(active, inn, minus), gap_p, gap_n


def _valid(v, shape, device):
    return torch.ones(shape, dtype=torch.bool, device=device) if v is None else v.to(device).reshape(shape) != 0


def mine(q, g, q_label, g_label, q_valid=None, g_valid=None, normalize=True, eps=EPS):
    """The selection of every pair and direction: dict of q_idx_p / q_idx_n / q_gap_p / q_gap_n [P, N], g_* [P, Mg]."""
    P, N, _ = q.shape
    dev = q.device
    qh, _ = unit_rows(q, normalize, eps); gh, _ = unit_rows(g, normalize, eps)
    qv, gv = _valid(q_valid, (P, N), dev), _valid(g_valid, (g.shape[0],), dev)
    ql, gl = q_label.to(dev), g_label.to(dev)
    out = {k: [] for k in ('q_idx_p', 'q_idx_n', 'q_gap_p', 'q_gap_n', 'g_idx_p', 'g_idx_n', 'g_gap_p', 'g_gap_n')}
    for p in range(P):
        d2 = pairwise_d2(qh[p], gh)
        for side, vals in (('q', mine_direction(d2, ql, gl, qv[p], gv)), ('g', mine_direction(d2.t().contiguous(), gl, ql, gv, qv[p]))):
            for k, v in zip(('idx_p', 'idx_n', 'gap_p', 'gap_n'), vals):
                out[f'{side}_{k}'].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def evaluate(q, g, sel, margin, normalize=True, eps=EPS):
    """Distances, row losses, L [P], flag [P], n_qg / n_gq [P] (all fp64) for a GIVEN selection ``sel`` (q_idx_p, q_idx_n [P, N] rows
    of g; g_idx_p, g_idx_n [P, Mg] rows of pair p's q side)."""
    P = q.shape[0]
    qh, _ = unit_rows(q, normalize, eps); gh, _ = unit_rows(g, normalize, eps)
    out = {k: [] for k in ('q_d_ap', 'q_d_an', 'q_row_loss', 'q_d2p', 'q_d2n', 'g_d_ap', 'g_d_an', 'g_row_loss', 'g_d2p', 'g_d2n')}
    L, n_qg, n_gq = [], [], []
    for p in range(P):
        sums = []
        for side, A, C in (('q', qh[p], gh), ('g', gh, qh[p])):
            ip, inn = sel[f'{side}_idx_p'][p].long().to(A.device), sel[f'{side}_idx_n'][p].long().to(A.device)
            act = ip >= 0
            a = torch.nonzero(act).flatten()
            z = torch.zeros(A.shape[0], dtype=torch.float64, device=A.device)
            d2p, d2n, d_ap, d_an, rl = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
            d2p[a] = ((A[a] - C[ip[a]]) ** 2).sum(-1); d2n[a] = ((A[a] - C[inn[a]]) ** 2).sum(-1)
            d_ap[a] = d2p[a].clamp(min=CLAMP).sqrt(); d_an[a] = d2n[a].clamp(min=CLAMP).sqrt()
            rl[a] = row_loss_fn(d_ap[a] - d_an[a], margin)
            n = int(act.sum())
            sums.append(float(rl.sum()) / max(1, n))
            (n_qg if side == 'q' else n_gq).append(n)
            for k, v in (('d_ap', d_ap), ('d_an', d_an), ('row_loss', rl), ('d2p', d2p), ('d2n', d2n)):
                out[f'{side}_{k}'].append(v)
        L.append(0.5 * (sums[0] + sums[1]) if n_qg[-1] + n_gq[-1] > 0 else 0.0)
    res = {k: torch.stack(v) for k, v in out.items()}
    res.update(L=L, flag=[1.0 if a + b > 0 else 0.0 for a, b in zip(n_qg, n_gq)], n_qg=n_qg, n_gq=n_gq)
    return res


def reference(q, g, q_label, g_label, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    sel = mine(q, g, q_label, g_label, q_valid, g_valid, normalize, eps)
    out = evaluate(q, g, sel, margin, normalize, eps)
    out.update(sel)
    return out


def gradient(q, g, margin, normalize, sel, gscale=None, eps=EPS):
    """(dq [P, N, D], dg [Mg, D]) fp64 of sum_p gscale[p] L_p for a GIVEN selection: the analytic formula of the header, through the
    normalisation (dx = (G - x^ (x^ . G)) / |x| where |x| >= eps, G / eps below)."""
    P = q.shape[0]
    e = evaluate(q, g, sel, margin, normalize, eps)
    qh, qn = unit_rows(q, normalize, eps); gh, gn = unit_rows(g, normalize, eps)
    gs = [1.0] * P if gscale is None else [float(v) for v in gscale]
    Gq, Gg = torch.zeros_like(qh), torch.zeros_like(gh)
    for p in range(P):
        for side, A, C, GA, GC, n in (('q', qh[p], gh, Gq[p], Gg, e['n_qg'][p]), ('g', gh, qh[p], Gg, Gq[p], e['n_gq'][p])):
            ip, inn = sel[f'{side}_idx_p'][p].long().to(A.device), sel[f'{side}_idx_n'][p].long().to(A.device)
            a = torch.nonzero(ip >= 0).flatten()
            jp, jn = ip[a], inn[a]
            dp, dn = e[f'{side}_d_ap'][p][a], e[f'{side}_d_an'][p][a]
            c = gs[p] * 0.5 * row_dloss_fn(dp - dn, margin) / max(1, n)
            sp = torch.where(e[f'{side}_d2p'][p][a] > CLAMP, c / dp, torch.zeros_like(c))
            sn = torch.where(e[f'{side}_d2n'][p][a] > CLAMP, c / dn, torch.zeros_like(c))
            tp = sp[:, None] * (A[a] - C[jp]); tn = sn[:, None] * (A[a] - C[jn])
            GA.index_add_(0, a, tp - tn)
            GC.index_add_(0, jp, -tp)
            GC.index_add_(0, jn, tn)
    if not normalize:
        return Gq, Gg

    def project(G, xh, n):
        proj = (G - xh * (xh * G).sum(-1, keepdim=True)) / n.clamp(min=eps)[..., None]
        return torch.where((n >= eps)[..., None], proj, G / eps)
    return project(Gq, qh, qn), project(Gg, gh, gn)


def torch_loss(q, g, q_label, g_label, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    """L [P] of the same definition written with whole-tensor torch ops (normalise, pairwise distances, masked max / min), for autograd.
    (Its max / min take the first extreme of a row, which is the tie rule; its clamp passes no gradient below 1e-12.)"""
    P, N, _ = q.shape
    dev = q.device
    qv, gv = _valid(q_valid, (P, N), dev), _valid(g_valid, (g.shape[0],), dev)
    if normalize:
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(eps)
        g = g / g.norm(dim=-1, keepdim=True).clamp_min(eps)
    same = q_label[:, None] == g_label[None, :]
    out = []
    for p in range(P):
        d = ((q[p][:, None, :] - g[None, :, :]) ** 2).sum(-1).clamp_min(CLAMP).sqrt()
        ok = qv[p][:, None] & gv[None, :]
        terms = []
        for dd, pos, av in ((d, same & ok, qv[p]), (d.t(), (same & ok).t(), gv)):
            neg = (~same & ok) if dd is d else (~same & ok).t()
            act = av & pos.any(1) & neg.any(1)
            d_ap = torch.where(pos, dd, torch.full_like(dd, -math.inf)).max(1).values
            d_an = torch.where(neg, dd, torch.full_like(dd, math.inf)).min(1).values
            z = torch.where(act, d_ap - d_an, torch.zeros_like(d_ap))
            rl = torch.where(act, row_loss_fn(z, margin), torch.zeros_like(z))
            terms.append(rl.sum() / act.sum().clamp_min(1))
        out.append(0.5 * (terms[0] + terms[1]))
    return torch.stack(out)


def torch_loss_at(q, g, sel, margin, normalize=True, eps=EPS):
    """L [P] at a GIVEN selection with differentiable torch ops (for autograd where mining is ill-conditioned: a zero row is at
    distance 1 from every unit row)."""
    if normalize:
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(eps)
        g = g / g.norm(dim=-1, keepdim=True).clamp_min(eps)
    out = []
    for p in range(q.shape[0]):
        terms = []
        for side, A, C in (('q', q[p], g), ('g', g, q[p])):
            ip, inn = sel[f'{side}_idx_p'][p].long(), sel[f'{side}_idx_n'][p].long()
            a = torch.nonzero(ip >= 0).flatten()
            d_ap = ((A[a] - C[ip[a]]) ** 2).sum(-1).clamp_min(CLAMP).sqrt()
            d_an = ((A[a] - C[inn[a]]) ** 2).sum(-1).clamp_min(CLAMP).sqrt()
            terms.append(row_loss_fn(d_ap - d_an, margin).sum() / max(1, a.numel()))
        out.append(0.5 * (terms[0] + terms[1]))
    return torch.stack(out)


def loop_reference(q, g, q_label, g_label, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    """The same definition with plain Python loops over lists (small inputs only)."""
    def rows(x):
        X = [[float(v) for v in r] for r in x.double().tolist()]
        if not normalize:
            return X
        return [[v / max(math.sqrt(sum(c * c for c in r)), eps) for v in r] for r in X]

    P, N, Mg = q.shape[0], q.shape[1], g.shape[0]
    G = rows(g)
    QL, GL = [int(v) for v in q_label.tolist()], [int(v) for v in g_label.tolist()]
    QV = [[True] * N for _ in range(P)] if q_valid is None else [[bool(v) for v in r] for r in q_valid.reshape(P, N).tolist()]
    GV = [True] * Mg if g_valid is None else [bool(v) for v in g_valid.tolist()]

    def direction(A, AL, AV, C, CL, CV):
        n = len(A)
        idx_p, idx_n, d_ap, d_an, rl = [-1] * n, [-1] * n, [0.0] * n, [0.0] * n, [0.0] * n
        for i in range(n):
            if not AV[i]:
                continue
            bp, jp, bn, jn = -1.0, -1, math.inf, -1
            for j in range(len(C)):
                if not CV[j]:
                    continue
                d2 = sum((a - b) ** 2 for a, b in zip(A[i], C[j]))
                if CL[j] == AL[i]:
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
                           'L', 'flag', 'n_qg', 'n_gq')}
    for p in range(P):
        Q = rows(q[p])
        sums, counts = [], []
        for side, vals in (('q', direction(Q, QL, QV[p], G, GL, GV)), ('g', direction(G, GL, GV, Q, QL, QV[p]))):
            for k, v in zip(('idx_p', 'idx_n', 'd_ap', 'd_an', 'row_loss'), vals):
                out[f'{side}_{k}'].append(v)
            n = sum(1 for j in vals[0] if j >= 0)
            counts.append(n); sums.append(sum(vals[4]) / max(1, n))
        out['n_qg'].append(counts[0]); out['n_gq'].append(counts[1])
        out['flag'].append(1.0 if sum(counts) > 0 else 0.0)
        out['L'].append(0.5 * (sums[0] + sums[1]) if sum(counts) > 0 else 0.0)
    return out


K_ROWS = 4                               # rows per identity and side in make_case


def small_gaps(ref, D, normalize, factor):
    """Per side, the active anchors whose fp64 gap between the best and the runner-up distance is within ``factor`` x the distance
    bound: [(side, kind, mask [P, n])]."""
    out = []
    for s in 'qg':
        act = ref[f'{s}_idx_p'] >= 0
        for kind, d in (('p', ref[f'{s}_d_ap']), ('n', ref[f'{s}_d_an'])):
            out.append((s, kind, act & (ref[f'{s}_gap_{kind}'] <= factor * dist_bound(D, d, normalize))))
    return out


def make_case(P, N, Mg, D, ratio, seed, device='cpu', clear_gaps=False):
    """The generator of the issue: rows = common mean x ratio + identity offset x 0.7 + modality offset x 0.5 + N(0, 1), as float32;
    identity of row r of either side = r // 4 (sides of different length: the longer one's last identities have no positive).
    The common mean has |m_c| in [0.5, 1.5) with a random sign.  Returns q [P, N, D], g [Mg, D], q_label [N], g_label [Mg].
    ``clear_gaps``: a row that is some anchor's best candidate by less than 11 x the distance bound (normalised or not) is moved by
    0.002 of its length towards that anchor (a negative) or away from it (a positive) until no such anchor is left -- the fixtures on
    which fp32 mining must reproduce the fp64 indices.  Always generated on
    the CPU (the same bits everywhere), then moved."""
    gen = torch.Generator().manual_seed(seed)
    m = (0.5 + torch.rand(D, generator=gen, dtype=torch.float64)) * (torch.randint(0, 2, (D,), generator=gen).double() * 2 - 1)
    ql, gl = torch.arange(N) // K_ROWS, torch.arange(Mg) // K_ROWS
    off = torch.randn(max(N, Mg) // K_ROWS + 1, D, generator=gen, dtype=torch.float64)
    mod = torch.randn(P + 1, D, generator=gen, dtype=torch.float64)
    q = (m * ratio + 0.7 * off[ql][None] + 0.5 * mod[:P, None, :] + torch.randn(P, N, D, generator=gen, dtype=torch.float64)).float()
    g = (m * ratio + 0.7 * off[gl] + 0.5 * mod[P] + torch.randn(Mg, D, generator=gen, dtype=torch.float64)).float()
    for _ in range(100 if clear_gaps else 0):
        moves = []                                         # (side of the moved row, pair, row, step towards (+) / away from (-) the anchor)
        for normalize in (True, False):
            ref = reference(q, g, ql, gl, None, None, 0.3, normalize)
            for s, kind, mask in small_gaps(ref, D, normalize, 11.0):
                for p, a in torch.nonzero(mask).tolist():
                    j = int(ref[f'{s}_idx_{kind}'][p][a])
                    anchor = q[p, a] if s == 'q' else g[a]
                    moves.append(('g' if s == 'q' else 'q', p, j, anchor.double(), 1.0 if kind == 'n' else -1.0))
        if not moves:
            break
        for side, p, j, anchor, sign in moves:
            row = (g[j] if side == 'g' else q[p, j]).double()
            v = anchor - row
            row = (row + sign * 0.002 * row.norm() * v / v.norm()).float()
            if side == 'g':
                g[j] = row
            else:
                q[p, j] = row
    else:
        assert not clear_gaps, 'make_case: the gaps did not clear'
    return q.to(device), g.to(device), ql.to(device), gl.to(device)


# (P, N, Mg, D, pad) of the GPU test, and which generated fixtures it checks for INDEX EQUALITY (test_cross_triplet_cpu.py clears them:
# every anchor's fp64 gap between the best and the runner-up distance exceeds 10 x the distance bound)
SHAPES = [(1, 1, 1, 4, 0), (2, 8, 8, 512, 0), (3, 15, 11, 96, 8), (4, 64, 64, 512, 0), (2, 260, 300, 256, 0), (1, 6, 6, 1024, 0),
          (4, 1024, 1024, 512, 0)]
EXACT_INDEX = [(s, 0.0) for s in SHAPES[:4]]


def case_seed(P, N, Mg, D, ratio):
    return 1000 * P + 7 * N + 3 * Mg + D + int(ratio)


@functools.lru_cache(maxsize=None)
def _fixture_cpu(shape, ratio):
    P, N, Mg, D, _ = shape
    return make_case(P, N, Mg, D, ratio, case_seed(P, N, Mg, D, ratio), clear_gaps=(shape, ratio) in EXACT_INDEX)


def fixture(shape, ratio, device='cpu'):
    """The generated case of a GPU-test shape (made once per process): gaps cleared where the indices are compared exactly."""
    return tuple(t.clone().to(device) for t in _fixture_cpu(shape, ratio))
