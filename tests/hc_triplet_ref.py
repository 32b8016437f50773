"""fp64 reference of the hetero-center triplet loss (include/reid_hip.h, reid_hc_triplet_*), written plainly in
torch and sharing no code with the package.

    q [P, N, D] = P query sides, g [Mg, D] = the vis side, q_label [N] shared by the pairs, g_label [Mg]; q_valid [P, N], g_valid [Mg].
    unit rows (normalize): x / max(|x|, eps).
    centres of a side: leader(i) = the lowest valid row with row i's label; the leaders in ascending order are the slots 0 .. S-1;
    centre = mean of the members' (unit) rows.  lead [n] = slot of a row (-1: invalid), count / label [n] per slot (0 behind S).
    per pair p the union U_p = [q centres of pair p | g centres] in the index space 0 .. N+Mg-1 (q centre s -> s, g centre t -> N + t):
    every centre is an anchor; positive = the centre of the other side with its label; negative = the centre of another label with the
    smallest d2 from either side, ties -> lowest index; d = sqrt(max(d2, 1e-12)), no gradient where d2 <= 1e-12.
    active anchor: has both; indices -1 and distances / loss 0 otherwise.
    l = max(0, d_ap - d_an + margin) (margin >= 0) or softplus(d_ap - d_an) (margin None);
    L_p = sum_active l / max(1, n_q + n_g), flag_p = [n_q + n_g > 0].
"""
import functools
import math

import torch

CLAMP = 1e-12
EPS = 1e-12
U = 2.0 ** -24


def unit_rows(x, normalize, eps=EPS):
    """(rows used for the centres, |x|) in fp64."""
    x = x.double()
    n = (x * x).sum(-1).sqrt()
    return (x / n.clamp(min=eps)[..., None] if normalize else x), n


def row_loss_fn(z, margin):
    if margin is None:
        return z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    return (z + margin).clamp(min=0)


def _valid(v, shape, device):
    return torch.ones(shape, dtype=torch.bool, device=device) if v is None else v.to(device).reshape(shape) != 0


def leaders(labels, valid):
    """lead [n] (slot of a row, -1 = invalid), count [n] and label [n] per slot (0 behind S), S."""
    n = labels.shape[0]
    ar = torch.arange(n, device=labels.device)
    same = (labels[:, None] == labels[None, :]) & valid[None, :]
    first = torch.where(same, ar[None, :].expand(n, n), torch.full((n, n), n, device=labels.device)).min(dim=1).values      # lowest valid row with my label
    is_leader = valid & (first == ar)
    slot_of_row = torch.cumsum(is_leader.long(), 0) - 1
    lead = torch.where(valid, slot_of_row[first.clamp(max=n - 1)], torch.full_like(ar, -1))
    S = int(is_leader.sum())
    count = torch.zeros(n, dtype=torch.int64, device=labels.device)
    count.index_add_(0, lead[valid], torch.ones(int(valid.sum()), dtype=torch.int64, device=labels.device))
    clabel = torch.zeros(n, dtype=torch.int64, device=labels.device)
    clabel[:S] = labels[is_leader]
    return lead, count, clabel, S


def side_centres(xh, lead, count, S):
    """[S, D] means of the rows xh [n, D] by slot (differentiable in xh)."""
    ok = lead >= 0
    c = torch.zeros(S, xh.shape[1], dtype=xh.dtype, device=xh.device).index_add(0, lead[ok], xh[ok])
    return c / count[:S, None].to(xh.dtype)


def dist_bound(D, d, normalize, cmax, rowmax=None):
    """The fp32 kernels' allowance on a centre distance d (u = 2^-24).  A centre of c members is within
    (D / 2 + 3) u (its unit rows, section 14) + (c + 1) / 2 u (c - 1 additions whose partial sums have norm <= 2 .. c, over c) + u (the
    division) of the fp64 centre in norm, relative to the rows' norm (1 for unit rows, ``rowmax`` = the largest row norm otherwise, where
    the rows carry no error of their own); two centres move d by the sum of both, the difference-form sum adds D u / 2 relative."""
    if normalize:
        return (D + 9 + cmax) * U + 0.5 * D * U * d
    return (3 + cmax) * U * rowmax + 0.5 * D * U * d


def centre_bound(D, normalize, c, rowmax=None):
    """The allowance on |fp32 centre - fp64 centre| (vector norm) of a centre of c members: one half of dist_bound's absolute term."""
    return (0.5 * D + 4 + 0.5 * (c + 1)) * U if normalize else (1 + 0.5 * (c + 1)) * U * rowmax


def prepare(q, g, q_label, g_label, q_valid=None, g_valid=None, normalize=True, eps=EPS):
    """Leaders and fp64 centres of every side: dict with q_lead / q_count / q_label [P, N], g_* [Mg], S_q [P], S_g, cq (list of
    [S_q[p], D]), cg [S_g, D], cmax (the largest member count) and rowmax (the largest norm of a valid row)."""
    P, N, _ = q.shape
    dev = q.device
    qh, qn = unit_rows(q, normalize, eps); gh, gn = unit_rows(g, normalize, eps)
    qv, gv = _valid(q_valid, (P, N), dev), _valid(g_valid, (g.shape[0],), dev)
    ql, gl = q_label.to(dev), g_label.to(dev)
    out = dict(q_lead=[], q_count=[], q_label=[], S_q=[], cq=[])
    for p in range(P):
        lead, count, clabel, S = leaders(ql, qv[p])
        out['q_lead'].append(lead); out['q_count'].append(count); out['q_label'].append(clabel); out['S_q'].append(S)
        out['cq'].append(side_centres(qh[p], lead, count, S))
    for k in ('q_lead', 'q_count', 'q_label'):
        out[k] = torch.stack(out[k])
    out['g_lead'], out['g_count'], out['g_label'], out['S_g'] = leaders(gl, gv)
    out['cg'] = side_centres(gh, out['g_lead'], out['g_count'], out['S_g'])
    out['cmax'] = int(max(int(out['q_count'].max()), int(out['g_count'].max())))
    norms = torch.cat([qn[qv], gn[gv]])
    out['rowmax'] = float(norms.max()) if norms.numel() else 0.0
    return out


def _union(prep, p, N):
    """(centres [S, D], labels [S], index-space index [S], is_q [S]) of U_p."""
    Sq, Sg = prep['S_q'][p], prep['S_g']
    dev = prep['cg'].device
    c = torch.cat([prep['cq'][p], prep['cg']])
    lab = torch.cat([prep['q_label'][p][:Sq], prep['g_label'][:Sg]])
    index = torch.cat([torch.arange(Sq, device=dev), N + torch.arange(Sg, device=dev)])
    is_q = torch.cat([torch.ones(Sq, dtype=torch.bool, device=dev), torch.zeros(Sg, dtype=torch.bool, device=dev)])
    return c, lab, index, is_q


def mine(q, g, q_label, g_label, q_valid=None, g_valid=None, normalize=True, eps=EPS, prep=None):
    """The selection of every pair in the index space: idx_p, idx_n [P, N + Mg] (int64, -1 = unused slot or inactive anchor) and gap_n
    [P, N + Mg], the fp64 gap in DISTANCE between the nearest and the second-nearest negative (inf without a runner-up)."""
    P, N, _ = q.shape
    Mg = g.shape[0]
    prep = prep or prepare(q, g, q_label, g_label, q_valid, g_valid, normalize, eps)
    dev = q.device
    idx_p = torch.full((P, N + Mg), -1, dtype=torch.int64, device=dev)
    idx_n = idx_p.clone()
    gap_n = torch.full((P, N + Mg), math.inf, dtype=torch.float64, device=dev)
    for p in range(P):
        c, lab, index, is_q = _union(prep, p, N)
        S = c.shape[0]
        if S == 0:
            continue
        d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1) if S * S * c.shape[1] <= (1 << 24) else \
            torch.stack([((c[i][None, :] - c) ** 2).sum(-1) for i in range(S)])
        same = lab[:, None] == lab[None, :]
        pos = same & (is_q[:, None] != is_q[None, :])
        ar = torch.arange(S, device=dev)
        has_p = pos.any(1)
        jp = torch.where(pos, ar[None, :].expand(S, S), torch.full((S, S), S, device=dev)).min(1).values
        neg = torch.where(~same, d2, torch.full_like(d2, math.inf))
        top = torch.topk(neg, min(2, S), dim=1, largest=False).values
        best = top[:, 0]
        second = top[:, 1] if S > 1 else torch.full_like(best, math.inf)
        has_n = torch.isfinite(best)
        jn = torch.where(neg == best[:, None], ar[None, :].expand(S, S), torch.full((S, S), S, device=dev)).min(1).values      # lowest index
        act = has_p & has_n
        dist = lambda v: v.clamp(min=CLAMP).sqrt()
        gap = torch.where(torch.isfinite(second), dist(second) - dist(best), torch.full_like(best, math.inf))
        a = torch.nonzero(act).flatten()
        idx_p[p, index[a]] = index[jp[a]]
        idx_n[p, index[a]] = index[jn[a]]
        gap_n[p, index[a]] = gap[a]
    return dict(idx_p=idx_p, idx_n=idx_n, gap_n=gap_n)


def loss_at(q, g, sel, margin, normalize, q_label, g_label, q_valid=None, g_valid=None, eps=EPS, detail=False):
    """L [P] (fp64, differentiable in q and g) at a GIVEN selection ``sel`` (idx_p, idx_n [P, N + Mg] in the index space): normalise,
    centres by index_add, distances, clamp (no gradient below 1e-12), row loss, mean over the active anchors.  ``detail``: also the
    per-anchor d_ap, d_an, loss [P, N + Mg] and n_q, n_g."""
    P, N, D = q.shape
    Mg = g.shape[0]
    dev = q.device
    q, g = q.double(), g.double()
    qv, gv = _valid(q_valid, (P, N), dev), _valid(g_valid, (Mg,), dev)
    if normalize:
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(eps)
        g = g / g.norm(dim=-1, keepdim=True).clamp_min(eps)
    glead, gcount, _, Sg = leaders(g_label.to(dev), gv)
    cg = side_centres(g, glead, gcount, Sg)
    Ls, det = [], dict(d_ap=[], d_an=[], loss=[], n_q=[], n_g=[])
    for p in range(P):
        lead, count, _, Sq = leaders(q_label.to(dev), qv[p])
        cq = side_centres(q[p], lead, count, Sq)
        full = torch.zeros(N + Mg, D, dtype=torch.float64, device=dev)
        full = torch.cat([cq, full[Sq:N], cg, full[N + Sg:]])                                   # centres at their index-space positions
        ip, inn = sel['idx_p'][p].long().to(dev), sel['idx_n'][p].long().to(dev)
        a = torch.nonzero(ip >= 0).flatten()
        d_ap = ((full[a] - full[ip[a]]) ** 2).sum(-1).clamp_min(CLAMP).sqrt()
        d_an = ((full[a] - full[inn[a]]) ** 2).sum(-1).clamp_min(CLAMP).sqrt()
        rl = row_loss_fn(d_ap - d_an, margin)
        Ls.append(rl.sum() / max(1, a.numel()))
        if detail:
            z = torch.zeros(N + Mg, dtype=torch.float64, device=dev)
            for k, v in (('d_ap', d_ap), ('d_an', d_an), ('loss', rl)):
                t = z.clone(); t[a] = v.detach(); det[k].append(t)
            det['n_q'].append(int((a < N).sum())); det['n_g'].append(int((a >= N).sum()))
    L = torch.stack(Ls)
    if not detail:
        return L
    out = {k: torch.stack(det[k]) for k in ('d_ap', 'd_an', 'loss')}
    out.update(n_q=det['n_q'], n_g=det['n_g'], L=[float(v) for v in L.detach()],
               flag=[1.0 if a + b > 0 else 0.0 for a, b in zip(det['n_q'], det['n_g'])])
    return out


def evaluate(q, g, sel, margin, normalize, q_label, g_label, q_valid=None, g_valid=None, eps=EPS):
    """d_ap, d_an, loss [P, N + Mg], L, flag, n_q, n_g (fp64) for a GIVEN selection."""
    with torch.no_grad():
        return loss_at(q, g, sel, margin, normalize, q_label, g_label, q_valid, g_valid, eps, detail=True)


def reference(q, g, q_label, g_label, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    prep = prepare(q, g, q_label, g_label, q_valid, g_valid, normalize, eps)
    sel = mine(q, g, q_label, g_label, q_valid, g_valid, normalize, eps, prep=prep)
    out = evaluate(q, g, sel, margin, normalize, q_label, g_label, q_valid, g_valid, eps)
    out.update(sel)
    out.update({k: prep[k] for k in ('q_lead', 'q_count', 'q_label', 'g_lead', 'g_count', 'g_label', 'S_q', 'S_g', 'cmax', 'rowmax')})
    return out


def gradient(q, g, margin, normalize, sel, q_label, g_label, q_valid=None, g_valid=None, gscale=None, eps=EPS):
    """(dq [P, N, D], dg [Mg, D]) fp64 of sum_p gscale[p] L_p at a GIVEN selection, through autograd."""
    P = q.shape[0]
    qa, ga = q.double().clone().requires_grad_(True), g.double().clone().requires_grad_(True)
    L = loss_at(qa, ga, sel, margin, normalize, q_label, g_label, q_valid, g_valid, eps)
    gs = torch.tensor([1.0] * P if gscale is None else [float(v) for v in gscale], dtype=torch.float64, device=q.device)
    total = (L * gs).sum()
    if not total.requires_grad:                                # nothing active in any pair
        return torch.zeros_like(qa), torch.zeros_like(ga)
    dq, dg = torch.autograd.grad(total, (qa, ga), allow_unused=True)
    return (torch.zeros_like(qa) if dq is None else dq), (torch.zeros_like(ga) if dg is None else dg)


def torch_loss(q, g, q_label, g_label, margin=0.3, normalize=True, eps=EPS):
    """L [P] of the same definition written with whole-tensor torch ops in the inputs' dtype (normalise, one-hot centre means, cdist-like
    distances, masked min), every row valid and labels that occur on both sides or not: what tools/bench_hc_triplet.py times against."""
    P, N, _ = q.shape
    if normalize:
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(eps)
        g = g / g.norm(dim=-1, keepdim=True).clamp_min(eps)
    uq, iq = torch.unique(q_label, return_inverse=True)
    ug, ig = torch.unique(g_label, return_inverse=True)
    oq = torch.nn.functional.one_hot(iq, uq.numel()).to(q.dtype); og = torch.nn.functional.one_hot(ig, ug.numel()).to(q.dtype)
    cg = (og.t() @ g) / og.sum(0)[:, None]
    out = []
    for p in range(P):
        cq = (oq.t() @ q[p]) / oq.sum(0)[:, None]
        c = torch.cat([cq, cg]); lab = torch.cat([uq, ug])
        side = torch.cat([torch.zeros_like(uq), torch.ones_like(ug)])
        d = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1).clamp_min(CLAMP).sqrt()
        same = lab[:, None] == lab[None, :]
        pos = same & (side[:, None] != side[None, :])
        act = pos.any(1) & (~same).any(1)
        d_ap = torch.where(pos, d, torch.zeros_like(d)).sum(1)                                   # at most one positive
        d_an = torch.where(~same, d, torch.full_like(d, math.inf)).min(1).values
        z = torch.where(act, d_ap - d_an, torch.zeros_like(d_ap))
        rl = torch.where(act, row_loss_fn(z, margin), torch.zeros_like(z))
        out.append(rl.sum() / act.sum().clamp_min(1))
    return torch.stack(out)


def loop_reference(q, g, q_label, g_label, q_valid=None, g_valid=None, margin=0.3, normalize=True, eps=EPS):
    """The same definition with plain Python loops over lists (small inputs only)."""
    def rows(x):
        X = [[float(v) for v in r] for r in x.double().tolist()]
        if not normalize:
            return X
        return [[v / max(math.sqrt(sum(c * c for c in r)), eps) for v in r] for r in X]

    P, N, Mg = q.shape[0], q.shape[1], g.shape[0]
    QL, GL = [int(v) for v in q_label.tolist()], [int(v) for v in g_label.tolist()]
    QV = [[True] * N for _ in range(P)] if q_valid is None else [[bool(v) for v in r] for r in q_valid.reshape(P, N).tolist()]
    GV = [True] * Mg if g_valid is None else [bool(v) for v in g_valid.tolist()]

    def side(X, labs, val):
        n = len(X)
        lead, slots = [-1] * n, []                             # slots: [label, [member rows]]
        for i in range(n):
            if not val[i]:
                continue
            for s, (lab, members) in enumerate(slots):
                if lab == labs[i]:
                    members.append(i); lead[i] = s
                    break
            else:
                slots.append([labs[i], [i]]); lead[i] = len(slots) - 1
        cen = [[sum(X[i][c] for i in members) / len(members) for c in range(len(X[0]))] for _, members in slots]
        count = [len(m) for _, m in slots] + [0] * (n - len(slots))
        label = [lab for lab, _ in slots] + [0] * (n - len(slots))
        return lead, count, label, cen

    out = {k: [] for k in ('q_lead', 'q_count', 'q_label', 'idx_p', 'idx_n', 'd_ap', 'd_an', 'loss', 'L', 'flag', 'n_q', 'n_g')}
    out['g_lead'], out['g_count'], out['g_label'], cg = side(rows(g), GL, GV)
    for p in range(P):
        lead, count, label, cq = side(rows(q[p]), QL, QV[p])
        out['q_lead'].append(lead); out['q_count'].append(count); out['q_label'].append(label)
        cen = cq + cg
        lab = label[:len(cq)] + out['g_label'][:len(cg)]
        index = list(range(len(cq))) + [N + t for t in range(len(cg))]
        n = N + Mg
        idx_p, idx_n, d_ap, d_an, rl = [-1] * n, [-1] * n, [0.0] * n, [0.0] * n, [0.0] * n
        for i in range(len(cen)):
            jp, bn, jn = -1, math.inf, -1
            for j in range(len(cen)):
                d2 = sum((a - b) ** 2 for a, b in zip(cen[i], cen[j]))
                if lab[j] == lab[i]:
                    if (i < len(cq)) != (j < len(cq)):
                        jp, bp = j, d2
                elif d2 < bn:
                    bn, jn = d2, j
            if jp < 0 or jn < 0:
                continue
            u = index[i]
            idx_p[u], idx_n[u] = index[jp], index[jn]
            d_ap[u], d_an[u] = math.sqrt(max(bp, CLAMP)), math.sqrt(max(bn, CLAMP))
            z = d_ap[u] - d_an[u]
            rl[u] = max(0.0, z + margin) if margin is not None else max(z, 0.0) + math.log1p(math.exp(-abs(z)))
        nq, ng = sum(1 for j in idx_p[:N] if j >= 0), sum(1 for j in idx_p[N:] if j >= 0)
        for k, v in (('idx_p', idx_p), ('idx_n', idx_n), ('d_ap', d_ap), ('d_an', d_an), ('loss', rl)):
            out[k].append(v)
        out['n_q'].append(nq); out['n_g'].append(ng)
        out['flag'].append(1.0 if nq + ng > 0 else 0.0)
        out['L'].append(sum(rl) / max(1, nq + ng))
    return out


def make_case(P, N, Mg, D, ratio, seed, K=4, device='cpu'):
    """rows = common mean x ratio + identity offset x 0.7 + modality offset x 0.5 + N(0, 1), as float32 (the generator of
    cross_triplet_ref.make_case); identity of row r of either side = r // K (sides of different length: the longer one's last
    identities have no positive).  The common mean has |m_c| in [0.5, 1.5) with a random sign.  Returns q [P, N, D], g [Mg, D],
    q_label [N], g_label [Mg].  Always generated on the CPU (the same bits everywhere), then moved."""
    gen = torch.Generator().manual_seed(seed)
    m = (0.5 + torch.rand(D, generator=gen, dtype=torch.float64)) * (torch.randint(0, 2, (D,), generator=gen).double() * 2 - 1)
    ql, gl = torch.arange(N) // K, torch.arange(Mg) // K
    off = torch.randn(max(N, Mg) // K + 1, D, generator=gen, dtype=torch.float64)
    mod = torch.randn(P + 1, D, generator=gen, dtype=torch.float64)
    q = (m * ratio + 0.7 * off[ql][None] + 0.5 * mod[:P, None, :] + torch.randn(P, N, D, generator=gen, dtype=torch.float64)).float()
    g = (m * ratio + 0.7 * off[gl] + 0.5 * mod[P] + torch.randn(Mg, D, generator=gen, dtype=torch.float64)).float()
    return q.to(device), g.to(device), ql.to(device), gl.to(device)


def cleared(q, g, ql, gl, factor=2.0):
    """The rule for index equality: for every active anchor, with unit rows and without, the fp64 gap between the nearest and the
    second-nearest negative exceeds ``factor`` x the distance bound (a positive has no competitor: there is at most one).  Returns
    (cleared, the smallest gap / bound)."""
    D = q.shape[-1]
    worst = math.inf
    for normalize in (True, False):
        ref = reference(q, g, ql, gl, None, None, 0.3, normalize)
        act = ref['idx_p'] >= 0
        if bool(act.any()):
            b = dist_bound(D, ref['d_an'], normalize, ref['cmax'], ref['rowmax'])
            worst = min(worst, float((ref['gap_n'] / b)[act].min()))
    return worst > factor, worst


# (P, N, Mg, D, pad) of the GPU test -> rows per identity, and which generated fixtures it checks for INDEX EQUALITY
# (test_hc_triplet_cpu.py asserts that they are cleared)
SHAPES = [(1, 8, 8, 4, 0), (2, 13, 11, 36, 4), (4, 64, 64, 512, 0), (3, 300, 270, 128, 0), (1, 6, 6, 1024, 0), (4, 1024, 1024, 512, 0)]
K_OF = {SHAPES[3]: 1}
EXACT_INDEX = [(s, 0.0) for s in SHAPES[:4]]
# the seed of a fixture; where the default does not clear the rule above, the first seed counted up from it that does
SEEDS = {(SHAPES[2], 0.0): 5156}


def case_seed(shape, ratio):
    P, N, Mg, D, _ = shape
    return SEEDS.get((shape, ratio), 1000 * P + 7 * N + 3 * Mg + D + int(ratio))


@functools.lru_cache(maxsize=None)
def _fixture_cpu(shape, ratio):
    P, N, Mg, D, _ = shape
    return make_case(P, N, Mg, D, ratio, case_seed(shape, ratio), K=K_OF.get(shape, 4))


def fixture(shape, ratio, device='cpu'):
    """The generated case of a GPU-test shape (made once per process)."""
    return tuple(t.clone().to(device) for t in _fixture_cpu(shape, ratio))
