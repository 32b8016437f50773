"""numpy fp64 references of the cutoff metrics (include/reid_hip.h: reid_rank_metrics_at, reid_list_metrics): a walk of the stable
descending argsort of one query's fp32 score row, as loss_refs.rank_metrics_ref does it, and the same quantities from a ranked list.
Shared by tests/test_metrics_at_k_cpu.py, test_metrics_at_k_gpu.py and test_list_metrics_gpu.py."""
import numpy as np

from helpers import SENTINEL32

GUARD = 32                        # guard words on either side of a kernel output
MAX_POS = 8192


def _dropped(n, g_img, excl):
    d = np.zeros(n, bool)
    if g_img is not None and excl is not None:
        ids = [int(e) for e in excl if int(e) >= 0]
        gi = np.asarray(g_img)
        if ids:
            d = (gi >= 0) & np.isin(gi, ids)
    return d


def _from_ranks(ranks, ks):
    """hits [n_cut], sum_at [n_cut] of the ascending 1-based ranks of the positives: terms (r + 1) / rank_r summed in fp64."""
    terms = np.arange(1, len(ranks) + 1, dtype=np.float64) / ranks.astype(np.float64)
    hits = np.array([int((ranks <= K).sum()) for K in ks], dtype=np.int64)
    sum_at = np.array([float(np.sum(terms[ranks <= K])) for K in ks], dtype=np.float64)
    return hits, sum_at


def rows_ref(scores, g_pid, q_pid, ks, g_img=None, excl=None, has_slot=True):
    """dict(hits, sum_at, rank_last, npos, rank1) of one query from its fp32 score row.  Ranking: score descending, gallery index
    ascending on ties; gallery rows whose image id (>= 0) is one of ``excl`` are removed.  No positive: all zero; more than 8192
    positives: npos = -1 and everything else zero (what the kernel writes)."""
    s = np.asarray(scores, dtype=np.float32)
    g_pid = np.asarray(g_pid)
    dropped = _dropped(s.shape[0], g_img, excl)
    pos = (g_pid == q_pid) & ~dropped
    if not has_slot:
        pos[:] = False
    npos = int(pos.sum())
    zero = dict(hits=np.zeros(len(ks), np.int64), sum_at=np.zeros(len(ks)), rank_last=0, npos=0, rank1=0)
    if npos == 0:
        return zero
    if npos > MAX_POS:
        return dict(zero, npos=-1)
    order = np.argsort(-s.astype(np.float64), kind='stable')
    walk = order[~dropped[order]]
    ranks = np.nonzero(pos[walk])[0] + 1
    hits, sum_at = _from_ranks(ranks, ks)
    return dict(hits=hits, sum_at=sum_at, rank_last=int(ranks[-1]), npos=npos, rank1=int(ranks[0]))


def list_ref(idx, g_pid, q_pid, ks, g_img=None, excl=None):
    """dict(hits, sum_at, npos, rank1) of one query from its ranked list ``idx`` (gallery rows, best first; -1 = no entry, trailing):
    an excluded gallery row is skipped and the positions behind it move up; npos counts the unmasked positives of the gallery;
    rank1 = 0 when the list holds no positive."""
    g_pid = np.asarray(g_pid)
    dropped = _dropped(g_pid.shape[0], g_img, excl)
    npos = int(((g_pid == q_pid) & ~dropped).sum())
    lst = np.asarray(idx, dtype=np.int64)
    lst = lst[lst >= 0]
    lst = lst[~dropped[lst]]
    ranks = np.nonzero(g_pid[lst] == q_pid)[0] + 1
    hits, sum_at = _from_ranks(ranks, ks)
    return dict(hits=hits, sum_at=sum_at, npos=npos, rank1=int(ranks[0]) if len(ranks) else 0)


def sum_bound(hits, sum_at):
    """|kernel - reference| allowed for sum_at: (hits + 1) * 2^-52 * sum_at, twice the standard bound gamma_n = n u / (1 - n u),
    u = 2^-53, of a sum of `hits` correctly rounded quotients in any order (each term one division: (1 + d), |d| <= u; a sum of n
    terms adds at most n - 1 more roundings: relative error <= gamma_n of the sum of non-negative terms, for the kernel and for
    the reference alike)."""
    return (np.asarray(hits, dtype=np.float64) + 1.0) * 2.0 ** -52 * np.asarray(sum_at, dtype=np.float64)


def summary_ref(per_query, ks, norm='hits'):
    """mAP@K / R@K / num_queries@K / mINP of a list of rows_ref / list_ref dictionaries (the arithmetic of evaluate.cutoff_summary,
    in numpy fp64)."""
    out = {}
    with_pos = [d for d in per_query if d['npos'] > 0]
    for c, K in enumerate(ks):
        if norm == 'hits':
            aps = [d['sum_at'][c] / d['hits'][c] for d in per_query if d['hits'][c] > 0]
        else:
            aps = [d['sum_at'][c] / min(K, d['npos']) for d in with_pos]
        out[f'mAP@{K}'] = float(np.mean(aps)) if aps else 0.0
        out[f'R@{K}'] = float(np.mean([1 <= d['rank1'] <= K for d in with_pos])) if with_pos else 0.0
        out[f'num_queries@{K}'] = len(aps)
    if with_pos and 'rank_last' in with_pos[0]:
        out['mINP'] = float(np.mean([d['npos'] / d['rank_last'] for d in with_pos]))
    return out


# ---- shared by the GPU tests -------------------------------------------------------------------------------------------------
def guarded(shape, dtype):
    """(sentinel buffer of GUARD + n + GUARD 32-bit words, its middle as a `dtype` tensor of `shape`)."""
    import torch
    words = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
    buf = torch.full((words + 2 * GUARD,), SENTINEL32, dtype=torch.int32, device='cuda')
    return buf, buf[GUARD:GUARD + words].view(dtype).view(*shape)


def check_guarded(bufs):
    import torch
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        words = buf.numel() - 2 * GUARD
        assert bool((buf[:GUARD] == SENTINEL32).all()) and bool((buf[GUARD + words:] == SENTINEL32).all()), f'{name}: guard words overwritten'
        w = buf[GUARD:GUARD + words].view(view.numel(), -1)
        assert not bool((w == SENTINEL32).all(1).any()), f'{name}: elements not written'


def make_case(Nq, Ng, npid, D=512):
    """The recipe of test_metrics_vs_oracle, plus two planted pairs: queries 0 and 4 (no exclusion ids) each find an exact copy of
    themselves in a positive AND in a non-positive gallery row -- ranks 1 and 2 with equal scores, the non-positive first (the lower
    gallery index) for query 0 and the positive first for query 4, so only the tie rule decides hits at K = 1."""
    import torch
    g = torch.Generator().manual_seed(Nq + Ng)
    centers = torch.randn(npid + 3, D, generator=g)
    gp = torch.randint(0, npid, (Ng,), generator=g)
    qp = torch.randint(0, npid + 3, (Nq,), generator=g)
    qp[0] = qp[3] = qp[4] = 0                                          # (query 3: three drawn ids and a positive's = 4 exclusion ids)
    qp[1] = npid + 1; qp[7] = npid + 2                                 # query pids without a gallery row (query 7: 3 exclusion ids)
    G = centers[gp] * 0.6 + torch.randn(Ng, D, generator=g)
    Q = centers[qp] * 0.6 + torch.randn(Nq, D, generator=g)
    dup = torch.randint(0, Ng, (Ng // 10,), generator=g)
    G[dup] = G[(dup * 7 + 3) % Ng]
    if npid > 1:
        pos = (gp == 0).nonzero().flatten().tolist(); neg = (gp != 0).nonzero().flatten().tolist()
        a = next(j for j in pos if j > neg[0])
        p2 = next(j for j in pos if j != a); b = next(j for j in neg[1:] if j > p2)
        G[neg[0]] = G[a] = Q[0]                                        # non-positive first (lower index), positive second ...
        G[p2] = G[b] = Q[4]                                            # ... and the other way round
        assert len({neg[0], a, p2, b}) == 4 and neg[0] < a and p2 < b
    g_img = [f'im{i}' for i in range(Ng)]
    q_img = []
    for i in range(Nq):
        own = [g_img[j] for j in torch.randint(0, Ng, (i % 4,), generator=g).tolist()]
        pos = (gp == qp[i]).nonzero().flatten().tolist()
        if pos and i % 2:
            own = own[:3] + [g_img[pos[0]]]
        q_img.append(own)
    assert {len(x) for x in q_img} == {0, 1, 2, 3, 4}
    return Q, G, qp, gp, q_img, g_img
