"""DBSCAN on the k-reciprocal Jaccard distance (prcv2025reid_amd/cluster.py, csrc/cluster.hip) per stage, against the same stages
written with torch ops in the same session.

    python tools/cluster_times.py [--cases 16384:dense,16384:sparse,200000:sparse] [--D 256] [--runs 5] [--chunk 1024]
                                  [--per-id 16] [--noise 1.0] [--walk 0.0] [--summary table.md] [--no-sklearn]

Seeded synthetic identities (``--per-id`` unit rows each: centroid + noise, with ``--walk`` a random walk along the identity's rows, which
gives chain-shaped clusters, border rows and noise), ClusterParams' defaults (k1 = 30, k2 = 6, eps = 0.6, min_samples = 4).  Stages,
each timed with device events around work that ends in a synchronise, after a warm-up of the same shape:
  build       the pooled re-ranker (``for_pool``): kNN lists, weights, expansion
  rows        every chunk's s* rows (``rows(a, b)``), drawn and dropped
  count+fill  per resident chunk: reid_dbscan_count, the chunk's cumsum and its one host read, reid_dbscan_fill -- in turns with
              ``(S >= thr)`` with the diagonal set and ``.nonzero()`` on the same rows; the two CSRs must be equal
  components  the hook / compress rounds on the finished CSR, host reads included -- in turns with the same CSR turned into edge vectors,
              ``scatter_reduce_('amin')`` hook rounds and pointer jumping ``parent = parent[parent]``; the roots must be equal
  border      reid_dbscan_border -- in turns with the core -> non-core edge vectors and one ``scatter_reduce_('amin')``
and the whole ``jaccard_dbscan`` call.  At 16 384 rows, when sklearn imports, also ``sklearn.cluster.DBSCAN(metric='precomputed')`` on
the distance matrix copied back to the host (the copy and the clustering timed apart, host clock), and whether its labels are ours.
One JSON line per case; ``--summary`` writes the same numbers as a markdown table, every stage where the torch form wins included."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from prcv2025reid_amd import ops
from prcv2025reid_amd.cluster import ClusterParams, cluster_scores, jaccard_dbscan, round_cap
from prcv2025reid_amd.rerank import Reranker, SparseReranker

UNREACHED = 2 ** 31 - 1


def event_ms(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'runs': len(ms)}


def timed_alternating(fns, runs, warmup=1):
    """Several callables in one session, taking turns run by run, so that a change of the GPU's state falls on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            ms[name].append(event_ms(fn)[0])
    return {name: stats(v) for name, v in ms.items()}


def identities(N, D, dev, seed=0, per_id=16, noise=1.0, walk=0.0):
    """Unit rows of ceil(N / per_id) identities in a permuted order: centroid + noise * N(0, 1) and, with ``walk`` > 0, a random walk of
    that step along the identity's rows (a tracklet that drifts: chain-shaped clusters, border rows, noise)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    n_id = (N + per_id - 1) // per_id
    cent = torch.randn(n_id, D, device=dev, generator=g)
    X = cent[:, None, :] + noise * torch.randn(n_id, per_id, D, device=dev, generator=g)
    if walk:
        X = X + walk * torch.randn(n_id, per_id, D, device=dev, generator=g).cumsum(1)
    pid = torch.arange(n_id, device=dev).repeat_interleave(per_id)
    order = torch.randperm(n_id * per_id, device=dev, generator=g)[:N]
    return torch.nn.functional.normalize(X.reshape(-1, D)[order], dim=1).contiguous(), pid[order]


# ------------------------------------------------------------------------------------------------ the stages, ours and in torch ops
def ours_count_fill(S, N, a, thr, min_samples):
    nr = S.shape[0]
    count = torch.empty(nr, dtype=torch.int32, device=S.device)
    core = torch.empty(nr, dtype=torch.uint8, device=S.device)
    ops.dbscan_count(S, N, a, thr, min_samples, count, core)
    ptr = torch.zeros(nr + 1, dtype=torch.int64, device=S.device)
    torch.cumsum(count, 0, dtype=torch.int64, out=ptr[1:])
    cols = torch.empty(int(ptr[nr]), dtype=torch.int32, device=S.device)
    ops.dbscan_fill(S, N, a, thr, ptr, cols)
    return count, core, cols


def torch_count_fill(S, N, a, thr, min_samples):
    nr = S.shape[0]
    near = S[:, :N] >= thr
    near[torch.arange(nr, device=S.device), torch.arange(a, a + nr, device=S.device)] = True
    count = near.sum(1, dtype=torch.int32)
    cols = near.nonzero()[:, 1].int()                                   # row-major: ascending inside a row (one host read, as ours)
    return count, (count >= min_samples).to(torch.uint8), cols


def ours_components(rowptr, cols, core):
    N = core.shape[0]
    parent = torch.arange(N, dtype=torch.int32, device=core.device)
    changed = torch.zeros(round_cap(N), dtype=torch.int32, device=core.device)
    for r in range(round_cap(N)):
        ops.dbscan_hook(rowptr, cols, core, parent, changed[r:r + 1])
        if int(changed[r]) == 0:
            return parent, r + 1
        ops.dbscan_compress(parent)
    raise RuntimeError('components did not settle')


def torch_components(rowptr, cols, core):
    """The same scheme in torch ops from the same CSR: the core-core edges as index vectors, amin hooks on the parents, then pointer
    jumping to the roots."""
    N = core.shape[0]
    src, dst = edge_lists(rowptr, cols, core, to_core=True)
    parent = torch.arange(N, dtype=torch.int64, device=src.device)
    rounds = 0
    while True:
        rounds += 1
        pu, pv = parent[src], parent[dst]
        differ = pu != pv
        if not bool(differ.any()):
            return parent.int(), rounds
        parent.scatter_reduce_(0, torch.maximum(pu, pv)[differ], torch.minimum(pu, pv)[differ], 'amin')
        while True:
            up = parent[parent]
            if torch.equal(up, parent):
                break
            parent = up


def edge_lists(rowptr, cols, core, to_core):
    """The edges of the CSR from a core to a core (``to_core``) or to a non-core row, as index vectors (src, dst), for the torch forms."""
    N = core.shape[0]
    src = torch.repeat_interleave(torch.arange(N, device=cols.device), rowptr[1:] - rowptr[:-1], output_size=cols.shape[0])
    dst = cols.long()
    c = core.bool()
    keep = c[src] & (c[dst] if to_core else ~c[dst])
    return src[keep], dst[keep]


def run_case(N, sparse, D, runs, chunk, with_sklearn, data):
    dev = torch.device('cuda', 0)
    params = ClusterParams(sparse=sparse)
    rp = params.rerank_params(N)
    thr, ms_ = params.threshold, params.min_samples
    X, pid = identities(N, D, dev, **data)
    res = {'N': N, 'D': D, 'form': 'sparse' if sparse else 'dense', 'chunk': chunk, 'k1': params.k1, 'k2': params.k2, 'eps': params.eps,
           'min_samples': ms_, 'data': data}
    cls = SparseReranker if sparse else Reranker
    heavy = max(1, runs if N <= 65536 else 1)                            # runs of the stages that take seconds at 200 000 rows

    cls.for_pool(X, rp)                                                  # warm-up
    torch.cuda.synchronize()
    build = [event_ms(lambda: cls.for_pool(X, rp)) for _ in range(heavy)]
    res['build'] = stats([b[0] for b in build])
    rr = build[-1][1]
    del build
    starts = list(range(0, N, chunk))

    def all_rows():
        for a in starts:
            rr.rows(a, min(N, a + chunk))
    all_rows() if N <= 65536 else rr.rows(0, chunk)
    torch.cuda.synchronize()
    res['rows'] = stats([event_ms(all_rows)[0] for _ in range(heavy)])

    # count + fill per resident chunk, both forms in turns on the same rows; the first chunk once more beforehand as warm-up
    S = rr.rows(0, min(N, chunk))
    ours_count_fill(S, N, 0, thr, ms_); torch_count_fill(S, N, 0, thr, ms_)
    t_ours = t_torch = 0.0
    counts, cores, parts = [], [], []
    for a in starts:
        S = rr.rows(a, min(N, a + chunk))
        torch.cuda.synchronize()
        m1, (count, core, cols) = event_ms(lambda: ours_count_fill(S, N, a, thr, ms_))
        m2, (count_t, core_t, cols_t) = event_ms(lambda: torch_count_fill(S, N, a, thr, ms_))
        assert torch.equal(count, count_t) and torch.equal(core, core_t) and torch.equal(cols, cols_t), f'chunk at {a}: the two CSRs differ'
        t_ours += m1; t_torch += m2
        counts.append(count); cores.append(core); parts.append(cols)
    del S
    res['count_fill'] = {'ours_ms': t_ours, 'torch_ms': t_torch, 'chunks': len(starts)}
    core = torch.cat(cores)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.cat(counts), 0, dtype=torch.int64, out=rowptr[1:])
    cols = torch.cat(parts)
    del parts
    res['nnz_per_row'] = cols.shape[0] / N
    res['cores'] = int(core.sum())

    parent, rounds = ours_components(rowptr, cols, core)
    parent_t, rounds_t = torch_components(rowptr, cols, core)
    assert torch.equal(parent, parent_t), 'the two forms find different roots'
    res['components'] = timed_alternating({'ours': lambda: ours_components(rowptr, cols, core),
                                           'torch': lambda: torch_components(rowptr, cols, core)}, runs)
    res['components'].update(rounds=rounds, torch_rounds=rounds_t, core_core_edges=int(edge_lists(rowptr, cols, core, True)[0].shape[0]))

    start = torch.where(core.bool(), parent, torch.full_like(parent, UNREACHED))

    def ours_border():
        label = start.clone()
        ops.dbscan_border(rowptr, cols, core, parent, label)
        return label

    def torch_border():
        bsrc, bdst = edge_lists(rowptr, cols, core, to_core=False)
        return start.clone().scatter_reduce_(0, bdst, parent[bsrc], 'amin')
    assert torch.equal(ours_border(), torch_border()), 'the two forms label border rows differently'
    res['border'] = timed_alternating({'ours': ours_border, 'torch': torch_border}, runs)
    res['border']['core_border_edges'] = int(edge_lists(rowptr, cols, core, False)[0].shape[0])
    del rr
    torch.cuda.empty_cache()

    jaccard_dbscan(X, params, normalized=True, chunk=chunk) if N <= 65536 else None      # warm-up
    whole = [event_ms(lambda: jaccard_dbscan(X, params, normalized=True, chunk=chunk)) for _ in range(heavy)]
    res['whole_call'] = stats([w[0] for w in whole])
    got = whole[-1][1]
    assert torch.equal(got.rowptr, rowptr) and torch.equal(got.cols, cols) and got.rounds <= round_cap(N)
    res.update(n_clusters=got.n_clusters, noise_rows=int((got.labels < 0).sum()), identities=int(pid.max()) + 1,
               border_rows=int(((got.labels >= 0) & ~got.core).sum()), largest_cluster=int(torch.bincount(got.labels[got.labels >= 0]).max()))
    res['precision'], res['recall'], res['f1'] = cluster_scores(got.labels, pid)

    if with_sklearn and N <= 16384:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            res['sklearn'] = 'not importable on this machine: not measured'
        else:
            rr = cls.for_pool(X, rp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            # (s* of a row against itself can round an ulp above 1; sklearn refuses negative distances)
            dist = (1.0 - torch.cat([rr.rows(a, min(N, a + chunk))[:, :N] for a in starts])).clamp_(min=0).cpu().numpy()
            t1 = time.perf_counter()
            # float32(1 - s*) <= eps against s* >= float32(1 - eps): the same neighbours except for an s* within an ulp of the threshold
            labels = DBSCAN(eps=params.eps, min_samples=ms_, metric='precomputed').fit(dist).labels_
            t2 = time.perf_counter()
            res['sklearn'] = {'rows_and_copy_ms': (t1 - t0) * 1e3, 'dbscan_ms': (t2 - t1) * 1e3,
                              'labels_equal_ours': bool((torch.as_tensor(labels) == got.labels.cpu()).all())}
    return res


def markdown(results):
    out = ['| N | form | stage | ours, ms | torch ops, ms | note |', '|---|---|---|---|---|---|']
    fmt = lambda s: f"{s['median_ms']:.3f} ({s['min_ms']:.3f}–{s['max_ms']:.3f}, {s['runs']} runs)"
    for r in results:
        head = f"| {r['N']} | {r['form']} "
        out.append(head + f"| build (`for_pool`) | {fmt(r['build'])} | | |")
        out.append(head + f"| `rows`, {r['count_fill']['chunks']} chunks of {r['chunk']} | {fmt(r['rows'])} | | |")
        cf = r['count_fill']
        out.append(head + f"| count + fill, all chunks | {cf['ours_ms']:.3f} | {cf['torch_ms']:.3f} | one pass over the chunks, sums; "
                   f"{r['nnz_per_row']:.1f} neighbours per row, {r['cores']} cores{'; torch wins' if cf['torch_ms'] < cf['ours_ms'] else ''} |")
        for stage, note in (('components', f"{r['components']['rounds']} rounds (torch {r['components']['torch_rounds']}), "
                                           f"{r['components']['core_core_edges']} core-core edges"),
                            ('border', f"{r['border']['core_border_edges']} core-border edges")):
            s = r[stage]
            wins = '; torch wins' if s['torch']['median_ms'] < s['ours']['median_ms'] else ''
            out.append(head + f"| {stage} | {fmt(s['ours'])} | {fmt(s['torch'])} | {note}{wins} |")
        out.append(head + f"| whole `jaccard_dbscan` | {fmt(r['whole_call'])} | | {r['n_clusters']} clusters of {r['identities']} identities "
                   f"(largest {r['largest_cluster']} rows), {r['border_rows']} border and {r['noise_rows']} noise rows; pairwise precision "
                   f"{r['precision']:.4f}, recall {r['recall']:.4f} |")
        if isinstance(r.get('sklearn'), dict):
            s = r['sklearn']
            out.append(head + f"| sklearn on the copied-back matrix | | | rows + copy {s['rows_and_copy_ms']:.0f} ms, DBSCAN {s['dbscan_ms']:.0f} ms "
                       f"(host clock, one run); labels equal ours: {s['labels_equal_ours']} |")
        elif 'sklearn' in r:
            out.append(head + f"| sklearn | | | {r['sklearn']} |")
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='16384:dense,16384:sparse,200000:sparse')
    ap.add_argument('--D', type=int, default=256)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=1024)
    ap.add_argument('--per-id', type=int, default=16, help='rows per synthetic identity')
    ap.add_argument('--noise', type=float, default=1.0, help='noise level of a row around its centroid')
    ap.add_argument('--walk', type=float, default=0.0, help='step of a random walk along an identity\'s rows (0: none)')
    ap.add_argument('--summary', default=None, help='write the markdown table to this file')
    ap.add_argument('--no-sklearn', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('cluster_times.py measures on the GPU: no device found, nothing measured')
    results = []
    for case in args.cases.split(','):
        n, form = case.split(':')
        res = run_case(int(n), form == 'sparse', args.D, args.runs, args.chunk, not args.no_sklearn,
                       dict(per_id=args.per_id, noise=args.noise, walk=args.walk))
        print(json.dumps(res), flush=True)
        results.append(res)
        if args.summary:                                                 # after every case: a later case that fails loses nothing
            with open(args.summary, 'w') as f:
                f.write(markdown(results))


if __name__ == '__main__':
    main()
