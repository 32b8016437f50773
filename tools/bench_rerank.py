"""k-reciprocal re-ranking (prcv2025reid_amd/rerank.py, csrc/rerank.hip) per stage at protocol scale.

    python tools/bench_rerank.py [--shapes 4096x16384,2048x8192] [--D 512] [--k1 20] [--k2 6] [--runs 10] [--yard-runs 10]
    python tools/bench_rerank.py --sparse [--shapes 4096x16384,2048x8192,10000x200000] ...
    python tools/bench_rerank.py [--sparse] --lists 100 [--lists-only] ...

Seeded clustered rows (16 images per identity), warm-up, then ``--runs`` timed runs per stage with device events: median, min and
max in ms.  Stages: pooled kNN lists, cosine rows (all query chunks), weights, expand, Jaccard (all query chunks).  The Jaccard
stage does Nq * Ng * N min-add pairs; its rate is pairs over the median time.

Yardstick of the Jaccard stage (there is no older implementation): the same definition in torch ops on the same GPU and the same
V2, chunked ``torch.minimum(A[:, None, :], B[None, :, :]).sum(-1)``, then J and the blend.  Its result is compared with the
kernel's before it is timed.  Last, the accuracy line: mAP of the small Gaussian test fixture before and after re-ranking, fp64
reference against the evaluator.  One JSON line per shape and one for the accuracy line.

``--sparse``: the same stages of the sparse form (RerankParams(sparse=True): padded weights, count + cumsum + fill, the transposition
of the gallery rows, the sparse Jaccard), the whole call, the whole evaluation through ``ProtocolEvaluator.per_query``, nnz(V2) / N,
the s* row traffic of the Jaccard stage against its three-pass budget, and the peak device memory of one whole call
(``torch.cuda.max_memory_allocated``).  No torch yardstick (it needs the dense V2); the accuracy line runs the sparse form.

``--lists K`` (default 100; 0 skips it), in both modes: the ranked lists of the s* rows.  Every chunk's rows stay on the device
(Nq * Ng * 4 bytes); ``ops.rows_topk`` and the yardstick -- the stable descending sort ``export_submission_csv`` used before,
``torch.sort(..., stable=True)[1][:, :K]`` on the same rows -- must give identical lists, then take turns for 2 warm-up and ``--runs``
timed runs each (device events).  Reported: both timings, Nq * Ng * 4 bytes over the kernel's median as TB/s, the peak device memory
of each, and the whole ``ProtocolEvaluator.ranked_lists`` call.  ``--lists-only`` runs nothing else."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from prcv2025reid_amd import ops
from prcv2025reid_amd.evaluate import ProtocolEvaluator, split_gallery, split_scores
from prcv2025reid_amd.rerank import RerankParams, Reranker, SparseReranker, csc_of_rows, list_width
from prcv2025reid_amd.retrieval import GalleryIndex


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'runs': runs}


def timed_alternating(fns, runs, warmup=2):
    """``timed`` for several callables measured in ONE session, taking turns run by run, so that a change of the GPU's state
    (clocks, other tenants) falls on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'runs': runs} for name, v in ms.items()}


def peak_over_base(fn):
    """Peak device memory of one call above what was allocated before it, in bytes."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def lists_stage(X, pid, Nq, Ng, params, K, runs, chunk):
    """Ranked lists of length K from the s* rows of every query chunk, resident on the device: ``ops.rows_topk`` against the stable
    sort it replaces in ``export_submission_csv`` (compared before anything is timed, then timed in turns), the whole
    ``ProtocolEvaluator.ranked_lists`` call, and the peak device memory of each."""
    starts = list(range(0, Nq, chunk))
    rr = (SparseReranker if params.sparse else Reranker)(X[:Nq], X[Nq:], params)
    rows = [rr.rows(a, min(Nq, a + chunk)) for a in starts]
    del rr
    torch.cuda.empty_cache()

    def kernel():
        return torch.cat([ops.rows_topk(S, Ng, K)[0] for S in rows], 0)

    def sort():
        return torch.cat([torch.sort(S[:, :Ng], dim=1, descending=True, stable=True)[1][:, :K] for S in rows], 0)     # the line it replaces
    assert torch.equal(kernel().long(), sort()), 'ops.rows_topk and the stable sort disagree'
    res = {'K': K, 'row_bytes': float(Nq) * Ng * 4}
    res.update(timed_alternating({'kernel': kernel, 'stable_sort': sort}, runs))
    res['kernel_TBps'] = res['row_bytes'] / (res['kernel']['median_ms'] * 1e-3) / 1e12
    res['sort_min_over_kernel_median'] = res['stable_sort']['min_ms'] / res['kernel']['median_ms']
    res['kernel_peak_memory_bytes'] = peak_over_base(kernel)
    res['stable_sort_peak_memory_bytes'] = peak_over_base(sort)
    zeros = [float((S[:, :Ng] == 0).float().mean()) for S in rows[:1]]
    res['zero_fraction_first_chunk'] = zeros[0]
    del rows
    torch.cuda.empty_cache()
    ev = ProtocolEvaluator(X[Nq:], pid[Nq:], normalized=True)

    def whole():
        return ev.ranked_lists(X[:Nq], k=K, chunk=chunk, normalized=True, rerank=params)
    res['ranked_lists_call'] = timed(whole, max(3, runs // 3), warmup=1)
    res['ranked_lists_peak_memory_bytes'] = peak_over_base(whole)
    return res


def clustered(Nq, Ng, D, dev, seed=0, per_id=16, noise=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    N = Nq + Ng
    cent = torch.randn((N + per_id - 1) // per_id, D, device=dev, generator=g)
    pid = torch.randperm(N, device=dev, generator=g) % cent.shape[0]
    X = cent[pid] + noise * torch.randn(N, D, device=dev, generator=g)
    return torch.nn.functional.normalize(X, dim=1), pid


def torch_jaccard(A, B, cos, lam, qc=64, gc=1024):
    out = torch.empty(A.shape[0], B.shape[0], device=A.device)
    for a in range(0, A.shape[0], qc):
        for b in range(0, B.shape[0], gc):
            m = torch.minimum(A[a:a + qc, None, :], B[None, b:b + gc, :]).sum(-1)
            out[a:a + qc, b:b + gc] = (1 - lam) * (m / (2 - m)) + lam * cos[a:a + qc, b:b + gc]
    return out


def run_shape(Nq, Ng, D, params, runs, yard_runs, chunk, lists=0, lists_only=False):
    dev = torch.device('cuda', 0)
    X, pid = clustered(Nq, Ng, D, dev)
    N = Nq + Ng
    k1, k2, lam = params.k1, params.k2, params.lambda_value
    res = {'Nq': Nq, 'Ng': Ng, 'N': N, 'D': D, 'k1': k1, 'k2': k2, 'lambda': lam, 'chunk': chunk}
    if lists:
        res['lists'] = lists_stage(X, pid, Nq, Ng, params, lists, runs, chunk)
    if lists_only:
        return res
    index = GalleryIndex(X, normalized=True)
    res['knn_lists'] = timed(lambda: index.topk(X, k=k1 + 1, normalized=True), runs)
    nbr = index.topk(X, k=k1 + 1, normalized=True)[0]
    Gcat = split_gallery(X[Nq:])
    res['cosine_rows'] = timed(lambda: [split_scores(X[a:a + chunk], Gcat) for a in range(0, Nq, chunk)], runs)
    ld = (N + 3) // 4 * 4
    V = torch.empty(N, ld, device=dev); V2 = torch.empty(N, ld, device=dev)
    res['weights'] = timed(lambda: ops.rerank_weights(nbr, X, V, k1), runs)
    res['expand'] = timed(lambda: ops.rerank_expand(V, nbr, V2, k1, k2), runs)
    res['v2_nonzero_fraction'] = float((V2[:, :N] != 0).float().mean())
    cos = [split_scores(X[a:a + chunk], Gcat) for a in range(0, Nq, chunk)]
    outs = [torch.empty_like(c) for c in cos]

    def jaccard():
        for i, a in enumerate(range(0, Nq, chunk)):
            ops.rerank_jaccard(V2[a:a + chunk], V2[Nq:], cos[i], outs[i], Ng, N, lam)
    res['jaccard'] = timed(jaccard, runs)
    pairs = float(Nq) * Ng * N
    res['jaccard_pairs'] = pairs
    res['jaccard_pairs_per_s'] = pairs / (res['jaccard']['median_ms'] * 1e-3)
    res['total_median_ms'] = sum(res[s]['median_ms'] for s in ('knn_lists', 'cosine_rows', 'weights', 'expand', 'jaccard'))
    res['whole_call'] = timed(lambda: [Reranker(X[:Nq], X[Nq:], params, Gcat).rows(a, min(Nq, a + chunk)) for a in range(0, Nq, chunk)][-1],
                              max(3, runs // 3), warmup=1)
    # yardstick: the same V2 through torch ops; compared before it is timed
    A, B = V2[:Nq, :N], V2[Nq:, :N]
    cos_all = torch.cat([c[:, :Ng] for c in cos], 0)
    want = torch_jaccard(A[:128], B, cos_all[:128], lam)
    res['kernel_vs_torch_max_abs'] = float((outs[0][:128, :Ng] - want).abs().max())
    res['torch_jaccard'] = timed(lambda: torch_jaccard(A, B, cos_all, lam), yard_runs, warmup=1)
    res['torch_over_kernel'] = res['torch_jaccard']['median_ms'] / res['jaccard']['median_ms']
    return res


def run_shape_sparse(Nq, Ng, D, params, runs, chunk, lists=0, lists_only=False):
    dev = torch.device('cuda', 0)
    X, pid = clustered(Nq, Ng, D, dev)
    N = Nq + Ng
    k1, k2, lam = params.k1, params.k2, params.lambda_value
    res = {'form': 'sparse', 'Nq': Nq, 'Ng': Ng, 'N': N, 'D': D, 'k1': k1, 'k2': k2, 'lambda': lam, 'chunk': chunk}
    if lists:
        res['lists'] = lists_stage(X, pid, Nq, Ng, params, lists, runs, chunk)
    if lists_only:
        return res
    few = max(3, runs // 3)
    index = GalleryIndex(X, normalized=True)
    index.exact_scratch_bytes = 2 << 30
    res['knn_lists'] = timed(lambda: index.topk(X, k=k1 + 1, normalized=True), runs if N <= 65536 else few, warmup=1)
    nbr = index.topk(X, k=k1 + 1, normalized=True)[0]
    del index
    Gcat = split_gallery(X[Nq:])
    res['cosine_rows'] = timed(lambda: [split_scores(X[a:a + chunk], Gcat) for a in range(0, Nq, chunk)], runs)
    W = list_width(k1)
    vcols = torch.empty(N, W, dtype=torch.int32, device=dev); vvals = torch.empty(N, W, device=dev)
    vcnt = torch.empty(N, dtype=torch.int32, device=dev); cnt = torch.empty(N, dtype=torch.int32, device=dev)
    res['weights'] = timed(lambda: ops.rerank_weights_sparse(nbr, X, vcols, vvals, vcnt, k1), runs)
    res['expand_count'] = timed(lambda: ops.rerank_expand_count(vcols, vvals, vcnt, nbr, cnt, k1, k2), runs)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cnt.long().cumsum(0)])
    nnz, first = int(rowptr[N]), int(rowptr[Nq])
    cols = torch.empty(nnz, dtype=torch.int32, device=dev); vals = torch.empty(nnz, device=dev)
    res['expand_fill'] = timed(lambda: ops.rerank_expand_sparse(vcols, vvals, vcnt, nbr, rowptr, cols, vals, k1, k2), runs)
    res['nnz_v2_per_row'] = nnz / N
    res['v2_nonzero_fraction'] = nnz / N / N
    res['transpose'] = timed(lambda: csc_of_rows(cols[first:], vals[first:], cnt[Nq:], N), runs)
    colptr, grows, cvals = csc_of_rows(cols[first:], vals[first:], cnt[Nq:], N)
    res['longest_csc_column'] = int((colptr[1:] - colptr[:-1]).max())
    starts = list(range(0, Nq, chunk))
    few_rows = Nq * Ng > (1 << 28)                              # the cosine rows of every chunk at once would be Nq * Ng * 8 bytes
    cos = None if few_rows else [split_scores(X[a:a + chunk], Gcat) for a in starts]
    outs = None if few_rows else [torch.empty_like(c) for c in cos]
    if few_rows:
        cos1 = split_scores(X[:chunk], Gcat); out1 = torch.empty_like(cos1)

    def jaccard():
        for i, a in enumerate(starts):
            b = min(Nq, a + chunk)
            if few_rows:                                        # one cosine chunk for every query chunk: the same traffic, not the same values
                ops.rerank_jaccard_sparse(rowptr[a:b + 1], cols, vals, colptr, grows, cvals, cos1[:b - a], out1[:b - a], Ng, lam)
            else:
                ops.rerank_jaccard_sparse(rowptr[a:b + 1], cols, vals, colptr, grows, cvals, cos[i], outs[i], Ng, lam)
    res['jaccard'] = timed(jaccard, runs)
    # the budget: three passes over every s* row (zero fill, accumulate in place, finish) plus the cosine row read once
    res['jaccard_row_bytes'] = float(Nq) * Ng * 4 * 4
    res['jaccard_row_GBps'] = res['jaccard_row_bytes'] / (res['jaccard']['median_ms'] * 1e-3) / 1e9
    stages = ('knn_lists', 'cosine_rows', 'weights', 'expand_count', 'expand_fill', 'transpose', 'jaccard')
    res['total_median_ms'] = sum(res[s]['median_ms'] for s in stages)
    res['jaccard_share'] = res['jaccard']['median_ms'] / res['total_median_ms']
    del vcols, vvals, cols, vals, colptr, grows, cvals, cos, outs
    torch.cuda.empty_cache()

    def whole():
        rr = SparseReranker(X[:Nq], X[Nq:], params, Gcat)
        return [rr.rows(a, min(Nq, a + chunk)) for a in starts][-1]
    res['whole_call'] = timed(whole, few, warmup=1)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    whole()
    torch.cuda.synchronize()
    res['peak_memory_bytes'] = torch.cuda.max_memory_allocated()
    res['peak_memory_over_inputs_bytes'] = res['peak_memory_bytes'] - base
    ev = ProtocolEvaluator(X[Nq:], pid[Nq:], normalized=True)
    res['per_query_evaluation'] = timed(lambda: ev.per_query(X[:Nq], pid[:Nq], normalized=True, chunk=chunk, rerank=params), few, warmup=1)
    return res


def accuracy_line(sparse=False):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import numpy as np
    import rerank_ref as R
    X, qp, gp = R.gaussian_fixture(422, 32, 219, 64, 24, 2.2)
    Nq, k1, k2, lam = 32, 8, 3, 0.3
    ref = R.rerank_ref(X, Nq, k1, k2, lam)
    keep = np.ones(len(gp), bool)

    def mean_ap(s):
        return float(np.mean([R.ap_cmc(s[i], gp, qp[i], keep)[0] for i in range(Nq)]))
    ev = ProtocolEvaluator(torch.as_tensor(X[Nq:]).cuda(), torch.as_tensor(gp), normalized=True)
    Q, qpt = torch.as_tensor(X[:Nq]).cuda(), torch.as_tensor(qp)
    return {'fixture': 'gaussian seed 422, 32 x 219, D 64, k1 8, k2 3, lambda 0.3',
            'ref_mAP_cosine': mean_ap(ref['cos'][:Nq, Nq:]), 'ref_mAP_reranked': mean_ap(ref['s']),
            'gpu_mAP_cosine': ev.rank_and_metrics(Q, qpt)['mAP'],
            'gpu_mAP_reranked': ev.rank_and_metrics(Q, qpt, rerank=RerankParams(k1, k2, lam, sparse=sparse))['mAP']}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x16384,2048x8192')
    ap.add_argument('--D', type=int, default=512)
    ap.add_argument('--k1', type=int, default=20)
    ap.add_argument('--k2', type=int, default=6)
    ap.add_argument('--lambda-value', type=float, default=0.3)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--yard-runs', type=int, default=10)
    ap.add_argument('--chunk', type=int, default=1024)
    ap.add_argument('--sparse', action='store_true', help='the sparse form (RerankParams(sparse=True)); takes shapes beyond 65 536 pooled rows')
    ap.add_argument('--lists', type=int, default=100, help='length K of the ranked lists stage (ops.rows_topk against the stable sort); 0 = skip it')
    ap.add_argument('--lists-only', action='store_true', help='the ranked lists stage alone')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_rerank.py needs the GPU: nothing is measured without one')
    for shape in a.shapes.split(','):
        Nq, Ng = (int(v) for v in shape.split('x'))
        if a.sparse:
            print(json.dumps(run_shape_sparse(Nq, Ng, a.D, RerankParams(a.k1, a.k2, a.lambda_value, sparse=True), a.runs, a.chunk, a.lists,
                                              a.lists_only)), flush=True)
        else:
            print(json.dumps(run_shape(Nq, Ng, a.D, RerankParams(a.k1, a.k2, a.lambda_value), a.runs, a.yard_runs, a.chunk, a.lists,
                                       a.lists_only)), flush=True)
    if not a.lists_only:
        print(json.dumps(accuracy_line(a.sparse)), flush=True)
