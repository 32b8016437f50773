"""Cutoff metrics (csrc/metrics.hip reid_rank_metrics_at, csrc/list_metrics.hip reid_list_metrics): what they cost.

    python tools/metrics_at_k_times.py rows    reid_rank_metrics_at with cutoffs (1, 5, 10, 100), and with (100,) alone, against
                                               reid_rank_metrics on the same 1024 x 200 000 fp32 score rows (20 gallery rows per
                                               identity), alternating windows
    python tools/metrics_at_k_times.py lists   reid_list_metrics on 10 000 lists of 100 against the same quantities written with torch
                                               ops (gather, compare, cumsum, divide, masked sums, bincount for npos)
    python tools/metrics_at_k_times.py calls   whole ProtocolEvaluator.rank_and_metrics(ks=(100,)) calls against today's call,
                                               10 000 queries x 200 000 gallery rows x 512

Each mode is one GPU step: run each under its own time limit and chain them,
    timeout -k 10 300 python tools/metrics_at_k_times.py rows && timeout -k 10 300 python tools/metrics_at_k_times.py lists && \
    timeout -k 10 600 python tools/metrics_at_k_times.py calls
Times are HIP events around windows of many launches that end in a synchronise, after a warm-up of every shape; the variants of a mode
alternate window by window, so drift hits them alike; every line printed is one JSON record with the median, the minimum and the
maximum over the windows (the spread a difference has to exceed to mean anything)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

NG, D, PER_ID = 200000, 512, 20
KS = (1, 5, 10, 100)


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3            # us per call


def unit_rows(n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, D, generator=g, device='cuda'), dim=1)


def stats(v, digits=2):
    v = sorted(v)
    return round(v[len(v) // 2], digits), round(v[0], digits), round(v[-1], digits)


def alternate(calls, reps, rounds):
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            samples[k].append(window(fn, reps))
    return samples


def evaluator(nq, seed=1):
    """Gallery of NG unit rows, PER_ID rows per identity, clustered: a row is its identity's centre plus noise of 1.8 times the centre's
    norm, so two rows of one identity have a cosine of about 0.23, five standard deviations above the background of 0.044 -- most
    positives rank early, the weakest ones far down, as a trained model's do (the records carry the mean rank of the last positive).
    Queries are drawn the same way; every tenth has an identity the gallery lacks."""
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    n_id = NG // PER_ID
    centers = unit_rows(n_id, seed)
    gp = torch.arange(NG, device='cuda') % n_id
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    G = torch.nn.functional.normalize(centers[gp] + 0.08 * torch.randn(NG, D, generator=g, device='cuda'), dim=1)
    qp = torch.randint(0, n_id, (nq,), generator=g, device='cuda')
    Q = torch.nn.functional.normalize(centers[qp] + 0.08 * torch.randn(nq, D, generator=g, device='cuda'), dim=1)
    qp[::10] = NG                                           # absent from the gallery
    return ProtocolEvaluator(G, gp, normalized=True), Q, qp


def rows(rounds=9, reps=10):
    from prcv2025reid_amd import ops
    nq = 1024
    ev, Q, qp = evaluator(nq)
    S = ev.scores(Q, normalized=True)
    qp32, slot = ev._query_ids(qp)
    i32 = dict(dtype=torch.int32, device='cuda')
    ap, rank1, npos, rank_last = torch.zeros(nq, dtype=torch.float64, device='cuda'), torch.zeros(nq, **i32), torch.zeros(nq, **i32), torch.zeros(nq, **i32)
    hits, sum_at = torch.zeros(nq, len(KS), **i32), torch.zeros(nq, len(KS), dtype=torch.float64, device='cuda')
    ids = (S, ev.g_pid, ev.g_img, qp32, slot, None, ev.csr_off, ev.csr_idx, ev.Ng, ev.max_pos)
    hits1, sum1 = torch.zeros(nq, 1, **i32), torch.zeros(nq, 1, dtype=torch.float64, device='cuda')
    calls = {'rank_metrics': lambda: ops.rank_metrics(*ids, ap, rank1, npos),
             'rank_metrics_at': lambda: ops.rank_metrics_at(*ids, KS, ap, rank1, npos, rank_last, hits, sum_at),
             'rank_metrics_at_one_cutoff': lambda: ops.rank_metrics_at(*ids, KS[-1:], ap, rank1, npos, rank_last, hits1, sum1)}
    samples = alternate(calls, reps, rounds)
    rec = dict(mode='rows', nq=nq, Ng=NG, per_id=PER_ID, cutoffs=KS, rounds=rounds, reps=reps, bytes=nq * NG * 12,
               mean_rank_last=float(rank_last[npos > 0].double().mean()))
    for k, v in samples.items():
        rec[k + '_us_median'], rec[k + '_us_min'], rec[k + '_us_max'] = stats(v)
    rec['at_over_plain'] = round(rec['rank_metrics_at_us_median'] / rec['rank_metrics_us_median'], 4)
    print(json.dumps(rec), flush=True)


def torch_list_metrics(idx, g_pid, q_pid, counts, slot, ks):
    """npos, rank1, hits, sum_at of reid_list_metrics without exclusion, with torch ops."""
    k = idx.shape[1]
    hit = (g_pid[idx.clamp(min=0).long()] == q_pid[:, None]) & (idx >= 0)
    prec = hit.cumsum(1).double() / torch.arange(1, k + 1, device=idx.device, dtype=torch.float64)
    term = prec * hit
    hits = torch.stack([hit[:, :K].sum(1) for K in ks], 1).to(torch.int32)
    sum_at = torch.stack([term[:, :K].sum(1) for K in ks], 1)
    first = torch.where(hit.any(1), hit.to(torch.int8).argmax(1) + 1, 0).to(torch.int32)
    npos = torch.where(slot >= 0, counts[slot.clamp(min=0).long()], 0).to(torch.int32)
    return npos, first, hits, sum_at


def lists(rounds=9, reps=50):
    from prcv2025reid_amd import ops
    nq, k = 10000, 100
    ev, Q, qp = evaluator(nq)
    idx, _ = ev.ranked_lists(Q, k=k, normalized=True)
    qp32, slot = ev._query_ids(qp)
    counts = (ev.csr_off[1:] - ev.csr_off[:-1]).contiguous()
    out = ops.list_metrics(idx, ev.g_pid, None, qp32, slot, None, ev.csr_off, ev.csr_idx, ev.Ng, KS)
    calls = {'hip': lambda: ops.list_metrics(idx, ev.g_pid, None, qp32, slot, None, ev.csr_off, ev.csr_idx, ev.Ng, KS, out=out),
             'torch': lambda: torch_list_metrics(idx, ev.g_pid, qp32, counts, slot, KS)}
    samples = alternate(calls, reps, rounds)
    a, b = calls['hip'](), calls['torch']()
    same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    rec = dict(mode='lists', nq=nq, k=k, Ng=NG, cutoffs=KS, rounds=rounds, reps=reps, integers_equal=same,
               max_abs_diff_sum=float((a[3] - b[3]).abs().max()), mean_hits_at_100=float(a[2][:, -1].double().mean()))
    for name, v in samples.items():
        rec[name + '_us_median'], rec[name + '_us_min'], rec[name + '_us_max'] = stats(v)
    rec['torch_over_hip'] = round(rec['torch_us_median'] / rec['hip_us_median'], 2)
    print(json.dumps(rec), flush=True)


def calls(rounds=5):
    nq = 10000
    ev, Q, qp = evaluator(nq)
    variants = {'rank_and_metrics': lambda: ev.rank_and_metrics(Q, qp), 'rank_and_metrics_ks100': lambda: ev.rank_and_metrics(Q, qp, ks=(100,))}
    samples = alternate(variants, 1, rounds)
    res = variants['rank_and_metrics_ks100']()
    rec = dict(mode='calls', nq=nq, Ng=NG, D=D, rounds=rounds, result={k: round(float(v), 6) for k, v in res.items()})
    for name, v in samples.items():
        rec[name + '_ms_median'], rec[name + '_ms_min'], rec[name + '_ms_max'] = (round(x / 1e3, 3) for x in stats(v, 1))
    rec['ks_over_plain'] = round(rec['rank_and_metrics_ks100_ms_median'] / rec['rank_and_metrics_ms_median'], 4)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('metrics_at_k_times.py needs the GPU: nothing is measured without one')
    {'rows': rows, 'lists': lists, 'calls': calls}[sys.argv[1] if len(sys.argv) > 1 else 'rows']()
