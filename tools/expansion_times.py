"""Query expansion / database-side augmentation (csrc/expand.hip): what it costs.

    python tools/expansion_times.py kernel   reid_expand_rows alone at 200 000 rows (k = 10, kl = 11, the augmentation form) and at 10 000
                                             query rows (k = kl = 10), D = 512, against the same computation written with torch ops
                                             (table[idx] gather, pow, weighted sum, F.normalize) and next to reid_l2norm_rows on a
                                             [200 000, 512] tensor, all on the same GPU in the same process, in alternating windows
    python tools/expansion_times.py calls    whole calls of augment_gallery (200 000 x 512) and expand_queries (10 000 queries against
                                             200 000 rows), each split into its list time (GalleryIndex.topk) and its kernel time

Each mode is one GPU step: run each under its own time limit and chain them,
    timeout -k 10 600 python tools/expansion_times.py kernel && timeout -k 10 900 python tools/expansion_times.py calls
Times are HIP events around windows of many launches that end in a synchronise, after a warm-up of every shape; every line printed is
one JSON record.  Bytes of the kernel: (rows (n_used + 1) + rows) D 4 -- every used table row and x read once, out written once (the
lists themselves, 88 bytes per row, are left out); of reid_l2norm_rows: 2 rows D 4.  The torch side is given the compacted lists (the row's own
index already dropped, exactly k entries): its selection step is not timed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

NG, NQ, D, K, ALPHA = 200000, 10000, 512, 10, 3


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


def synthetic_lists(rows, kl, M, own, seed):
    """Lists as GalleryIndex.topk returns them for a large gallery: kl random rows of the table (a uniform gather), scores
    descending in (0.3, 1]; own: entry 0 is the row's own index (the augmentation form)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    nbr = torch.randint(0, M, (rows, kl), generator=g, device='cuda', dtype=torch.int32)
    if own:                                                     # the row itself first, and nowhere else in its list
        me = torch.arange(rows, device='cuda', dtype=torch.int32)[:, None]
        nbr = (me + 1 + nbr % (M - 1)) % M
        nbr[:, 0] = me[:, 0]
    score = torch.sort(0.3 + 0.7 * torch.rand(rows, kl, generator=g, device='cuda'), dim=1, descending=True)[0].contiguous()
    return nbr, score


def torch_expand(x, table, idx, score, alpha):
    w = score.clamp_min(0).pow(alpha)
    return torch.nn.functional.normalize(x + (w.unsqueeze(-1) * table[idx]).sum(1), dim=1)


def median_min(v):
    v = sorted(v)
    return round(v[len(v) // 2], 2), round(v[0], 2)


def kernel(rounds=7):
    from prcv2025reid_amd import ops
    table = unit_rows(NG, 1)
    y = torch.empty_like(table)
    for name, rows, kl, own, reps in (('augment_200000', NG, K + 1, True, 20), ('queries_10000', NQ, K, False, 200)):
        x = table if own else unit_rows(rows, 2)
        nbr, score = synthetic_lists(rows, kl, NG, own, 3)
        out = torch.empty(rows, D, device='cuda')
        idx_t, score_t = (nbr[:, 1:].long().contiguous(), score[:, 1:].contiguous()) if own else (nbr.long(), score)
        calls = {
            'hip': lambda: ops.expand_rows(x, table, nbr, score, K, ALPHA, self_base=0 if own else -1, out=out),
            'torch': lambda: torch_expand(x, table, idx_t, score_t, ALPHA),
            'l2norm_200000': lambda: ops.l2norm_rows(table, y=y),
        }
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        diff = float((calls['hip']() - calls['torch']()).abs().max())
        samples = {k: [] for k in calls}
        for _ in range(rounds):                                  # alternating windows: drift hits every variant alike
            for k, fn in calls.items():
                samples[k].append(window(fn, reps if k != 'torch' else max(3, reps // 10)))
        rec = dict(mode='kernel', case=name, rows=rows, table_rows=NG, D=D, k=K, kl=kl, alpha=ALPHA, rounds=rounds, reps=reps,
                   max_abs_diff_hip_torch=diff)
        for k, v in samples.items():
            rec[k + '_us_median'], rec[k + '_us_min'] = median_min(v)
        nbytes = (rows * (K + 1) + rows) * D * 4
        rec['hip_bytes'] = nbytes
        rec['hip_TBps'] = round(nbytes / rec['hip_us_median'] / 1e6, 3)
        rec['l2norm_TBps'] = round(2 * NG * D * 4 / rec['l2norm_200000_us_median'] / 1e6, 3)
        rec['torch_over_hip'] = round(rec['torch_us_median'] / rec['hip_us_median'], 2)
        print(json.dumps(rec), flush=True)


def calls(rounds=3):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.expansion import ExpansionParams, augment_gallery, expand_queries
    from prcv2025reid_amd.retrieval import GalleryIndex
    p = ExpansionParams(K, ALPHA)
    G, Q = unit_rows(NG, 1), unit_rows(NQ, 2)
    chunk = 16384

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    # augment_gallery, and its pieces as the function runs them
    augment_gallery(G, p, normalized=True, chunk=chunk); torch.cuda.synchronize()              # warm-up of every shape
    whole, lists, kern, build = [], [], [], []
    out = torch.empty_like(G)
    for _ in range(rounds):
        whole.append(timed(lambda: augment_gallery(G, p, normalized=True, chunk=chunk))[0])
        t, index = timed(lambda: GalleryIndex(G, normalized=True))
        build.append(t)
        tl = tk = 0.0
        for a in range(0, NG, chunk):
            b = min(NG, a + chunk)
            t, (nbr, score) = timed(lambda: index.topk(G[a:b], k=K + 1, normalized=True))
            tl += t
            tk += timed(lambda: ops.expand_rows(G[a:b], G, nbr, score, K, ALPHA, self_base=a, out=out[a:b]))[0]
        lists.append(tl); kern.append(tk)
    rec = dict(mode='calls', case='augment_gallery', rows=NG, D=D, k=K, alpha=ALPHA, chunk=chunk, rounds=rounds)
    for k, v in (('whole_ms', whole), ('index_build_ms', build), ('lists_ms', lists), ('kernel_ms', kern)):
        rec[k + '_median'], rec[k + '_min'] = median_min(v)
    print(json.dumps(rec), flush=True)

    index = GalleryIndex(G, normalized=True)
    expand_queries(Q, index, p, normalized=True); torch.cuda.synchronize()
    whole, lists, kern = [], [], []
    for _ in range(rounds):
        whole.append(timed(lambda: expand_queries(Q, index, p, normalized=True))[0])
        t, (nbr, score) = timed(lambda: index.topk(Q, k=K, normalized=True))
        lists.append(t)
        kern.append(timed(lambda: ops.expand_rows(Q, index.Gf, nbr, score, K, ALPHA))[0])
    rec = dict(mode='calls', case='expand_queries', rows=NQ, table_rows=NG, D=D, k=K, alpha=ALPHA, rounds=rounds)
    for k, v in (('whole_ms', whole), ('lists_ms', lists), ('kernel_ms', kern)):
        rec[k + '_median'], rec[k + '_min'] = median_min(v)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('expansion_times.py needs the GPU: nothing is measured without one')
    {'kernel': kernel, 'calls': calls}[sys.argv[1] if len(sys.argv) > 1 else 'kernel']()
