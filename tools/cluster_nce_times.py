"""Cluster-contrast memory loss (csrc/cluster_nce.hip): what it costs.

    python tools/cluster_nce_times.py     host time per forward (without and with the gradient pass), per update and per backward
                                          through the ops wrappers at (R, K, D) = (64, 1000, 512), (320, 8192, 512) and (320, 32768, 512),
                                          against the same computation written with torch ops in the same process -- normalize, mm,
                                          cross_entropy (autograd for the backward), an index loop for the update -- in alternating
                                          windows; and the forward's bytes per second against the table size

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

SHAPES = ((64, 1000, 512), (320, 8192, 512), (320, 32768, 512))
TAU, MOMENTUM = 0.05, 0.1


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def torch_update(table, xhat, labels, momentum):
    """Cluster-Contrast's sequential loop, as its memory's backward writes it."""
    for r, y in enumerate(labels.tolist()):
        table[y] = momentum * table[y] + (1 - momentum) * xhat[r]
        table[y] /= table[y].norm().clamp_min(1e-12)


def measure(R, K, D, reps, rounds, update_reps):
    from prcv2025reid_amd import ops
    g = torch.Generator().manual_seed(R + K)
    table = F.normalize(torch.randn(K, D, generator=g), dim=1).cuda()
    labels = torch.randint(0, K, (R // 4,), generator=g).repeat_interleave(4).cuda()      # P x K sampling: 4 rows per cluster
    x = (table[labels] + 0.5 * torch.randn(R, D, generator=g).cuda() / D ** 0.5).contiguous()
    ws = torch.empty(ops.cluster_nce_ws_floats(1, R, D, K), device='cuda')
    row_loss, tcos, res = torch.empty(R, device='cuda'), torch.empty(R, device='cuda'), torch.empty(2, device='cuda')
    dloss, dx = torch.ones(1, device='cuda'), torch.empty(R, D, device='cuda')
    ours, theirs = table.clone(), table.clone()
    xa = x.clone().requires_grad_(True)
    labels_host = labels.cpu()
    state = {}

    def torch_fwd():
        state['loss'] = F.cross_entropy(F.normalize(xa, dim=1, eps=1e-12) @ theirs.T / TAU, labels)

    def torch_fwd_nograd():
        with torch.no_grad():
            F.cross_entropy(F.normalize(x, dim=1, eps=1e-12) @ theirs.T / TAU, labels)

    def torch_fwd_bwd():
        xa.grad = None
        torch_fwd()
        state['loss'].backward()

    calls = {
        'fwd_nograd': lambda: ops.cluster_nce_fwd(x, labels, None, ours, TAU, False, ws, row_loss, tcos, res),
        'fwd_grad': lambda: ops.cluster_nce_fwd(x, labels, None, ours, TAU, True, ws, row_loss, tcos, res),
        'bwd': lambda: ops.cluster_nce_bwd(ws, res, dloss, dx),
        'torch_fwd_nograd': torch_fwd_nograd,
        'torch_fwd': torch_fwd,
        'torch_fwd_bwd': torch_fwd_bwd,
    }
    slow = {
        'update': lambda: ops.cluster_nce_update(labels, None, row_loss, tcos, ws, ours, MOMENTUM, 'mean'),
        'torch_update': lambda: torch_update(theirs, F.normalize(x, dim=1), labels_host, MOMENTUM),
    }
    rec = dict(R=R, K=K, D=D, tau=TAU, momentum=MOMENTUM, reps=reps, update_reps=update_reps, rounds=rounds, plan=list(ops.cluster_nce_plan(R, K, D)),
               table_mb=round(K * D * 4 / 1e6, 2))
    for fn in list(calls.values()) + list(slow.values()):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rec['loss_difference'] = abs(float(res[0]) - float(state['loss'].detach()))
    rec['dx_max_difference'] = float((dx - xa.grad).abs().max())
    rec['dx_max'] = float(xa.grad.abs().max())
    samples = {k: [] for k in list(calls) + list(slow)}
    for _ in range(rounds):                               # alternating windows: drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, reps))
        for k, fn in slow.items():
            samples[k].append(window(fn, update_reps))
    for k, v in samples.items():
        rec[k + '_us_median'] = round(median(v), 1); rec[k + '_us_min'] = round(min(v), 1)
    rec['torch_bwd_us_median'] = round(rec['torch_fwd_bwd_us_median'] - rec['torch_fwd_us_median'], 1)
    # bytes per second against the table size: one pass without gradients, two with
    rec['fwd_nograd_table_gbps'] = round(K * D * 4 / rec['fwd_nograd_us_median'] / 1e3, 1)
    rec['fwd_grad_table_gbps'] = round(2 * K * D * 4 / rec['fwd_grad_us_median'] / 1e3, 1)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('cluster_nce_times.py needs the GPU: nothing is measured without one')
    for R, K, D in SHAPES:
        measure(R, K, D, reps=50, rounds=5, update_reps=3)
