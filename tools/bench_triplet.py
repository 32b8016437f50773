"""Batch-hard triplet loss (csrc/triplet.hip): what it costs.

    python tools/bench_triplet.py kernels     forward and backward alone at B = 64 and B = 1024 (D = 512) against the same loss written
                                              with torch ops (the usual Gram formulation) on the same GPU in the same process
    python tools/bench_triplet.py launches    device kernels per direction of both (torch profiler; a run of its own)
    python tools/bench_triplet.py step        the config-2 training step (P = 16, K = 4, rank 8: bench.py's headline, eager StepDriver)
                                              with triplet_weight 0 against 0.3, alternating blocks on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch


MARGIN = 4.0          # opens about half of the hinges of make_rows data at D = 512: both backward passes carry a real gradient


def torch_triplet(x, labels, margin=MARGIN):
    """The hand-written version: Gram-matrix distances, masked max / min, margin ranking."""
    sq = (x * x).sum(1)
    d = (sq[:, None] + sq[None, :] - 2.0 * (x @ x.t())).clamp(min=1e-12).sqrt()
    same = labels[:, None] == labels[None, :]
    eye = torch.eye(x.shape[0], dtype=torch.bool, device=x.device)
    d_ap = d.masked_fill(~same | eye, float('-inf')).max(1).values
    d_an = d.masked_fill(same, float('inf')).min(1).values
    return (d_ap - d_an + margin).clamp(min=0).mean()


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def make_calls(B, D=512, ratio=30.0):
    import triplet_ref as R
    from prcv2025reid_amd.losses import TripletHardFn
    x, labels = R.make_rows(B // 4, 4, D, ratio, seed=B, device='cuda')
    one = torch.ones((), device='cuda')
    xa = x.clone().requires_grad_(True); xb = x.clone().requires_grad_(True)
    state = {}

    def hip_fwd():
        state['hip'] = TripletHardFn.apply(xa, labels, None, MARGIN)[0]

    def hip_bwd():
        xa.grad = None
        state['hip'].backward(one, retain_graph=True)

    def torch_fwd():
        state['torch'] = torch_triplet(xb, labels)

    def torch_bwd():
        xb.grad = None
        state['torch'].backward(one, retain_graph=True)

    return dict(hip_fwd=hip_fwd, hip_bwd=hip_bwd, torch_fwd=torch_fwd, torch_bwd=torch_bwd), state


def kernels():
    for B in (64, 1024):
        calls, state = make_calls(B)
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        rec = dict(mode='kernels', B=B, D=512, margin=MARGIN, reps=1000, rounds=7)
        samples = {k: [] for k in calls}
        for _ in range(7):                                   # alternating windows: drift hits every variant alike
            for k, fn in calls.items():
                samples[k].append(window(fn, 1000))                  # 30 ... 250 ms per window
        for k, v in samples.items():
            v.sort()
            rec[k + '_us_median'] = round(v[len(v) // 2], 2); rec[k + '_us_min'] = round(v[0], 2)
        rec['loss_hip'] = float(state['hip'].detach()); rec['loss_torch_gram'] = float(state['torch'].detach())
        print(json.dumps(rec), flush=True)


def launches():
    from torch.profiler import profile, ProfilerActivity
    for B in (64, 1024):
        calls, _ = make_calls(B)
        for fn in calls.values():
            fn(); fn()
        torch.cuda.synchronize()
        rec = dict(mode='launches', B=B)
        for k, fn in calls.items():
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
            rec[k + '_device_kernels'] = len(names)
            rec[k + '_names'] = sorted(set(n[:60] for n in names))
        print(json.dumps(rec), flush=True)


def step(steps=10, rounds=6, warmup=3):
    import argparse
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    P, K, C = 16, 4, 400
    args = argparse.Namespace(optimizer='fused', accum=1, graph='off')
    steppers = {}
    for w in (0.0, 0.3):
        torch.manual_seed(0)
        model = bench.build_model(0, 8, 'bf16', C)
        model.triplet_weight = w
        batch = synthetic_batch(P, K, model.arch, seed=1000, num_classes=C)
        images = {m: t.cuda() for m, t in batch['images'].items()}
        tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
        tokens = {k: v.cuda() for k, v in tok.items()}
        st, _, _ = bench.make_stepper(model, DataParallel(model), args, images, tokens, batch['modality_mask'], batch['person_id'].cuda(), 1)
        steppers[w] = st
        for _ in range(warmup):
            L = st()
        torch.cuda.synchronize()
        print(json.dumps(dict(mode='step-warmup', triplet_weight=w, keys=sorted(L), total_loss=float(L['total_loss']),
                              triplet_loss=float(L['triplet_loss']) if 'triplet_loss' in L else None)), flush=True)
    samples = {w: [] for w in steppers}
    for _ in range(rounds):
        for w, st in steppers.items():
            samples[w].append(window(st, steps) / 1e3)
    rec = dict(mode='step', P=P, K=K, rank=8, steps_per_window=steps, rounds=rounds)
    for w, v in samples.items():
        rec[f'ms_per_step_w{w}'] = [round(t, 3) for t in v]
        s = sorted(v)
        rec[f'median_ms_w{w}'] = round(s[len(s) // 2], 3)
    rec['added_ms_median'] = round(rec['median_ms_w0.3'] - rec['median_ms_w0.0'], 3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('bench_triplet.py needs the GPU: nothing is measured without one')
    {'kernels': kernels, 'launches': launches, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
