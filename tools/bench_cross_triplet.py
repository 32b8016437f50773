"""Cross-modal batch-hard triplet loss (csrc/cross_triplet.hip): what it costs.

    python tools/bench_cross_triplet.py kernels   forward and backward alone at (P, N = Mg, D) = (4, 64, 512), (4, 256, 512) and
                                                  (4, 1024, 512) against the same loss written with torch ops (normalise, cdist, masked
                                                  max / min, autograd) on the same GPU in the same process
    python tools/bench_cross_triplet.py step      the config-2 training step (P = 16, K = 4, rank 8: bench.py's headline, eager
                                                  StepDriver) with cross_triplet_weight 0 against 0.5, alternating blocks on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

MARGIN = 0.3          # between unit rows most hinges of make_case data are open: both backward passes carry a real gradient
SHAPES = [(4, 64, 512), (4, 256, 512), (4, 1024, 512)]


def torch_cross_triplet(q, g, ql, gl, margin=MARGIN):
    """The hand-written version for data in which every anchor has a positive and a negative: L [P]."""
    qh = torch.nn.functional.normalize(q, dim=-1); gh = torch.nn.functional.normalize(g, dim=-1)
    d = torch.cdist(qh, gh[None].expand(q.shape[0], -1, -1))                       # [P, N, Mg]
    same = (ql[:, None] == gl[None, :])[None]
    pos, neg = d.masked_fill(~same, float('-inf')), d.masked_fill(same, float('inf'))
    lq = (pos.max(2).values - neg.min(2).values + margin).clamp(min=0).mean(1)
    lg = (pos.max(1).values - neg.min(1).values + margin).clamp(min=0).mean(1)
    return 0.5 * (lq + lg)


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def make_calls(P, N, D, ratio=30.0):
    import cross_triplet_ref as R
    from prcv2025reid_amd.losses import CrossTripletFn
    q, g, ql, gl = R.make_case(P, N, N, D, ratio, seed=N, device='cuda')
    one = torch.ones((), device='cuda')
    qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    qb, gb = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    state = {}

    def hip_fwd():
        state['hip'] = CrossTripletFn.apply(qa, ga, ql, gl, None, None, MARGIN, True)[0].sum()

    def hip_bwd():
        qa.grad = ga.grad = None
        state['hip'].backward(one, retain_graph=True)

    def torch_fwd():
        state['torch'] = torch_cross_triplet(qb, gb, ql, gl).sum()

    def torch_bwd():
        qb.grad = gb.grad = None
        state['torch'].backward(one, retain_graph=True)

    return dict(hip_fwd=hip_fwd, hip_bwd=hip_bwd, torch_fwd=torch_fwd, torch_bwd=torch_bwd), state


def kernels(reps=500, rounds=7):
    for P, N, D in SHAPES:
        calls, state = make_calls(P, N, D)
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        rec = dict(mode='kernels', P=P, N=N, Mg=N, D=D, margin=MARGIN, reps=reps, rounds=rounds)
        samples = {k: [] for k in calls}
        for _ in range(rounds):                              # alternating windows: drift hits every variant alike
            for k, fn in calls.items():
                samples[k].append(window(fn, reps))
        for k, v in samples.items():
            v.sort()
            rec[k + '_us_median'] = round(v[len(v) // 2], 2); rec[k + '_us_min'] = round(v[0], 2)
        rec['loss_sum_hip'] = float(state['hip'].detach()); rec['loss_sum_torch'] = float(state['torch'].detach())
        print(json.dumps(rec), flush=True)


def step(steps=10, rounds=6, warmup=3):
    import argparse
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    P, K, C = 16, 4, 400
    args = argparse.Namespace(optimizer='fused', accum=1, graph='off')
    steppers = {}
    for w in (0.0, 0.5):
        torch.manual_seed(0)
        model = bench.build_model(0, 8, 'bf16', C)
        model.cross_triplet_weight = w
        batch = synthetic_batch(P, K, model.arch, seed=1000, num_classes=C)
        images = {m: t.cuda() for m, t in batch['images'].items()}
        tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
        tokens = {k: v.cuda() for k, v in tok.items()}
        st, _, _ = bench.make_stepper(model, DataParallel(model), args, images, tokens, batch['modality_mask'], batch['person_id'].cuda(), 1)
        steppers[w] = st
        for _ in range(warmup):
            L = st()
        torch.cuda.synchronize()
        print(json.dumps(dict(mode='step-warmup', cross_triplet_weight=w, keys=sorted(L), total_loss=float(L['total_loss'].detach()),
                              cross_triplet_loss=float(L['cross_triplet_loss'].detach()) if 'cross_triplet_loss' in L else None,
                              active=int(L['cross_triplet_active_cnt']) if 'cross_triplet_active_cnt' in L else None)), flush=True)
    samples = {w: [] for w in steppers}
    for _ in range(rounds):
        for w, st in steppers.items():
            samples[w].append(window(st, steps) / 1e3)
    rec = dict(mode='step', P=P, K=K, rank=8, steps_per_window=steps, rounds=rounds)
    for w, v in samples.items():
        rec[f'ms_per_step_w{w}'] = [round(t, 3) for t in v]
        s = sorted(v)
        rec[f'median_ms_w{w}'] = round(s[len(s) // 2], 3)
    rec['added_ms_median'] = round(rec['median_ms_w0.5'] - rec['median_ms_w0.0'], 3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('bench_cross_triplet.py needs the GPU: nothing is measured without one')
    {'kernels': kernels, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
