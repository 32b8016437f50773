"""Cosine-margin identity heads (csrc/margin_ce.hip): what they cost.

    python tools/margin_ce_times.py head [out.md]   forward + backward of the head alone at B = 64 and 256, C = 1000, D = 512: every kind
                                                    (CosineLinearFn + MarginCEFn), the linear head the default keeps (LinearF32Fn +
                                                    CrossEntropyLSFn) and the same math written with torch ops, alternating windows in
                                                    one process; x and W both take a gradient
    python tools/margin_ce_times.py step [out.md]   the eager config-2 training step (P = 16, K = 4, LoRA rank 8, bench.py's model) with
                                                    id_head 'linear' (the parent's step: nothing of this file's subject is launched)
                                                    against 'cosface', alternating windows on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record, and the same records are
appended as a table to ``out.md`` (default profiles/margin_ce_summary.md) under a heading that names the mode."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

Pi, K, C_STEP, RANK = 16, 4, 400, 8
C, D = 1000, 512
KINDS = ('cosine', 'cosface', 'arcface', 'circle')
# launches of the library per direction (csrc/margin_ce.hip): norms, logits tiles, CE rows, CE reduction | CE, fp64 products, projections
LAUNCHES = dict(margin=dict(forward=4, backward=3), linear=dict(forward=2, backward=3))


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


def torch_margin(x, W, y, kind, s, m):
    """The same math with torch ops on the device (fp32, autograd)."""
    cos = F.linear(F.normalize(x, dim=1), F.normalize(W, dim=1))
    tgt = F.one_hot(y, W.shape[0]).bool()
    if kind == 'cosine':
        z = s * cos
    elif kind == 'cosface':
        z = s * torch.where(tgt, cos - m, cos)
    elif kind == 'arcface':
        t = cos.clamp(-1 + 2.0 ** -23, 1 - 2.0 ** -23)
        phi = torch.where(t > math.cos(math.pi - m), t * math.cos(m) - (1 - t * t).sqrt() * math.sin(m), t - m * math.sin(math.pi - m))
        z = s * torch.where(tgt, phi, cos)
    else:
        ap, an = (1 + m - cos.detach()).clamp_min(0), (cos.detach() + m).clamp_min(0)
        z = s * torch.where(tgt, ap * (cos - (1 - m)), an * (cos - m))
    return F.cross_entropy(z, y, label_smoothing=0.1)


def head(out, reps=100, rounds=7):
    from prcv2025reid_amd.head import CosineLinearFn, LinearF32Fn
    from prcv2025reid_amd.losses import CrossEntropyLSFn, MarginCEFn, MARGIN_DEFAULTS
    rows = []
    for B in (64, 256):
        g = torch.Generator(device='cuda').manual_seed(B)
        x = (8 * F.normalize(torch.randn(B, D, device='cuda', generator=g), dim=1)).requires_grad_(True)
        W = (0.02 * torch.randn(C, D, device='cuda', generator=g)).requires_grad_(True)
        y = torch.randint(0, C, (B,), device='cuda', generator=g)
        valid = torch.ones(B, dtype=torch.uint8, device='cuda')

        def run(loss_fn):
            def f():
                x.grad = W.grad = None
                loss_fn().backward()
            return f

        calls = {'linear + CE (the default head)': run(lambda: CrossEntropyLSFn.apply(LinearF32Fn.apply(x, W, None), y, valid, 0.1)[0])}
        for kind in KINDS:
            s, m = MARGIN_DEFAULTS[kind]
            calls[kind] = run(lambda kind=kind, s=s, m=m: MarginCEFn.apply(CosineLinearFn.apply(x, W, s), y, valid, 0.1, kind, s, m)[0])
            calls[kind + ', torch ops'] = run(lambda kind=kind, s=s, m=m: torch_margin(x, W, y, kind, s, m))
        for fn in calls.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in calls}
        for _ in range(rounds):                           # alternating windows: drift hits every variant alike
            for k, fn in calls.items():
                samples[k].append(window(fn, reps))
        for k, v in samples.items():
            kind = 'linear' if k.startswith('linear') else ('torch' if k.endswith('torch ops') else 'margin')
            rec = dict(mode='head', B=B, C=C, D=D, variant=k, us_median=round(median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                       reps=reps, rounds=rounds, launches_forward=LAUNCHES.get(kind, {}).get('forward'),
                       launches_backward=LAUNCHES.get(kind, {}).get('backward'))
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    with open(out, 'a') as f:
        f.write(f'\n## Head alone, forward + backward (x and W take a gradient), C = {C}, D = {D}; us per call, median (min .. max) of '
                f'{rounds} alternating windows of {reps} calls\n\n| B | variant | us | library launches fwd / bwd |\n|---|---|---|---|\n')
        for r in rows:
            la = '-' if r['launches_forward'] is None else f"{r['launches_forward']} / {r['launches_backward']}"
            f.write(f"| {r['B']} | {r['variant']} | {r['us_median']} ({r['us_min']} .. {r['us_max']}) | {la} |\n")


def step(out, steps=10, rounds=5, warmup=3):
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    from prcv2025reid_amd.losses import margin_args
    inputs, steppers, last = None, {}, {}
    for kind in ('linear', 'cosface'):
        torch.manual_seed(0)
        model = bench.build_model(0, RANK, 'bf16', C_STEP)
        if kind != 'linear':
            model.id_head, model.id_scale, model.id_margin = margin_args('margin_ce_times', kind, None, None)
        if inputs is None:
            batch = synthetic_batch(Pi, K, model.arch, seed=1000, num_classes=C_STEP)
            tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
            inputs = ({m: t.cuda() for m, t in batch['images'].items()}, {k: v.cuda() for k, v in tok.items()},
                      batch['modality_mask'], batch['person_id'].cuda())
        dp = DataParallel(model)
        groups = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in model.get_learnable_params()]
        d = StepDriver(dp, FusedAdamW([g for g in groups if g['params']], weight_decay=1e-4), accum_steps=1, adaptive_clip=True, dp=dp)
        steppers[kind] = lambda d=d: d.step(*inputs)['total_loss'].detach()
    for kind, st in steppers.items():
        for _ in range(warmup):
            last[kind] = st()
    torch.cuda.synchronize()
    samples = {kind: [] for kind in steppers}
    for _ in range(rounds):
        for kind, st in steppers.items():
            samples[kind].append(window(st, steps) / 1e3)
    rec = dict(mode='step', P=Pi, K=K, rank=RANK, C=C_STEP, steps_per_window=steps, rounds=rounds)
    for kind, v in samples.items():
        rec[kind + '_ms'] = [round(t, 3) for t in v]
        rec[kind + '_median_ms'] = round(median(v), 3)
        rec[kind + '_warmup_loss'] = float(last[kind])
    rec['added_ms_median'] = round(rec['cosface_median_ms'] - rec['linear_median_ms'], 3)
    print(json.dumps(rec), flush=True)
    with open(out, 'a') as f:
        f.write(f'\n## Eager config-2 step (P = {Pi}, K = {K}, rank {RANK}, C = {C_STEP}); ms per step, median of {rounds} alternating windows '
                f'of {steps} steps\n\n| id_head | ms (median) | windows |\n|---|---|---|\n')
        for kind in samples:
            f.write(f"| {kind} | {rec[kind + '_median_ms']} | {rec[kind + '_ms']} |\n")
        f.write(f"\ncosface - linear: {rec['added_ms_median']} ms\n")


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('margin_ce_times.py needs the GPU: nothing is measured without one')
    mode = sys.argv[1] if len(sys.argv) > 1 else 'head'
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'margin_ce_summary.md')
    {'head': head, 'step': step}[mode](out)
