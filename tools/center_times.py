"""Center loss (csrc/center.hip): what it costs.

    python tools/center_times.py launch   forward + centre update + backward through losses.CenterLossFn at N = 64, D = 512, C = 1000 for
                                          S = 1 and S = 5, against the same arithmetic written with torch ops (index_select for the
                                          centres, index_add_ for the per-class sums and counts) through autograd, alternating windows
                                          in one process
    python tools/center_times.py step     the config-2 training step (BASELINE config 2: P = 16, K = 4, LoRA rank 8, bench.py's model),
                                          eager StepDriver, with center_weight 0 (nothing of this file's subject is allocated or
                                          launched: the parent's step) against 5e-4 for both center_source values, alternating windows
                                          on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

Pi, K, C, RANK = 16, 4, 400, 8
N, D, CLASSES, ALPHA = 64, 512, 1000, 0.5


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


def torch_center(x, labels, valid, centers, alpha):
    """The loss and Wen's update with torch ops; returns the loss (the table is updated in place, outside autograd)."""
    S, n, d = x.shape
    lab = labels.repeat(S)
    used = valid.reshape(-1).bool() & (lab >= 0) & (lab < centers.shape[0])
    idx = lab.clamp(0, centers.shape[0] - 1)
    diff = (x.reshape(S * n, d) - centers.index_select(0, idx)) * used[:, None]
    loss = 0.5 * (diff * diff).sum() / used.sum().clamp_min(1)
    with torch.no_grad():
        acc = torch.zeros_like(centers).index_add_(0, idx, -diff)
        cnt = torch.zeros(centers.shape[0], device=x.device).index_add_(0, idx, used.float())
        centers.sub_(alpha * acc / (1.0 + cnt)[:, None])
    return loss


def launch(reps=300, rounds=7):
    from prcv2025reid_amd.losses import CenterLossFn, ClassCenters
    rec = dict(mode='launch', N=N, D=D, C=CLASSES, alpha=ALPHA, reps=reps, rounds=rounds)
    for S in (1, 5):
        g = torch.Generator().manual_seed(S)
        x = torch.randn(S, N, D, generator=g).cuda().requires_grad_(True)
        labels = torch.randint(0, CLASSES, (N // 4,), generator=g).repeat_interleave(4).cuda()      # P x K sampling: 4 rows per identity
        valid = torch.ones(S, N, dtype=torch.uint8, device='cuda')
        ours, theirs = ClassCenters(CLASSES, D, 'cuda'), torch.zeros(CLASSES, D, device='cuda')

        def hip():
            x.grad = None
            CenterLossFn.apply(x, labels, valid, ours, ALPHA, True)[0].backward()

        def torch_ops():
            x.grad = None
            torch_center(x, labels, valid, theirs, ALPHA).backward()

        calls = dict(hip=hip, torch=torch_ops)
        for fn in calls.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        rec[f'S{S}_max_table_difference'] = float((ours.centers - theirs).abs().max())
        samples = {k: [] for k in calls}
        for _ in range(rounds):                           # alternating windows: drift hits both alike
            for k, fn in calls.items():
                samples[k].append(window(fn, reps))
        for k, v in samples.items():
            rec[f'S{S}_{k}_us_median'] = round(median(v), 2); rec[f'S{S}_{k}_us_min'] = round(min(v), 2)
    print(json.dumps(rec), flush=True)


def step(steps=10, rounds=5, warmup=3):
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    inputs = None
    rec = dict(mode='step', P=Pi, K=K, rank=RANK, center_weight=5e-4, steps_per_window=steps, rounds=rounds)
    steppers = {}
    for name, weight, source in (('off', 0.0, 'fused'), ('fused', 5e-4, 'fused'), ('modalities', 5e-4, 'modalities')):
        torch.manual_seed(0)
        model = bench.build_model(0, RANK, 'bf16', C)
        model.center_weight, model.center_source = weight, source
        if inputs is None:
            batch = synthetic_batch(Pi, K, model.arch, seed=1000, num_classes=C)
            tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
            inputs = ({m: t.cuda() for m, t in batch['images'].items()}, {k: v.cuda() for k, v in tok.items()},
                      batch['modality_mask'], batch['person_id'].cuda())
        dp = DataParallel(model)
        groups = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in model.get_learnable_params()]
        d = StepDriver(dp, FusedAdamW([g for g in groups if g['params']], weight_decay=1e-4), accum_steps=1, adaptive_clip=True, dp=dp)
        steppers[name] = lambda d=d: d.step(*inputs)['total_loss'].detach()
    last = {}
    for name, st in steppers.items():
        for _ in range(warmup):
            last[name] = st()
    torch.cuda.synchronize()
    samples = {name: [] for name in steppers}
    for _ in range(rounds):
        for name, st in steppers.items():
            samples[name].append(window(st, steps) / 1e3)
    for name, v in samples.items():
        rec[name + '_ms'] = [round(t, 3) for t in v]
        rec[name + '_median_ms'] = round(median(v), 3)
        rec[name + '_warmup_loss'] = float(last[name])
    for name in ('fused', 'modalities'):
        rec[name + '_added_ms_median'] = round(rec[name + '_median_ms'] - rec['off_median_ms'], 3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('center_times.py needs the GPU: nothing is measured without one')
    {'launch': launch, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'launch']()
