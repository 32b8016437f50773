"""Weight EMA of the fused optimizer (csrc/ema.hip): what it costs.

    python tools/ema_times.py launch   reid_ema_update and reid_ema_swap alone against the reid_opt_adamw launch, each on the table of
                                       the benchmark's trainable set (BASELINE config 2: P = 16, K = 4, LoRA rank 8, bench.py's model),
                                       alternating windows in one process.  Exits non-zero when the update's median is above the AdamW
                                       launch's: it moves 12 bytes per element against 32, so that would be a wrong kernel, not a slow one
    python tools/ema_times.py step     the config-2 training step, eager StepDriver and GraphedStep, with ema_decay None (nothing of
                                       this file's subject is allocated or launched: the parent's step) against 0.9999 with the BN-neck's
                                       running statistics listed, alternating windows on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

Pi, K, C, RANK = 16, 4, 400, 8
DECAY = 0.9999


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


def make_optimizer(model, ema: bool):
    from prcv2025reid_amd.trainer import FusedAdamW
    groups = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in model.get_learnable_params()]
    groups = [g for g in groups if g['params']]
    kw = dict(ema_decay=DECAY, ema_buffers=[model.bn_neck.bn.running_mean, model.bn_neck.bn.running_var]) if ema else {}
    return FusedAdamW(groups, weight_decay=1e-4, **kw)


def launch(reps=200, rounds=9):
    import bench
    from prcv2025reid_amd._lib import check, lib, ptr, stream_ptr
    model = bench.build_model(0, RANK, 'bf16', C)
    opt = make_optimizer(model, True)
    n, ne = len(opt.params), len(opt.ema_shadow)
    elems = sum(p.numel() for p in opt.params)
    coef = opt.state.data_ptr() + 8
    opt.state[2] = 1.0                                # clip coefficient the AdamW launch reads; the gradients are zero

    def adamw():
        check(lib().reid_opt_adamw(ptr(opt._table), n, coef, 0.9, 0.999, 1e-8, 1000, 1, ptr(opt.state), stream_ptr()))

    def update():
        check(lib().reid_ema_update(ptr(opt._ema_table), ne, DECAY, 1, 1000, ptr(opt.state), stream_ptr()))

    def update_counter():                             # t from state[16]: the form a captured graph replays
        check(lib().reid_ema_update(ptr(opt._ema_table), ne, DECAY, 1, 0, ptr(opt.state), stream_ptr()))

    def swap():
        check(lib().reid_ema_swap(ptr(opt._ema_table), ne, stream_ptr()))

    calls = dict(adamw=adamw, ema_update=update, ema_update_counter=update_counter, ema_swap=swap)
    opt.state[16] = 1000.0
    for fn in calls.values():
        for _ in range(10):                           # (an even number: the swaps cancel)
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in calls}
    for _ in range(rounds):                           # alternating windows: drift hits every launch alike
        for k, fn in calls.items():
            samples[k].append(window(fn, reps))
    rec = dict(mode='launch', P=Pi, K=K, rank=RANK, adamw_entries=n, ema_entries=ne, trainable_elements=elems,
               ema_elements=sum(s.numel() for s in opt.ema_shadow), reps=reps, rounds=rounds)
    for k, v in samples.items():
        rec[k + '_us_median'] = round(median(v), 2); rec[k + '_us_min'] = round(min(v), 2)
    rec['update_bytes_MB'] = round(12 * rec['ema_elements'] / 1e6, 1)
    rec['update_GBps_median'] = round(12 * rec['ema_elements'] / rec['ema_update_us_median'] / 1e3, 1)
    rec['update_not_slower_than_adamw'] = rec['ema_update_us_median'] <= rec['adamw_us_median']
    print(json.dumps(rec), flush=True)
    if not rec['update_not_slower_than_adamw']:
        raise SystemExit('reid_ema_update takes longer than reid_opt_adamw on the same table: the kernel is wrong')


def step(steps=10, rounds=5, warmup=3):
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    from prcv2025reid_amd.trainer import StepDriver, GraphedStep
    inputs = None
    rec = dict(mode='step', P=Pi, K=K, rank=RANK, ema_decay=DECAY, steps_per_window=steps, rounds=rounds)
    # Fresh models per kind, as bench.py builds them: a GraphedStep is captured on a driver that has not stepped eagerly before (a
    # loss dictionary kept from an eager step on another stream keeps its AccumulateGrad nodes, and their stream, alive into the capture).
    for kind in ('eager', 'graph'):
        steppers, opts = {}, {}
        for ema in (False, True):
            torch.manual_seed(0)
            model = bench.build_model(0, RANK, 'bf16', C)
            if inputs is None:
                batch = synthetic_batch(Pi, K, model.arch, seed=1000, num_classes=C)
                tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
                inputs = ({m: t.cuda() for m, t in batch['images'].items()}, {k: v.cuda() for k, v in tok.items()},
                          batch['modality_mask'], batch['person_id'].cuda())
            dp = DataParallel(model)
            opts[ema] = make_optimizer(model, ema)
            d = StepDriver(dp, opts[ema], accum_steps=1, adaptive_clip=True, dp=dp)
            if kind == 'graph':
                d = GraphedStep(d, *inputs, warmup=1)
            steppers[ema] = lambda d=d: d.step(*inputs)['total_loss'].detach()
        last = {}
        for ema, st in steppers.items():
            for _ in range(warmup):
                last[ema] = st()
        torch.cuda.synchronize()
        samples = {ema: [] for ema in steppers}
        for _ in range(rounds):
            for ema, st in steppers.items():
                samples[ema].append(window(st, steps) / 1e3)
        for ema, v in samples.items():
            name = f'{kind}_{"ema" if ema else "off"}'
            rec[name + '_ms'] = [round(t, 3) for t in v]
            rec[name + '_median_ms'] = round(median(v), 3)
            rec[name + '_warmup_loss'] = float(last[ema])
        rec[f'{kind}_added_ms_median'] = round(rec[f'{kind}_ema_median_ms'] - rec[f'{kind}_off_median_ms'], 3)
        rec[f'{kind}_ema_updates'], rec[f'{kind}_steps_taken'] = opts[True].ema_num_updates, opts[True].step_count
        print(json.dumps(dict(mode='step-' + kind, off_median_ms=rec[f'{kind}_off_median_ms'], ema_median_ms=rec[f'{kind}_ema_median_ms'])),
              flush=True)
        del steppers, opts, d, dp, model
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('ema_times.py needs the GPU: nothing is measured without one')
    {'launch': launch, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'launch']()
