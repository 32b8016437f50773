"""Hybrid memory loss (csrc/hybrid_nce.hip; SpCL): what it costs.

    python tools/hybrid_nce_times.py [--step]
        host time per forward (without and with the gradient pass), per update (instances + refresh) and per backward through the
        ops wrappers at (R, M, C, D) = (64, 16384, 3000, 512) and (320, 200000, 40000, 512), and at the second shape again with one
        class of 16384 members touched by the batch (the refresh's worst case: one workgroup gathers 16384 rows), against SpCL's own
        form written with torch ops in the same process -- normalize, x @ V.T over all M instances, index_add_ by class, divided by
        the counts, a masked softmax (autograd for the backward), an index loop for the update -- in alternating windows.
        --step: also the training step of bench.py's config 2 (P = 16, K = 4, rank 16) with the term off and on.

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

# (R, M, C, D, members of the one big class the batch touches: 0 = none)
SHAPES = ((64, 16384, 3000, 512, 0), (320, 200000, 40000, 512, 0), (320, 200000, 40000, 512, 16384))
TAU, MOMENTUM = 0.05, 0.2


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


def spcl_loss(x, V, cls, counts, index, tau):
    """SpCL's HybridMemory.forward, literally: similarities to ALL instances, aggregated by class, a masked softmax."""
    sim = (F.normalize(x, dim=1, eps=1e-12) @ V.T / tau).T                                      # [M, R]
    agg = torch.zeros(counts.shape[0], x.shape[0], device=x.device).index_add_(0, cls, sim)
    mask = (counts > 0).float().unsqueeze(1)
    agg = (agg / (mask * counts.unsqueeze(1) + (1 - mask))).T                                   # [R, C]
    e = torch.exp(agg) * mask.T
    p = e / (e.sum(dim=1, keepdim=True) + 1e-6)
    return F.nll_loss(torch.log(p + 1e-6), cls[index])


def spcl_update(V, xhat, index, momentum):
    """SpCL's HM.backward, literally: an index loop over the rows."""
    for r, i in enumerate(index.tolist()):
        V[i] = momentum * V[i] + (1 - momentum) * xhat[r]
        V[i] /= V[i].norm()


def measure(R, M, C, D, big, reps, rounds, update_reps):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.losses import HybridMemory
    g = torch.Generator().manual_seed(R + C)
    # classes: `big` instances in class 0 (when asked), about half of the remaining classes singletons, the rest spread evenly
    cls = torch.empty(M, dtype=torch.int64)
    first = 1 if big else 0
    cls[:big] = 0
    n_single = (C - first) // 2
    cls[big:big + n_single] = torch.arange(first, first + n_single)
    rest = M - big - n_single
    cls[big + n_single:] = first + n_single + torch.arange(rest) % (C - first - n_single)
    perm = torch.randperm(M, generator=g)
    cls = cls[perm].cuda()
    mem = HybridMemory.from_labels(torch.randn(M, D, generator=g).cuda(), cls)
    index = torch.randperm(M, generator=g)[:R].cuda()
    if big:
        index[0] = int((cls == 0).nonzero()[0])           # one row of the batch sits in the big class
    x = (mem.instances[index] + 0.5 * torch.randn(R, D, generator=g).cuda() / D ** 0.5).contiguous()
    labels = mem.classes_of(index).contiguous()
    ws = torch.empty(ops.cluster_nce_ws_floats(1, R, D, C), device='cuda')
    row_loss, tcos, res = torch.empty(R, device='cuda'), torch.empty(R, device='cuda'), torch.empty(2, device='cuda')
    dloss, dx = torch.ones(1, device='cuda'), torch.empty(R, D, device='cuda')
    theirs, counts = mem.instances.clone(), mem.counts.float()
    xa = x.clone().requires_grad_(True)
    state = {}

    def torch_fwd():
        state['loss'] = spcl_loss(xa, theirs, cls, counts, index, TAU)

    def torch_fwd_nograd():
        with torch.no_grad():
            spcl_loss(x, theirs, cls, counts, index, TAU)

    def torch_fwd_bwd():
        xa.grad = None
        torch_fwd()
        state['loss'].backward()

    def update():
        ops.hybrid_update_instances(index, None, row_loss, ws, mem.instances, MOMENTUM)
        ops.hybrid_refresh_classes(labels, None, row_loss, mem.instances, mem.order, mem.offsets, mem.table)

    calls = {
        'fwd_nograd': lambda: ops.cluster_nce_fwd(x, labels, None, mem.table, TAU, False, ws, row_loss, tcos, res),
        'fwd_grad': lambda: ops.cluster_nce_fwd(x, labels, None, mem.table, TAU, True, ws, row_loss, tcos, res),
        'bwd': lambda: ops.cluster_nce_bwd(ws, res, dloss, dx),
        'update': update,
        'update_instances': lambda: ops.hybrid_update_instances(index, None, row_loss, ws, mem.instances, MOMENTUM),
        'refresh_classes': lambda: ops.hybrid_refresh_classes(labels, None, row_loss, mem.instances, mem.order, mem.offsets, mem.table),
        'torch_fwd_nograd': torch_fwd_nograd,
        'torch_fwd': torch_fwd,
        'torch_fwd_bwd': torch_fwd_bwd,
    }
    slow = {'torch_update': lambda: spcl_update(theirs, F.normalize(x, dim=1), index, MOMENTUM)}
    rec = dict(R=R, M=M, C=C, D=D, big_class=big, largest_class=int(mem.counts.max()), touched_classes=int(labels.unique().numel()),
               tau=TAU, momentum=MOMENTUM, reps=reps, update_reps=update_reps, rounds=rounds, plan=list(ops.cluster_nce_plan(R, C, D)),
               entries_mb=round(M * D * 4 / 1e6, 1), table_mb=round(C * D * 4 / 1e6, 2))
    # the two losses and gradients from the same state, before anything moves
    ops.cluster_nce_fwd(x, labels, None, mem.table, TAU, True, ws, row_loss, tcos, res)
    ops.cluster_nce_bwd(ws, res, dloss, dx)
    torch_fwd_bwd()
    torch.cuda.synchronize()
    rec['loss_difference'] = abs(float(res[0]) - float(state['loss'].detach()))      # (SpCL's two 1e-6 guards are part of its form)
    rec['dx_max_difference'] = float((dx - xa.grad).abs().max())
    rec['dx_max'] = float(xa.grad.abs().max())
    for fn in list(calls.values()) + list(slow.values()):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    fresh = torch.empty_like(mem.table)
    ops.class_means(mem.instances, mem.order, mem.offsets, fresh)
    rec['table_is_exact_after_updates'] = bool(torch.equal(fresh.view(torch.int32), mem.table.view(torch.int32)))
    samples = {k: [] for k in list(calls) + list(slow)}
    for _ in range(rounds):                               # alternating windows: drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, reps))
        for k, fn in slow.items():
            samples[k].append(window(fn, update_reps))
    for k, v in samples.items():
        rec[k + '_us_median'] = round(median(v), 1); rec[k + '_us_min'] = round(min(v), 1)
    rec['torch_bwd_us_median'] = round(rec['torch_fwd_bwd_us_median'] - rec['torch_fwd_us_median'], 1)
    rec['class_means_us_median'] = round(median([window(lambda: ops.class_means(mem.instances, mem.order, mem.offsets, fresh), 5) for _ in range(rounds)]), 1)
    print(json.dumps(rec), flush=True)


def step_times(steps, warmup, rounds):
    """The training step of bench.py's config 2 (one GPU, P = 16 identities x K = 4, rank-16 adapters, synthetic batch) through
    StepDriver, eagerly: the hybrid term off, and on over a memory of 16384 instances in 3000 classes ('bn' source)."""
    from prcv2025reid_amd.config import TrainingConfig, arch_of
    from prcv2025reid_amd.losses import HybridMemory
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    from prcv2025reid_amd.synthetic import synthetic_batch
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    P, K, M, C = 16, 4, 16384, 3000
    out = {}
    g = torch.Generator().manual_seed(3)
    for name, weight in (('off', 0.0), ('on', 1.0)):
        cfg = TrainingConfig(device='cuda:0', mer_lora_rank=16, contrastive_weight=0.1, seed=0, init='seeded', hybrid_nce_weight=weight)
        arch = arch_of(cfg)
        model = CLIPBasedMultiModalReIDModel(cfg)
        model.set_num_classes(C)
        apply_reference_freeze(model)
        model.set_epoch(2); model.train()
        batch = synthetic_batch(P, K, arch, seed=9, mask_drop=0.3, num_classes=C)
        images = {m: t.cuda() for m, t in batch['images'].items()}
        tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
        tok = {k: v.cuda() for k, v in tok.items()}
        labels = batch['person_id'].cuda()
        if weight > 0:
            D = model(images=images, texts=batch['texts'], modality_masks=batch['modality_mask'])['bn_features'].shape[1]
            cls = torch.cat([torch.arange(C), torch.randint(0, C // 2, (M - C,), generator=g)])[torch.randperm(M, generator=g)]
            model.set_hybrid_memory(HybridMemory.from_labels(torch.randn(M, D, generator=g).cuda(), cls.cuda()))
            labels = torch.randperm(M, generator=g)[:P * K].cuda()       # dataset instance indices
        gs = [dict(params=[p for p in gr['params'] if p.requires_grad], lr=gr['lr'], name=gr['name']) for gr in model.get_learnable_params()]
        driver = StepDriver(model, FusedAdamW(gs, weight_decay=1e-4))
        for _ in range(warmup):
            L = driver.step(images, tok, dict(batch['modality_mask']), labels)
        torch.cuda.synchronize()
        v = [window(lambda: driver.step(images, tok, dict(batch['modality_mask']), labels), steps) / 1e3 for _ in range(rounds)]
        out[name] = dict(step_ms_median=round(median(v), 3), step_ms_min=round(min(v), 3), step_ms_max=round(max(v), 3),
                         total_loss=float(L['total_loss'].detach()))
        if weight > 0:
            out[name]['hybrid_nce_loss'] = float(L['hybrid_nce_loss'].detach())
        del model, driver
        torch.cuda.empty_cache()
    print(json.dumps(dict(step='config 2 (P=16, K=4, rank 16), StepDriver, eager', steps=steps, warmup=warmup, rounds=rounds, M=M, C=C, **out)), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('hybrid_nce_times.py needs the GPU: nothing is measured without one')
    for R, M, C, D, big in SHAPES:
        measure(R, M, C, D, big, reps=50, rounds=5, update_reps=3)
    if '--step' in sys.argv:
        step_times(steps=10, warmup=5, rounds=5)
