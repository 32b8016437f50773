"""Cross-modal Smooth-AP (csrc/smooth_ap.hip): what it costs.

    python tools/smooth_ap_times.py kernels   forward without gradients, forward with gradients and backward at (P, N, G, D) =
                                              (4, 64, 64, 512) in the batch and (4, 64, 4096, 512), (4, 64, 8192, 512) over a full ring,
                                              against the same loss written with torch ops (normalise, matmul, a [chunk, positives, G]
                                              sigmoid tensor per chunk of 16 anchors so that it fits, autograd) on the same GPU in the
                                              same process
    python tools/smooth_ap_times.py step      the config-2 training step (P = 16, K = 4, rank 8: bench.py's headline, eager StepDriver) with
                                              smooth_ap_weight 0 (nothing of this file's subject is allocated or launched: the parent's
                                              step) against 0.5 in the batch and 0.5 over a ring of 4096, alternating blocks on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

TAU = 0.01
P, N, D = 4, 64, 512
SHAPES = [('batch', 64), ('ring', 4096), ('ring', 8192)]
IDS = 16                                  # identities of a batch of 64: 4 instances each, as the sampler draws them
CHUNK = 16


def torch_direction(a, a_lab, c, c_lab, c_valid, pmax, tau=TAU):
    """mean over the active anchors of 1 - AP, anchors a [A, D] and gallery c [G, D] unit rows: the hand-written version.  ``pmax``: the
    largest number of positives of an anchor (known to the caller: no host read-back here)."""
    s = a @ c.T
    pos = (a_lab[:, None] == c_lab[None, :]) & c_valid[None, :]
    npos = pos.sum(1)
    active = (npos > 0) & (npos < c_valid.sum())
    idx = pos.float().topk(pmax, dim=1).indices                                    # the positives first
    pmask = pos.gather(1, idx)
    aps = []
    for c0 in range(0, a.shape[0], CHUNK):
        sc, ic = s[c0:c0 + CHUNK], idx[c0:c0 + CHUNK]
        d = (sc[:, None, :] - sc.gather(1, ic)[:, :, None]) / tau                  # [chunk, pmax, G]
        sig = (torch.sigmoid(d) * c_valid[None, None, :]).scatter(2, ic[:, :, None], 0.0)
        R, Rp = 1 + sig.sum(2), 1 + (sig * pos[c0:c0 + CHUNK, None, :]).sum(2)
        aps.append(((Rp / R) * pmask[c0:c0 + CHUNK]).sum(1) / npos[c0:c0 + CHUNK].clamp(min=1))
    ap = torch.cat(aps)
    return ((1 - ap) * active).sum() / active.sum().clamp(min=1)


def torch_smooth_ap(q, g, lab, ring, pmax):
    """L [P] of the batch form (ring None) or of the ring form (rows, labels, valid), the ring a constant."""
    qh = torch.nn.functional.normalize(q, dim=-1); gh = torch.nn.functional.normalize(g, dim=-1)
    out = []
    for p in range(q.shape[0]):
        if ring is None:
            on = torch.ones(lab.shape[0], dtype=torch.bool, device=q.device)
            L = torch_direction(qh[p], lab, gh, lab, on, pmax) + torch_direction(gh, lab, qh[p], lab, on, pmax)
        else:
            rows, rl, rv = ring
            L = torch_direction(qh[p], lab, rows[0], rl, rv[0] != 0, pmax) + torch_direction(gh, lab, rows[p + 1], rl, rv[p + 1] != 0, pmax)
        out.append(0.5 * L)
    return torch.stack(out)


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def stream_step(step, device='cuda'):
    """Batch ``step`` of a stream of identities: q [P, N, D], g [N, D] around per-identity directions, labels [N] (4 instances each)."""
    gen = torch.Generator().manual_seed(1000 + step)
    ids = torch.randperm(256, generator=gen)[:IDS]
    centres = torch.nn.functional.normalize(torch.randn(256, D, generator=torch.Generator().manual_seed(5)), dim=1)
    lab = ids.repeat_interleave(N // IDS)
    q = centres[lab][None] + 0.08 * torch.randn(P, N, D, generator=gen)
    g = centres[lab] + 0.08 * torch.randn(N, D, generator=gen)
    return q.to(device), g.to(device), lab.to(device)


def make_calls(form, G):
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.losses import CrossBatchMemory, SmoothAPFn, EPS
    memory = ring = None
    if form == 'ring':
        memory = CrossBatchMemory(G, P + 1, D, 'cuda')
        for s in range(1, G // N + 1):                            # a full ring of unit rows, the last batch the one that ranks it
            q, g, lab = stream_step(s)
            ops.xbm_enqueue(q.reshape(P * N, D), g, lab, None, None, True, EPS, memory.rows, memory.labels, memory.valid, memory.cursor, P=P)
        ring = (memory.rows, memory.labels, memory.valid)
        pmax = int((memory.labels[None, :] == lab[:, None]).sum(1).max())
    else:
        q, g, lab = stream_step(1)
        pmax = N // IDS
    one = torch.ones((), device='cuda')
    qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    qb, gb = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    state = {}

    def hip(with_grad):
        return SmoothAPFn.apply(qa, ga, lab, lab, None, None, memory, TAU, True, False, with_grad)[0].sum()

    def hip_fwd_nograd():
        state['hip0'] = hip(False)

    def hip_fwd():
        state['hip'] = hip(True)

    def hip_bwd():
        qa.grad = ga.grad = None
        state['hip'].backward(one, retain_graph=True)

    def torch_fwd_nograd():
        with torch.no_grad():
            state['torch0'] = torch_smooth_ap(qb, gb, lab, ring, pmax).sum()

    def torch_fwd():
        state['torch'] = torch_smooth_ap(qb, gb, lab, ring, pmax).sum()

    def torch_bwd():
        qb.grad = gb.grad = None
        state['torch'].backward(one, retain_graph=True)

    calls = dict(hip_fwd_nograd=hip_fwd_nograd, hip_fwd=hip_fwd, hip_bwd=hip_bwd, torch_fwd_nograd=torch_fwd_nograd, torch_fwd=torch_fwd,
                 torch_bwd=torch_bwd)
    return calls, state, (qa, qb), pmax


def kernels(rounds=5):
    for form, G in SHAPES:
        reps = 100 if G == 64 else 10
        calls, state, (qa, qb), pmax = make_calls(form, G)
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        rec = dict(mode='kernels', form=form, P=P, N=N, G=G, D=D, tau=TAU, positives_max=pmax, reps=reps, rounds=rounds,
                   loss_sum_hip=float(state['hip'].detach()), loss_sum_torch=float(state['torch'].detach()),
                   dq_max_abs_diff=float((qa.grad - qb.grad).abs().max()), dq_max_abs=float(qa.grad.abs().max()))
        samples = {k: [] for k in calls}
        for _ in range(rounds):                              # alternating windows: drift hits every variant alike
            for k, fn in calls.items():
                samples[k].append(window(fn, reps))
        for k, v in samples.items():
            v.sort()
            rec[k + '_us_median'] = round(v[len(v) // 2], 1); rec[k + '_us_min'] = round(v[0], 1); rec[k + '_us_max'] = round(v[-1], 1)
        print(json.dumps(rec), flush=True)


def step(steps=10, rounds=6, warmup=3):
    import argparse
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    Pi, K, C = 16, 4, 400
    args = argparse.Namespace(optimizer='fused', accum=1, graph='off')
    steppers = {}
    for name, w, size in (('off', 0.0, 0), ('batch', 0.5, 0), ('ring4096', 0.5, 4096)):
        torch.manual_seed(0)
        model = bench.build_model(0, 8, 'bf16', C)
        model.smooth_ap_weight, model.smooth_ap_size = w, size
        batch = synthetic_batch(Pi, K, model.arch, seed=1000, num_classes=C)
        images = {m: t.cuda() for m, t in batch['images'].items()}
        tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
        tokens = {k: v.cuda() for k, v in tok.items()}
        st, _, _ = bench.make_stepper(model, DataParallel(model), args, images, tokens, batch['modality_mask'], batch['person_id'].cuda(), 1)
        steppers[name] = st
        for _ in range(size // (Pi * K) + warmup):            # (the ring is full before anything is timed)
            L = st()
        torch.cuda.synchronize()
        print(json.dumps(dict(mode='step-warmup', variant=name, keys=sorted(L), total_loss=float(L['total_loss'].detach()),
                              smooth_ap_loss=float(L['smooth_ap_loss'].detach()) if 'smooth_ap_loss' in L else None,
                              active=int(L['smooth_ap_active_cnt']) if 'smooth_ap_active_cnt' in L else None,
                              filled=int(model.smooth_ap_memory.filled) if model.smooth_ap_memory is not None else None)), flush=True)
    samples = {k: [] for k in steppers}
    for _ in range(rounds):
        for k, st in steppers.items():
            samples[k].append(window(st, steps) / 1e3)
    rec = dict(mode='step', P=Pi, K=K, rank=8, steps_per_window=steps, rounds=rounds)
    for k, v in samples.items():
        rec[f'ms_per_step_{k}'] = [round(t, 3) for t in v]
        rec[f'median_ms_{k}'] = round(sorted(v)[len(v) // 2], 3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('smooth_ap_times.py needs the GPU: nothing is measured without one')
    {'kernels': kernels, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
