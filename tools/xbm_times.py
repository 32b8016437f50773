"""Cross-batch memory for the cross-modal triplet loss (csrc/xbm.hip): what it costs.

    python tools/xbm_times.py kernels   enqueue, forward (mining the full ring) and backward alone at P = 4, N = 64, D = 512 for
                                        M = 1024, 4096 and 8192, against the same loss written with torch ops (normalise, cdist in
                                        the difference form, masked max / min against the ring as a constant, autograd) on the same
                                        GPU in the same process
    python tools/xbm_times.py step      the config-2 training step (P = 16, K = 4, rank 8: bench.py's headline, eager StepDriver) with
                                        xbm_weight 0 (nothing of this file's subject is allocated or launched: the parent's step)
                                        against 0.5 with xbm_size 4096, alternating blocks on one device

Times are HIP events around windows that end in a synchronise; every line printed is one JSON record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

MARGIN = 0.3
P, N, D = 4, 64, 512
SIZES = [1024, 4096, 8192]


def torch_xbm(q, g, lab, rows, mem_labels, mem_valid, margin=MARGIN):
    """The hand-written version for data in which every anchor has a positive and a negative: L [P]; the ring is a constant."""
    qh = torch.nn.functional.normalize(q, dim=-1); gh = torch.nn.functional.normalize(g, dim=-1)
    same = (lab[:, None] == mem_labels[None, :])[None]                             # [1, N, M]
    dq = torch.cdist(qh, rows[0][None].expand(q.shape[0], -1, -1), compute_mode='donot_use_mm_for_euclid_dist')      # [P, N, M]
    dg = torch.cdist(gh[None].expand(q.shape[0], -1, -1), rows[1:], compute_mode='donot_use_mm_for_euclid_dist')     # [P, N, M]
    out = []
    for d, ok in ((dq, mem_valid[0][None, None, :] != 0), (dg, mem_valid[1:, None, :] != 0)):
        pos = d.masked_fill(~(same & ok), float('-inf')); neg = d.masked_fill(~(~same & ok), float('inf'))
        out.append((pos.max(2).values - neg.min(2).values + margin).clamp(min=0).mean(1))
    return 0.5 * (out[0] + out[1])


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def make_calls(M):
    import xbm_ref as X
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.losses import CrossBatchMemory, XbmTripletFn, EPS
    memory = CrossBatchMemory(M, P + 1, D, 'cuda')
    for s in range(1, M // N + 1):                            # a full ring of unit rows, the last batch the one that is mined
        q, g, lab = X.stream_step(P, N, D, 0.0, s, 'cuda')
        ops.xbm_enqueue(q.reshape(P * N, D), g, lab, None, None, True, EPS, memory.rows, memory.labels, memory.valid, memory.cursor, P=P)
    one = torch.ones((), device='cuda')
    qa, ga = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    qb, gb = q.clone().requires_grad_(True), g.clone().requires_grad_(True)
    q2 = q.reshape(P * N, D).contiguous()
    state = {}

    def hip_enqueue():
        ops.xbm_enqueue(q2, g, lab, None, None, True, EPS, memory.rows, memory.labels, memory.valid, memory.cursor, P=P)

    def hip_fwd():
        state['hip'] = XbmTripletFn.apply(qa, ga, lab, None, None, memory, MARGIN, True, False)[0].sum()

    def hip_bwd():
        qa.grad = ga.grad = None
        state['hip'].backward(one, retain_graph=True)

    def torch_fwd():
        state['torch'] = torch_xbm(qb, gb, lab, memory.rows, memory.labels, memory.valid).sum()

    def torch_bwd():
        qb.grad = gb.grad = None
        state['torch'].backward(one, retain_graph=True)

    # forward and backward first: the timed enqueues then refile the last batch (the ring stays full of unit rows)
    return dict(hip_fwd=hip_fwd, hip_bwd=hip_bwd, torch_fwd=torch_fwd, torch_bwd=torch_bwd, hip_enqueue=hip_enqueue), state, (qa, qb)


def kernels(reps=300, rounds=7):
    for M in SIZES:
        calls, state, (qa, qb) = make_calls(M)
        for k in ('hip_fwd', 'hip_bwd', 'torch_fwd', 'torch_bwd'):
            for _ in range(5):
                calls[k]()
        torch.cuda.synchronize()
        rec = dict(mode='kernels', P=P, N=N, D=D, M=M, margin=MARGIN, reps=reps, rounds=rounds,
                   loss_sum_hip=float(state['hip'].detach()), loss_sum_torch=float(state['torch'].detach()),
                   dq_max_abs_diff=float((qa.grad - qb.grad).abs().max()), dq_max_abs=float(qa.grad.abs().max()))
        for _ in range(5):
            calls['hip_enqueue']()
        samples = {k: [] for k in calls}
        for _ in range(rounds):                              # alternating windows: drift hits every variant alike
            for k, fn in calls.items():
                samples[k].append(window(fn, reps))
        for k, v in samples.items():
            v.sort()
            rec[k + '_us_median'] = round(v[len(v) // 2], 2); rec[k + '_us_min'] = round(v[0], 2)
        print(json.dumps(rec), flush=True)


def step(steps=10, rounds=6, warmup=3):
    import argparse
    import bench
    from prcv2025reid_amd.parallel import DataParallel
    from prcv2025reid_amd.synthetic import synthetic_batch
    Pi, K, C = 16, 4, 400
    args = argparse.Namespace(optimizer='fused', accum=1, graph='off')
    steppers = {}
    for w in (0.0, 0.5):
        torch.manual_seed(0)
        model = bench.build_model(0, 8, 'bf16', C)
        model.xbm_weight, model.xbm_size = w, 4096
        model.set_epoch(max(model.current_epoch, model.xbm_start_epoch))
        batch = synthetic_batch(Pi, K, model.arch, seed=1000, num_classes=C)
        images = {m: t.cuda() for m, t in batch['images'].items()}
        tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
        tokens = {k: v.cuda() for k, v in tok.items()}
        st, _, _ = bench.make_stepper(model, DataParallel(model), args, images, tokens, batch['modality_mask'], batch['person_id'].cuda(), 1)
        steppers[w] = st
        for _ in range(warmup if w == 0.0 else 4096 // (Pi * K) + warmup):     # (the ring is full before anything is timed)
            L = st()
        torch.cuda.synchronize()
        print(json.dumps(dict(mode='step-warmup', xbm_weight=w, keys=sorted(L), total_loss=float(L['total_loss'].detach()),
                              xbm_loss=float(L['xbm_loss'].detach()) if 'xbm_loss' in L else None,
                              active=int(L['xbm_active_cnt']) if 'xbm_active_cnt' in L else None,
                              filled=int(model.xbm_memory.filled) if model.xbm_memory is not None else None)), flush=True)
    samples = {w: [] for w in steppers}
    for _ in range(rounds):
        for w, st in steppers.items():
            samples[w].append(window(st, steps) / 1e3)
    rec = dict(mode='step', P=Pi, K=K, rank=8, xbm_size=4096, steps_per_window=steps, rounds=rounds)
    for w, v in samples.items():
        rec[f'ms_per_step_w{w}'] = [round(t, 3) for t in v]
        s = sorted(v)
        rec[f'median_ms_w{w}'] = round(s[len(s) // 2], 3)
    rec['added_ms_median'] = round(rec['median_ms_w0.5'] - rec['median_ms_w0.0'], 3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('xbm_times.py needs the GPU: nothing is measured without one')
    {'kernels': kernels, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
