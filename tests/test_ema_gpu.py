"""GPU: the weight EMA (csrc/ema.hip through the C ABI, FusedAdamW / StepDriver / GraphedStep, checkpoint.py) against the float32
numpy restatement of tests/ema_ref.py -- bit for bit: the update is three separately rounded float32 operations."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ema_ref as er
from helpers import GOLDEN, load_case, case_inputs

pytestmark = pytest.mark.gpu


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).ravel()


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def _table(ps, ss):
    from prcv2025reid_amd.trainer import _EmaEntry
    assert all(p.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0 and p.numel() == s.numel() for p, s in zip(ps, ss))
    ents = (_EmaEntry * len(ps))(*[_EmaEntry(p.data_ptr(), s.data_ptr(), p.numel()) for p, s in zip(ps, ss)])
    return torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8).cuda()


# ------------------------------------------------------------------------------------------------------------ 1. kernel bits
@pytest.mark.parametrize('warmup', [True, False])
def test_update_kernel_bits(warmup):
    """n = 1, 3 (scalar tail alone), 4, 5, 1023..1025 (fewer 16-byte groups than threads, an exact multiple), 131079 (a second
    grid-stride pass of 128 x 256 x 4 elements and a tail of 7); three updates, p re-drawn each time; host step and device counter."""
    from prcv2025reid_amd._lib import check, lib, ptr, stream_ptr
    decay = 0.999
    s0, draws = er.kernel_vectors()
    want = [s.copy() for s in s0]
    p_dev = [torch.empty(n, device='cuda') for n in er.KERNEL_SIZES]
    s_host = [torch.from_numpy(s).cuda() for s in s0]          # updated with the host step
    s_cnt = [torch.from_numpy(s).cuda() for s in s0]           # updated with the device counter
    t_host, t_cnt = _table(p_dev, s_host), _table(p_dev, s_cnt)
    state = torch.zeros(lib().reid_opt_state_floats(), device='cuda')
    for r, ps in enumerate(draws):
        t = r + 1
        for d, p in zip(p_dev, ps):
            d.copy_(torch.from_numpy(p))
        state[16] = float(t)                                  # what reid_opt_adamw's tick leaves behind
        check(lib().reid_ema_update(ptr(t_host), len(p_dev), decay, int(warmup), t, None, stream_ptr()))
        check(lib().reid_ema_update(ptr(t_cnt), len(p_dev), decay, int(warmup), 0, ptr(state), stream_ptr()))
        w = er.ema_weight(decay, warmup, t)
        want = [er.ema_update(p, s, w) for p, s in zip(ps, want)]
        for n, a, b, ref, p, d in zip(er.KERNEL_SIZES, s_host, s_cnt, want, ps, p_dev):
            assert same_bits(a, ref), (n, t, 'host step')
            assert same_bits(b, ref), (n, t, 'device counter')
            assert same_bits(a, b), (n, t)
            assert same_bits(d, p), (n, t, 'p is only read')
    assert float(state[16]) == 3.0                            # the state is only read


# ------------------------------------------------------------------------------------------------------------------ 2. swap
def _plant(t):
    v = t.view(torch.int32).view(-1)
    idx = [0, v.numel() // 2, v.numel() - 1]
    for i, word in zip(idx, (0x7fc12345, -2 ** 31, 0x00000001)):      # NaN with a payload, -0.0, the smallest denormal
        v[i] = word


def test_swap_kernel_words():
    from prcv2025reid_amd._lib import check, lib, ptr, stream_ptr
    g = torch.Generator().manual_seed(7)
    ps = [torch.randn(n, generator=g).cuda() for n in er.KERNEL_SIZES]
    ss = [torch.randn(n, generator=g).cuda() for n in er.KERNEL_SIZES]
    for p, s in zip(ps[2:], ss[2:]):
        _plant(p)
    _plant(ss[-1].narrow(0, 5, 1000))
    p0, s0 = [bits(p) for p in ps], [bits(s) for s in ss]
    assert (p0[-1] == 0x7fc12345).any() and (p0[-1] == -2 ** 31).any() and (p0[-1] == 1).any()
    tab = _table(ps, ss)
    check(lib().reid_ema_swap(ptr(tab), len(ps), stream_ptr()))
    for p, s, a, b in zip(ps, ss, p0, s0):
        assert np.array_equal(bits(p), b) and np.array_equal(bits(s), a), p.numel()
    check(lib().reid_ema_swap(ptr(tab), len(ps), stream_ptr()))
    for p, s, a, b in zip(ps, ss, p0, s0):                    # two swaps are the identity
        assert np.array_equal(bits(p), a) and np.array_equal(bits(s), b), p.numel()


def test_swap_ema_versions_and_step_guard():
    from prcv2025reid_amd.trainer import FusedAdamW
    g = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in [(1025,), (7, 5), (3,)]]
    buf = torch.randn(37, generator=g).cuda()
    opt = FusedAdamW([dict(params=params, lr=1e-3, name='x')], ema_decay=0.9, ema_buffers=[buf])
    assert all(same_bits(t, s) for t, s in zip(opt.ema_sources(), opt.ema_shadow))     # the shadows start equal
    for s in opt.ema_shadow:
        s.add_(1.0)
    _plant(params[0].detach()); _plant(opt.ema_shadow[1])
    live = [bits(t) for t in opt.ema_sources()]
    avg = [bits(s) for s in opt.ema_shadow]
    ver = [p._version for p in params]
    opt.swap_ema()
    assert all(p._version > v for p, v in zip(params, ver))
    assert all(np.array_equal(bits(t), a) and np.array_equal(bits(s), l)
               for t, s, l, a in zip(opt.ema_sources(), opt.ema_shadow, live, avg))
    with pytest.raises(RuntimeError, match='swap back'):
        opt.step()
    assert opt.step_count == 0
    ver = [p._version for p in params]
    opt.swap_ema()
    assert all(p._version > v for p, v in zip(params, ver))
    assert all(np.array_equal(bits(t), l) and np.array_equal(bits(s), a)
               for t, s, l, a in zip(opt.ema_sources(), opt.ema_shadow, live, avg))
    with pytest.raises(KeyError):                             # the context manager swaps back on an exception too
        with opt.ema_weights():
            assert np.array_equal(bits(params[1]), avg[1])
            raise KeyError('inside')
    assert all(np.array_equal(bits(t), l) for t, l in zip(opt.ema_sources(), live))
    params[0].detach().nan_to_num_(0.0)                       # (the planted NaN would only make the step's own arithmetic NaN)
    opt.step()
    assert opt.step_count == 1 and opt.ema_num_updates == 1
    with pytest.raises(RuntimeError):
        FusedAdamW([dict(params=params, lr=1e-3, name='x')]).swap_ema()     # no EMA kept


# ------------------------------------------------------------------------------------------------------------- 3. optimizer
@pytest.mark.parametrize('warmup', [True, False])
def test_fused_adamw_ema_chain_and_untouched_step(warmup):
    from prcv2025reid_amd.trainer import FusedAdamW
    shapes = [(70001,), (512, 33), (5,), (64, 16), (3,)]        # the set of test_step_gpu.py::test_fused_adamw_vs_oracle
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(*s, generator=g) for s in shapes]

    def make(**kw):
        ps = [torch.nn.Parameter(p.clone().cuda()) for p in init]
        groups = [dict(params=[ps[0], ps[1]], lr=5e-5, name='mer_loras'),
                  dict(params=[ps[2], ps[4]], lr=3e-3, name='classification_head'),
                  dict(params=[ps[3]], lr=5e-5, name='other_modules', weight_decay=0.0)]
        return ps, FusedAdamW(groups, weight_decay=1e-4, **kw)

    buf = torch.randn(37, generator=g).cuda()
    pa, a = make(ema_decay=0.9, ema_warmup=warmup, ema_buffers=[buf])
    pb, b = make()
    assert b.ema_decay is None and b.ema_shadow == [] and not hasattr(b, '_ema_table')      # off: nothing is allocated
    chain = [t.detach().cpu().numpy().copy() for t in a.ema_sources()]
    for step in range(6):
        scale = float(10.0 ** ((step % 5) - 3))
        grads = [torch.randn(p.shape, generator=g) * scale for p in init]
        if step == 2:
            grads[0][17] = float('nan'); grads[1][3, 4] = float('-inf'); grads[4][2] = float('inf')
        buf.copy_(torch.randn(37, generator=g))                  # what a forward does to a running statistic
        for ps in (pa, pb):
            for p, gr in zip(ps, grads):
                p.grad.copy_(gr)
        a.step(adaptive_clip=True, record_norm=True)
        b.step(adaptive_clip=True, record_norm=True)
        if step == 2:
            assert a.stats()['non_finite'] == 3
        w = er.ema_weight(0.9, warmup, step + 1)
        chain = [er.ema_update(t.detach().cpu().numpy(), s, w) for t, s in zip(a.ema_sources(), chain)]
        for i, (s, ref) in enumerate(zip(a.ema_shadow, chain)):
            assert same_bits(s, ref), (step, i)
        # existing behaviour is untouched: parameters and both moments are those of the twin without an EMA
        for x, y in zip(pa + a.exp_avg + a.exp_avg_sq, pb + b.exp_avg + b.exp_avg_sq):
            assert torch.equal(x.detach(), y.detach()), step
        assert torch.equal(a.state, b.state)
    assert a.ema_num_updates == 6 and b.ema_num_updates == 0
    assert all(np.isfinite(c).all() for c in chain)
    st = a.ema_state()
    assert st['decay'] == 0.9 and st['warmup'] is warmup and st['num_updates'] == 6 and len(st['shadows']) == 6
    for s in a.ema_shadow:
        s.zero_()
    a.load_ema_state(st)
    assert all(same_bits(s, ref) for s, ref in zip(a.ema_shadow, chain)) and a.ema_num_updates == 6


# ------------------------------------------------------------------------------------------------------------ 4. tiny model
def _case():
    z, meta = load_case('tiny_train_frozen')
    cfg, arch, state, batch, tokens = case_inputs(meta)
    images = {m: t.cuda() for m, t in batch['images'].items()}
    labels = batch['person_id'].cuda()
    return meta, state, batch, images, labels


def _groups(model, lr=None):
    return [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'] if lr is None else lr, name=g['name'])
            for g in model.get_learnable_params()]


def test_tiny_model_evaluates_on_the_average():
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    from test_model_gpu import build_model
    meta, state, batch, images, labels = _case()
    masks = {m: t.cuda() for m, t in batch['modality_mask'].items()}
    model = build_model(meta, state, True)
    # every group at 2e-3, no warm-up: after two optimizer steps the average sits 0.81 of the way back to the initial weights, far
    # enough from the live ones to show in 16-bit merged weights
    opt = FusedAdamW(_groups(model, lr=2e-3), weight_decay=1e-4, ema_decay=0.9, ema_warmup=False,
                     ema_buffers=[model.bn_neck.bn.running_mean, model.bn_neck.bn.running_var])
    drv = StepDriver(model, opt, accum_steps=2, adaptive_clip=True)
    drv.start_epoch(2)
    for _ in range(4):
        drv.step(images, batch['texts'], masks, labels)
    assert opt.step_count == 2 and opt.ema_num_updates == 2       # once per optimizer step, not per micro-batch
    model.eval()

    def features():
        with torch.no_grad():
            out = model(images=images, texts=batch['texts'], modality_masks=masks)
        return {'bn': out['bn_features'].clone(), 'fused': out['features'].clone(),
                **{m: t.clone() for m, t in out['raw_modality_features'].items()}}

    old = [bits(t) for t in opt.ema_sources()]
    live = features()
    with opt.ema_weights():
        avg = features()
    assert all(np.array_equal(bits(t), o) for t, o in zip(opt.ema_sources(), old))      # every parameter has its old bits
    again = features()
    assert all(torch.equal(live[k], again[k]) for k in live)                            # ... and the model computes with them again
    with torch.no_grad():                                                               # the same weights, put there by hand
        for t, s in zip(opt.ema_sources(), opt.ema_shadow):
            t.copy_(s)
    hand = features()
    assert all(torch.isfinite(v).all() for v in avg.values())
    for k in avg:
        assert torch.equal(avg[k], hand[k]), k
    # a stale merged-weight cache would have given the live model's features inside the context
    assert not torch.equal(avg['bn'], live['bn']) and not torch.equal(avg['fused'], live['fused'])
    assert any(not torch.equal(avg[m], live[m]) for m in images), 'image-encoder features did not move with the LoRA weights'


# ------------------------------------------------------------------------------------------------------------------ 5. graph
def test_graphed_step_replays_the_ema():
    """Three replays: the shadows follow the ema_ref chain over parameter snapshots, continued from the shadows read right after
    construction (whose warm-up steps advanced them).  Two swaps between replays change nothing: every bit of the optimizer's
    state is what it was, the next replay continues the chain, and it lands where a twin that never swapped lands."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_model_gpu import build_model
    meta, state, batch, images, labels = _case()
    masks = dict(batch['modality_mask'])

    init = {}                                                      # the trainable tensors before any step (the same for both runs)

    def make():
        m = build_model(meta, state, True)
        opt = FusedAdamW(_groups(m), weight_decay=1e-4, ema_decay=0.9)
        tok = m.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
        tok = {k: v.cuda() for k, v in tok.items()}
        init.update({k: p.detach().clone() for k, p in m.named_parameters() if p.requires_grad})
        return m, opt, tok, GraphedStep(StepDriver(m, opt), images, tok, masks, labels, warmup=2)

    def everything(opt):
        return [bits(t) for t in opt.ema_sources() + opt.ema_shadow + opt.exp_avg + opt.exp_avg_sq + [opt.state]]

    ma, a, tok, ga = make()
    torch.cuda.synchronize()
    assert a.step_count == 2 and a.ema_num_updates == 2
    chain = [s.detach().cpu().numpy().copy() for s in a.ema_shadow]
    assert any(not same_bits(t, s) for t, s in zip(a.ema_sources(), a.ema_shadow))      # the warm-up steps moved them apart

    def replay_and_check(t):
        nonlocal chain
        ga.step(images, tok, masks, labels)
        torch.cuda.synchronize()
        w = er.ema_weight(0.9, True, t)
        chain = [er.ema_update(p.detach().cpu().numpy(), s, w) for p, s in zip(a.ema_sources(), chain)]
        for i, (s, ref) in enumerate(zip(a.ema_shadow, chain)):
            assert same_bits(s, ref), (t, i)

    for t in (3, 4, 5):
        replay_and_check(t)
    assert a.step_count == 5 and a.ema_num_updates == 5
    before = everything(a)
    a.swap_ema()
    assert not np.array_equal(bits(a.params[0]), before[0])
    a.swap_ema()
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(everything(a), before))
    replay_and_check(6)                                            # the captured pointers are still the right ones

    mb, b, tok_b, gb = make()                                      # the twin: six steps, no swap
    for _ in range(4):
        gb.step(images, tok_b, masks, labels)
    torch.cuda.synchronize()
    assert a.step_count == b.step_count == 6
    # Two separately built runs are not bit-reproducible whether or not one of them swaps: the adapter gradients are summed with fp32
    # atomics in no fixed order (test_step_gpu.py compares its twins in the norm of the step taken for the same reason; measured here:
    # the arena differs by 1.5e-8 in single entries, every other tensor by nothing).  The bit-exact statement is the one above --
    # everything a replay reads is what it was before the two swaps -- and the twin is held to test_graphed_step_matches_eager's bound.
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k, p in pa.items():
        if p.requires_grad:
            step_sz = float((pb[k].detach() - init[k]).float().norm())
            diff = float((p.detach() - pb[k].detach()).float().norm())
            print(f'twin {k}: |a - b| = {diff:.3e}, |step| = {step_sz:.3e}')
            assert diff <= 0.05 * step_sz + 1e-7, k
    for x, y, t in zip(a.ema_shadow, b.ema_shadow, b.ema_sources()):
        assert float((x - y).norm()) <= 0.05 * float((y - t.detach()).norm()) + 1e-7


# ------------------------------------------------------------------------------------------------------------- 6. checkpoint
def test_checkpoint_restores_and_writes_the_average(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    from test_model_gpu import build_model
    meta, state, batch, images, labels = _case()
    masks = {m: t.cuda() for m, t in batch['modality_mask'].items()}

    def make(st, **kw):
        m = build_model(meta, st, True)
        return m, FusedAdamW(_groups(m), weight_decay=1e-4, **kw)

    def bufs(m):
        return [m.bn_neck.bn.running_mean, m.bn_neck.bn.running_var]

    a = build_model(meta, state, True)
    opt = FusedAdamW(_groups(a), weight_decay=1e-4, ema_decay=0.9, ema_buffers=bufs(a))
    drv = StepDriver(a, opt)
    for _ in range(2):
        drv.step(images, batch['texts'], masks, labels)
    p_ema, p_plain, p_avg = (str(tmp_path / 'ckpt' / f) for f in ('ema.pth', 'plain.pth', 'avg.pth'))
    ck.save_checkpoint(a, opt, None, 1, 0.25, a.config, p_ema)

    # saved with an EMA -> a fresh model + optimizer: shadow bits and the update count come back
    state2 = {k: v + 0.01 for k, v in state.items()}
    b = build_model(meta, state2, True)
    opt_b = FusedAdamW(_groups(b), weight_decay=1e-4, ema_decay=0.5, ema_warmup=False, ema_buffers=bufs(b))
    ck.load_checkpoint(p_ema, b, opt_b)
    assert opt_b.ema_num_updates == opt.ema_num_updates == 2 and opt_b.step_count == 2
    assert opt_b.ema_decay == 0.9 and opt_b.ema_warmup is True
    assert len(opt_b.ema_shadow) == len(opt.ema_shadow)
    for x, y in zip(opt.ema_shadow, opt_b.ema_shadow):
        assert same_bits(x, y)
    assert any(not same_bits(s, t) for s, t in zip(opt_b.ema_shadow, opt_b.ema_sources()))

    # written without an EMA -> an optimizer with one: the shadows are the loaded parameters, not the construction-time ones
    plain = FusedAdamW(_groups(a), weight_decay=1e-4)
    saved = ck.save_checkpoint(a, plain, None, 1, 0.25, a.config, p_plain)
    assert 'ema_state_dict' not in saved
    c = build_model(meta, state2, True)
    opt_c = FusedAdamW(_groups(c), weight_decay=1e-4, ema_decay=0.9, ema_buffers=bufs(c))
    ck.load_checkpoint(p_plain, c, opt_c)
    assert opt_c.ema_num_updates == 0
    for t, s, src in zip(opt_c.ema_sources(), opt_c.ema_shadow, opt.ema_sources()):
        assert same_bits(s, t) and same_bits(s, src)

    # use_ema=True: the averaged weights under the reference's key set
    live = [bits(t) for t in opt.ema_sources()]
    full = ck.save_checkpoint(a, opt, None, 1, 0.25, a.config, p_avg, use_ema=True)
    assert all(np.array_equal(bits(t), l) for t, l in zip(opt.ema_sources(), live))      # swapped back
    sd = torch.load(p_avg, map_location='cpu', weights_only=False)['model_state_dict']
    keys = json.load(open(os.path.join(GOLDEN, 'state_keys.json')))['tiny']['keys']
    assert set(sd) == {k for k, _, _ in keys} == set(full['model_state_dict'])
    shadow_of = {id(t): s for t, s in zip(opt.ema_sources(), opt.ema_shadow)}
    checked = 0
    for k, p in a._ref.items():
        if id(p) in shadow_of and p is not a.lora_arena:     # (the arena is stored as its per-adapter views: below)
            assert same_bits(sd[k], shadow_of[id(p)]), k
            checked += 1
    for k, t in a._bufs.items():
        if id(t) in shadow_of:
            assert same_bits(sd[k], shadow_of[id(t)]), k
            checked += 1
    arena_shadow = shadow_of[id(a.lora_arena)]
    lora_keys = [k for k in sd if '.loras.' in k]
    assert lora_keys
    for k in lora_keys:
        assert same_bits(sd[k], a.layout.ref_view(arena_shadow, k)), k
    assert checked + 1 == len(opt.ema_shadow)                   # every averaged tensor was compared
    live_sd = torch.load(p_ema, map_location='cpu', weights_only=False)['model_state_dict']
    assert any(not torch.equal(sd[k], live_sd[k]) for k in lora_keys)
