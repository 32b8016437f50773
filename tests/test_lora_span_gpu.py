"""GPU: the adapter-gradient image kernels (reid_lora_bwd_fused / reid_lora_da_fused) with several same-modality images per workgroup.

A workgroup owns LORA_SPAN consecutive images and works through them as maximal runs of one modality: one ring prologue, one step loop
and one flush of fp32 atomics per run.  Every forced span (knob LORA_SPAN = 1, 2, 4, 8) and the default rule must give, on EXACT
operands (helpers.exact_ints within a checked bit budget, so that fp32 atomics in any order are exact), fp32 outputs equal to the fp64
product, 16-bit U equal to its round-to-nearest-even, sentinels untouched in padding columns and guard rows, and the very bits of span 1
(one image per workgroup, the reference form) -- for image counts that are no multiple of the span (a short last span), images of one
32-row step, of a last step with one row, and of 197 rows, and modality orders that break runs inside a span (sorted with one modality
absent), never (all equal), at every image (alternating) and at random.

The engine-level test is the two-block 768-wide tower of test_lora_rank16_engine_gpu.py at ranks 8 and 16 with four images per modality
in packed (sorted) order, LoRA gradients against the oracle's autograd inside that file's gates."""
import numpy as np
import pytest
import torch

from helpers import assert_bit_budget, case_config, case_inputs, exact_ints, is_sentinel, load_case, round16, sentinel_buffer

pytestmark = pytest.mark.gpu

GUARD = 32
N = 768
SPANS = (1, 1, 2, 4, 8, -1)          # span 1 twice: a second call gives the same bits; -1: the default rule


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


def flavor():
    from prcv2025reid_amd import _lib
    return _lib.flavor()


def T16():
    from prcv2025reid_amd import _lib
    return _lib.t16()


def set_knob(name, value):
    from prcv2025reid_amd import _lib
    _lib.check(_lib.lib().reid_set_knob(name, value))


def padded16(vals, ld, fmt):
    rows, cols = vals.shape
    buf = sentinel_buffer(rows, ld, T16(), fmt)
    v = vals.to(T16())
    assert torch.equal(v.double(), vals), 'operand not representable in the 16-bit format'
    buf[:, :cols] = v
    return buf[:, :cols]


SORTED9 = (0, 0, 0, 0, 1, 1, 3, 3, 3)                     # runs break inside a span of 4 and of 8; modality 2 is absent


def img_mods(pattern, n_img, gen):
    if pattern == 'sorted':
        m = [SORTED9[i * 9 // n_img] for i in range(n_img)]
    elif pattern == 'equal':
        m = [1] * n_img
    elif pattern == 'alt':
        m = [(3, 0)[i & 1] for i in range(n_img)]
    else:
        return torch.randint(0, 4, (n_img,), generator=gen, device='cuda').to(torch.int32)
    return torch.tensor(m, dtype=torch.int32, device='cuda')


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


# rows_per_img 32 (one step), 33 (a last step of one row), 50, 197; n_img 1, 5, 9, 13; r = 8 and 2 at Rp = 32, r = 16 at Rp = 64
BWD_CASES = [(9, 197, 8, 32, 'sorted', 0), (13, 197, 16, 64, 'sorted', 0), (5, 197, 2, 32, 'alt', 0), (13, 50, 8, 32, 'random', 768),
             (9, 33, 16, 64, 'alt', 0), (13, 32, 8, 32, 'equal', 0), (5, 33, 2, 32, 'sorted', 0), (1, 197, 8, 32, 'equal', 0),
             (9, 50, 16, 64, 'random', 0), (13, 197, 8, 32, 'random', 0), (1, 32, 16, 64, 'equal', 0), (5, 32, 8, 32, 'alt', 0),
             (9, 197, 2, 32, 'equal', 0), (13, 33, 16, 64, 'sorted', 1536)]


@pytest.mark.parametrize('n_img,rpi,r,Rp,pattern,lddy_extra', BWD_CASES)
def test_lora_bwd_span_exact(ops, n_img, rpi, r, Rp, pattern, lddy_extra):
    """U = round16(mask(dY B) * scale) and dB = dB0 + dY^T T (T masked: the default path) exactly for every span, bit-equal to span 1."""
    fmt = flavor()
    M = n_img * rpi
    gen = torch.Generator(device='cuda').manual_seed(M * 5 + r + Rp + lddy_extra)
    dY64 = exact_ints((M, N + lddy_extra), -4, 4, 0, gen)
    o = lddy_extra // 2
    dY = padded16(dY64, N + lddy_extra + 8, fmt)[:, o:o + N]       # lddy_extra: lddy > N, the operand a column window of a wider tensor
    dY64 = dY64[:, o:o + N]
    mods = img_mods(pattern, n_img, gen)
    keep = (torch.arange(Rp, device='cuda').view(1, -1) // r) == mods.long().repeat_interleave(rpi).view(-1, 1)
    T64 = exact_ints((M, Rp), -4, 4, -2, gen) * keep
    Tm = padded16(T64, Rp + 8, fmt)
    BT64 = exact_ints((Rp, N), -4, 4, -4, gen)
    BT = padded16(BT64, N + 8, fmt)
    scale = 32.0 / r
    dB064 = exact_ints((N, Rp), -1024, 1024, -4, gen)
    assert_bit_budget((dY64.abs() @ BT64.abs().t()) * scale, 2.0 ** -4)
    assert_bit_budget(dB064.abs() + dY64.abs().t() @ T64.abs(), 2.0 ** -4)
    U_want = round16((dY64 @ BT64.t()) * scale * keep, fmt)
    dB_want = dB064 + dY64.t() @ T64
    first = None
    for span in SPANS:
        U = sentinel_buffer(M + GUARD, Rp + 8, T16(), fmt)
        dB = sentinel_buffer(N + GUARD, Rp + 8, torch.float32)
        dB[:N, :Rp] = dB064.float()
        set_knob(b'LORA_SPAN', span)
        try:
            ops.lora_bwd_fused(dY, Tm, BT, U[:M, :Rp], dB[:N, :Rp], mods, rpi, r, scale)
            torch.cuda.synchronize()
        finally:
            set_knob(b'LORA_SPAN', -1)
        assert torch.equal(U[:M, :Rp].double(), U_want), span
        assert bool((bits(U[:M, :Rp])[~keep] == 0).all()), span                       # other modalities' columns: +0.0
        assert torch.equal(dB[:N, :Rp].double(), dB_want), span
        assert bool(is_sentinel(U[:M, Rp:], fmt).all() and is_sentinel(U[M:], fmt).all()), span
        assert bool(is_sentinel(dB[:N, Rp:]).all() and is_sentinel(dB[N:]).all()), span
        if first is None:
            first = (U, dB)
        else:
            assert torch.equal(bits(U), bits(first[0])) and torch.equal(bits(dB), bits(first[1])), span


def test_lora_bwd_span_column_blocks_exact(ops):
    """A 3072-column cotangent as four column blocks through the fp32 scratch u_partial, on sorted modalities, for every span."""
    fmt = flavor()
    n_img, rpi, r, Nw, Rp = 9, 197, 8, 3072, 32
    M = n_img * rpi
    gen = torch.Generator(device='cuda').manual_seed(23)
    dY64 = exact_ints((M, Nw), -4, 4, 0, gen)
    dY = padded16(dY64, Nw + 8, fmt)
    mods = img_mods('sorted', n_img, gen)
    keep = (torch.arange(Rp, device='cuda').view(1, -1) // r) == mods.long().repeat_interleave(rpi).view(-1, 1)
    T64 = exact_ints((M, Rp), -4, 4, -2, gen) * keep
    Tm = padded16(T64, Rp + 8, fmt)
    BT64 = exact_ints((Rp, Nw), -4, 4, -4, gen)
    BT = padded16(BT64, Nw + 8, fmt)
    scale = 4.0
    assert_bit_budget((dY64.abs() @ BT64.abs().t()) * scale, 2.0 ** -4)
    assert_bit_budget(dY64.abs().t() @ T64.abs(), 2.0 ** -4)
    U_want = round16((dY64 @ BT64.t()) * scale * keep, fmt)
    dB_want = dY64.t() @ T64
    first = None
    for span in SPANS:
        U = sentinel_buffer(M + GUARD, Rp + 8, T16(), fmt)
        dB = sentinel_buffer(Nw + GUARD, Rp + 8, torch.float32)
        dB[:Nw, :Rp] = 0.0
        scratch = torch.full((M, Rp), float('nan'), device='cuda')
        set_knob(b'LORA_SPAN', span)
        try:
            ops.lora_bwd_fused(dY, Tm, BT, U[:M, :Rp], dB[:Nw, :Rp], mods, rpi, r, scale, u_partial=scratch)
            torch.cuda.synchronize()
        finally:
            set_knob(b'LORA_SPAN', -1)
        assert torch.equal(U[:M, :Rp].double(), U_want), span
        assert torch.equal(dB[:Nw, :Rp].double(), dB_want), span
        assert bool(is_sentinel(U[:M, Rp:], fmt).all() and is_sentinel(U[M:], fmt).all() and is_sentinel(dB[:Nw, Rp:]).all()
                    and is_sentinel(dB[Nw:]).all()), span
        if first is None:
            first = (U, dB)
        else:
            assert torch.equal(bits(U), bits(first[0])) and torch.equal(bits(dB), bits(first[1])), span


DA_CASES = [(9, 197, 8, 32, 768, 1, 'sorted'), (13, 197, 16, 64, 768, 3, 'sorted'), (5, 33, 2, 32, 1536, 1, 'alt'),
            (13, 50, 8, 32, 1536, 3, 'random'), (9, 32, 16, 64, 1536, 1, 'equal'), (1, 197, 8, 32, 768, 3, 'equal'),
            (13, 33, 8, 32, 768, 1, 'alt'), (5, 197, 16, 64, 1536, 3, 'random'), (9, 50, 2, 32, 768, 3, 'sorted')]


@pytest.mark.parametrize('n_img,rpi,r,Rp,K,G,pattern', DA_CASES)
def test_lora_da_span_exact(ops, n_img, rpi, r, Rp, K, G, pattern):
    """dA = dA0 + U^T X exactly for every span, bit-equal to span 1; rows of adapters whose modality no image has keep dA0's bits."""
    fmt = flavor()
    M = n_img * rpi
    gen = torch.Generator(device='cuda').manual_seed(M * 3 + K + G + Rp)
    X64 = exact_ints((M, K), -4, 4, -4, gen)
    X = padded16(X64, K + 8, fmt)
    mods = img_mods(pattern, n_img, gen)
    keep = ((torch.arange(G * Rp, device='cuda').view(1, -1) % Rp) // r) == mods.long().repeat_interleave(rpi).view(-1, 1)
    U64 = exact_ints((M, G * Rp), -4, 4, 0, gen) * keep
    U = padded16(U64, G * Rp + 8, fmt)
    dA064 = exact_ints((G * Rp, K), -1024, 1024, -4, gen)
    want = dA064 + U64.t() @ X64
    assert_bit_budget(dA064.abs() + U64.abs().t() @ X64.abs(), 2.0 ** -4)
    unused = ~keep.any(0)                                  # adapter rows no image's modality selects
    assert pattern == 'random' or bool(unused.any())
    assert ops.lora_da_fused_ok(K, Rp, rpi, r, G)
    first = None
    for span in SPANS:
        dA = sentinel_buffer(G * Rp + GUARD, K + 8, torch.float32)
        dA[:G * Rp, :K] = dA064.float()
        set_knob(b'LORA_SPAN', span)
        try:
            ops.lora_da_fused(X, U, dA[:G * Rp, :K], mods, rpi, r, n_groups=G)
            torch.cuda.synchronize()
        finally:
            set_knob(b'LORA_SPAN', -1)
        got = dA[:G * Rp, :K]
        assert torch.equal(got.double(), want), span
        assert torch.equal(bits(got[unused]), bits(dA064[unused].float())), span
        assert bool(is_sentinel(dA[:G * Rp, K:]).all() and is_sentinel(dA[G * Rp:]).all()), span
        if first is None:
            first = dA
        else:
            assert torch.equal(bits(dA), bits(first)), span


# ---- engine level ---------------------------------------------------------------------------------------------------------------
LAYERS = 2
PER_MOD = 4
_REF = {}


def l2rel(a, b):
    a = torch.as_tensor(np.asarray(a)).double().flatten(); b = torch.as_tensor(np.asarray(b)).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def tower_case(rank):
    """Inputs, weights and the oracle's LoRA gradients of the tower at `rank`: computed once, shared by both flavors, left unchanged."""
    if rank in _REF:
        return _REF[rank]
    from oracle import reid_oracle as O
    _, meta = load_case('tiny_train_frozen')
    meta = dict(meta); meta['rank'] = float(rank); meta['alpha'] = 2.0 * rank
    meta.update(vision_hidden_dim=768.0, vision_heads=12.0, vision_mlp_dim=3072.0, vision_layers=float(LAYERS))
    cfg, arch, state, batch, tokens = case_inputs(meta)
    g = torch.Generator().manual_seed(11)
    imgs = {m: torch.randn(PER_MOD, 3, 224, 224, generator=g) for m in ('vis', 'nir', 'sk', 'cp')}
    R = {m: torch.randn(PER_MOD, 512, generator=g) for m in imgs}
    lora_keys = [k for k in state if '.loras.' in k]
    for k in lora_keys:
        if 'lora_B' in k:                               # (a zero B would leave the merged update and dA at zero)
            state[k].copy_(0.05 * torch.randn(state[k].shape, generator=g))
        state[k].requires_grad_(True)
    loss = sum((O.encode_vision(imgs[m], m, state, arch) * R[m]).sum() for m in imgs)
    loss.backward()
    ref = {k: state[k].grad.detach().clone() for k in lora_keys}
    _REF[rank] = (meta, {k: v.detach() for k, v in state.items()}, imgs, R, lora_keys, ref)
    return _REF[rank]


@pytest.mark.parametrize('rank', [8, 16])
@pytest.mark.parametrize('flavor_name,tol', [('bf16', 4e-2), ('f16', 8e-3)])
def test_tower_lora_gradients_per_span(flavor_name, tol, rank):
    """Packed (sorted) modalities, four images each: LoRA gradients of the tower's backward against the oracle's autograd under the
    default rule, with one image per workgroup (LORA_SPAN = 1) and with four (a span = one modality's images)."""
    from prcv2025reid_amd.engine import VisionEncodeFn
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    meta, state, imgs, R, lora_keys, ref = tower_case(rank)
    cfg = case_config(meta, device='cuda')
    cfg.compute_dtype = flavor_name
    model = CLIPBasedMultiModalReIDModel(cfg)
    model.set_num_classes(int(meta['num_classes']))
    model.load_state_dict(state, strict=True)
    apply_reference_freeze(model)
    model.contrastive_weight = meta['contrastive_weight']
    model.set_epoch(2)
    model.train(True)
    model.engine.refresh()
    mods = tuple(model.vision_modalities.index(m) for m in imgs)
    cot = torch.cat([R[m] for m in imgs]).cuda()
    dev_imgs = [imgs[m].cuda() for m in imgs]
    worst = {}
    try:
        for span in (-1, 1, 4):
            set_knob(b'LORA_SPAN', span)
            model.lora_arena.grad = None
            feats = VisionEncodeFn.apply(model.engine, mods, model.lora_arena, len(imgs), *dev_imgs)
            (feats * cot).sum().backward()
            torch.cuda.synchronize()
            got = {k: model.lora_grad_view(k).detach().cpu().clone() for k in lora_keys}
            worst[span] = max(l2rel(got[k], ref[k]) for k in lora_keys)
    finally:
        set_knob(b'LORA_SPAN', -1)
        from prcv2025reid_amd import _lib
        _lib.set_flavor('bf16')
    print(f'\n  [{flavor_name}] rank {rank}: worst LoRA grad rel-L2 vs oracle by LORA_SPAN: {worst} (gate {tol})')
    for span, w in worst.items():
        assert w < tol, (span, w)
