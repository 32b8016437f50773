"""CPU: the stage references of engine_stage_ref.py are the reference model, and their bounds can see a wiring slip.

Composition: with no rounding anywhere (fmt None) the forward stages composed reproduce O.encode_vision / O.encode_text to 1e-12, the
backward stages composed reproduce autograd through the oracle to 1e-10 (adapters and, for the vision tower, every dense tensor), with
mixed modalities in non-sorted order and DropPath factors that include zeros.

Mutants: each slip an executor rewrite could make, applied to the reference on the inputs of one stage, must put its worst element at
least 8 of that stage's bf16 bounds (the looser flavor) away from the unmutated reference."""
import pytest
import torch

import engine_stage_ref as R
from helpers import case_inputs, load_case, round16
from oracle import reid_oracle as O

ORDER = (('cp', 2), ('vis', 3), ('nir', 1))               # uneven groups, not in modality order, sk absent


def tiny_case(rank=8, seed=3):
    """The tiny_train_all architecture with non-zero lora_B and biases, fp64; DropPath: None on layer 0's attention branch, an image
    dropped in every other branch, image 4 dropped in both branches of the last block."""
    _, meta = load_case('tiny_train_all')
    meta = dict(meta); meta['rank'] = float(rank); meta['alpha'] = 2.0 * rank
    cfg, arch, state, batch, tokens = case_inputs(meta)
    g = torch.Generator().manual_seed(seed)
    state = {k: v.detach().clone() for k, v in state.items()}
    for k, v in state.items():
        if 'lora_B' in k:
            v.copy_(0.05 * torch.randn(v.shape, generator=g))
        elif k.endswith('.bias') and k.startswith('clip_encoder.') and v.is_floating_point():
            v.add_(0.05 * torch.randn(v.shape, generator=g))
    groups = [(m, torch.randn(n, 3, 224, 224, generator=g)) for m, n in ORDER]
    drop = drop_factors(arch['vision_layers'], sum(n for _, n in ORDER))
    return meta, arch, state, groups, drop, tokens


def drop_factors(L, n):
    keep = [1.0 - 0.2 * l / max(1, L - 1) for l in range(L)]
    drop = []
    for l in range(L):
        sa = torch.full((n,), 1.0 / keep[l], dtype=torch.float64); sm = sa.clone()
        sa[(l + 1) % n] = 0.0; sm[(l + 3) % n] = 0.0
        if l == L - 1:
            sa[n - 2] = 0.0; sm[n - 2] = 0.0
        drop.append((None if l == 0 else sa, sm))
    return drop


def f64(state):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}


def oracle_vision(state, arch, groups, drop):
    out, start = [], 0
    for m, img in groups:
        n = img.shape[0]
        ds = [tuple(None if s is None else s[start:start + n] for s in pair) for pair in drop]
        out.append(O.encode_vision(img, m, state, arch, ds))
        start += n
    return torch.cat(out)


def test_vision_stages_compose_to_the_oracle():
    meta, arch, state, groups, drop, _ = tiny_case()
    s64 = f64(state)
    g64 = [(m, img.double()) for m, img in groups]
    mods = [m for m, img in groups for _ in range(img.shape[0])]
    dense_keys = [k for k in s64 if k.startswith('clip_encoder.') and not k.startswith(R.TXT) and k != 'clip_encoder.text_proj.weight'
                  and s64[k].is_floating_point()]
    leaf = {k: (v.clone().requires_grad_(True) if k in dense_keys else v) for k, v in s64.items()}
    want = oracle_vision(leaf, arch, g64, drop)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (want * cot).sum().backward()
    want = want.detach()
    gref = {k: (torch.zeros_like(s64[k]) if leaf[k].grad is None else leaf[k].grad) for k in dense_keys}   # (None: an absent modality)

    ref = R.VisionRef(arch, R.Operands.exact(s64, [m for m in arch['modalities'] if m != 'text']), mods, drop, None)
    feats, st = R.vision_forward(ref, g64)
    err = float((feats - want).abs().max() / want.abs().max())
    assert err <= 1e-12, err
    # the attention stage's two fp64 forms (oracle's attention_core, the kernel test's _attn_ref64) are one function
    at = ref.attn(st['layers'][0]['qkv'])
    oh = at['o_heads'].transpose(1, 2).reshape(at['o'][0].shape)
    assert float((oh - at['o'][0]).abs().max()) <= 1e-13

    for want_dense, scale in ((True, 1.0), (False, 64.0)):
        grads = R.vision_backward(ref, st, cot, scale=scale, want_dense=want_dense)
        keys = dense_keys if want_dense else [k for k in dense_keys if '.loras.' in k]
        gmax = max(float(gref[k].abs().max()) for k in keys)
        missing = set(keys) - set(grads)                    # (the patch convolution of a modality no image has gets no gradient)
        assert missing <= {k for k in keys if '.patch_embeds.sk.' in k} and all(float(gref[k].abs().max()) == 0.0 for k in missing), missing
        keys = [k for k in keys if k in grads]
        worst = 0.0
        for k in keys:
            g = gref[k]
            top = float(g.abs().max())
            den = top if top > 1e-9 * gmax else gmax        # (mathematically zero tensors: an absent modality, the key bias)
            e = float((grads[k] - g).abs().max()) / den
            worst = max(worst, e)
            assert e <= 1e-10, (k, e)
        absent = [k for k in keys if '.loras.sk.' in k]
        assert absent and all(float(grads[k].abs().max()) == 0.0 for k in absent)
        print(f'\nvision composition (dense {want_dense}): features {err:.2e}, worst gradient {worst:.2e} over {len(keys)} tensors')


def text_case(tokens, arch):
    """Prefix masks of lengths 2..T and an EOS that is not the last token (rows also get a second, later EOS)."""
    ids = tokens['input_ids'].clone()
    B, T = ids.shape
    lens = torch.tensor([2 + (i * (T - 2)) // max(1, B - 1) for i in range(B)])
    km = (torch.arange(T)[None] < lens[:, None]).long()
    eos = arch['text_eos_id']
    ids[ids == eos] = 5
    for i in range(B):
        ids[i, max(1, int(lens[i]) - 1 - (i % 2))] = eos       # first EOS: the last valid token or the one before it
        ids[i, T - 1] = eos if i % 3 == 0 else ids[i, T - 1]
    return ids, km


def test_text_stages_compose_to_the_oracle():
    meta, arch, state, groups, drop, tokens = tiny_case()
    s64 = f64(state)
    ids, km = text_case(tokens, arch)
    assert bool(((ids == arch['text_eos_id']).int().argmax(-1) < ids.shape[1] - 1).all()) and int(km.sum(1).min()) == 2 and int(km.sum(1).max()) == ids.shape[1]
    want = O.encode_text(ids, km, s64, arch)
    feats, _ = R.text_forward(R.TextRef(arch, s64, ids, km, None))
    err = float((feats - want).abs().max() / want.abs().max())
    print(f'\ntext composition: features {err:.2e}')
    assert err <= 1e-12, err


# ---------------------------------------------------------------------------------------------------------------- mutants
@pytest.fixture(scope='module')
def sim():
    """The stages composed with every output stored as the bf16 executor stores it: the inputs a stage sees in a run."""
    meta, arch, state, groups, drop, _ = tiny_case()
    s64 = f64(state)
    g64 = [(m, img.double()) for m, img in groups]
    mods = [m for m, img in groups for _ in range(img.shape[0])]
    ref = R.VisionRef(arch, R.Operands.from_state(s64, arch, 'bf16'), mods, drop, 'bf16', dx_fmt='f16')
    feats, st = R.vision_forward(ref, g64)
    return ref, st, s64, arch


def far(mut, stage, what):
    ref, bound = stage
    r = R.ratio(mut, ref, bound)
    print(f'\nmutant {what}: worst element {r:.1f} bounds from the reference')
    assert r >= 8.0, (what, r)


def test_mutant_residual_stream_rounded_to_16_bits(sim):
    ref, st, _, _ = sim
    s = st['layers'][0]
    stage = ref.xm(0, s['x'], s['o'])
    far(round16(stage[0], 'bf16'), stage, 'bf16 rounding of xm')
    s = st['layers'][1]
    stage = ref.xn(1, s['xm'], s['g'])
    far(round16(stage[0], 'bf16'), stage, 'bf16 rounding of x_final')


def test_mutant_branch_stored_in_the_wrong_format(sim):
    """The pruned last block adds its unrounded branch in the GEMM epilogue: a 16-bit store of that branch in the flavor's format."""
    ref, st, _, _ = sim
    s = st['layers'][1]
    x, o = ref.cls_rows(s['x']), s['o_rows']
    stage = ref.xm(1, x, o)
    br, _ = ref._lin(1, 'attn.out_proj', o, 1)
    sa = ref.drop[1][0][:, None]
    far(x + sa * round16(br, 'bf16'), stage, 'last block branch in bf16')


def _with_views(ref, fwd):
    ops = R.Operands(fwd, ref.ops.bwd, ref.ops.plain)
    return R.VisionRef(ref.a, ops, ref.mods, ref.drop, ref.fmt, ref.dx_fmt)


@pytest.mark.parametrize('lin', ['qkv', 'out', 'fc1', 'fc2'])
def test_mutant_bias_dropped(sim, lin):
    ref, st, _, _ = sim
    s = st['layers'][0]
    proj = R.PROJ[lin][-1]
    kb = f'{R.VIS}0.{proj}.shared_linear.bias'
    fwd = {m: {**v, kb: torch.zeros_like(v[kb])} for m, v in ref.ops.fwd.items()}
    mut = _with_views(ref, fwd)
    call = dict(qkv=lambda r: r.qkv(0, s['h']), out=lambda r: r.xm(0, s['x'], s['o']), fc1=lambda r: r.fc1(0, s['h2'])['g'],
                fc2=lambda r: r.xn(0, s['xm'], s['g']))[lin]
    far(call(mut)[0], call(ref), f'{lin} bias dropped')


@pytest.mark.parametrize('lin', ['qkv', 'out', 'fc1', 'fc2'])
def test_mutant_row_group_boundary_takes_the_neighbours_weight(sim, lin):
    ref, st, _, _ = sim
    s = st['layers'][0]
    mods = list(ref.mods); mods[1] = mods[2]                 # the last cp image multiplied with the vis stack
    mut = R.VisionRef(ref.a, ref.ops, mods, ref.drop, ref.fmt, ref.dx_fmt)
    call = dict(qkv=lambda r: r.qkv(0, s['h']), out=lambda r: r.xm(0, s['x'], s['o']), fc1=lambda r: r.fc1(0, s['h2'])['g'],
                fc2=lambda r: r.xn(0, s['xm'], s['g']))[lin]
    far(call(mut)[0], call(ref), f'{lin} neighbour weight at a row-group boundary')


def test_mutant_drop_factors_swapped(sim):
    ref, st, _, _ = sim
    s = st['layers'][1]
    sa, sm = ref.drop[1]
    swapped = R.VisionRef(ref.a, ref.ops, ref.mods, [ref.drop[0], (sm, sa)], ref.fmt, ref.dx_fmt)
    x, o = ref.cls_rows(s['x']), s['o_rows']
    far(swapped.xm(1, x, o)[0], ref.xm(1, x, o), 'sa / sm swapped (xm)')
    far(swapped.xn(1, s['xm'], s['g'])[0], ref.xn(1, s['xm'], s['g']), 'sa / sm swapped (xn)')
    # backward: the 16-bit copy leaving LN1 of layer 1 carries layer 0's MLP factor, not layer 1's
    g = torch.Generator().manual_seed(4)
    M, d = s['x'].shape
    dh = round16(torch.randn(M, d, generator=g, dtype=torch.float64), 'bf16')
    dxm = round16(torch.randn(M, d, generator=g, dtype=torch.float64), 'f16')
    wrong = R.VisionRef(ref.a, ref.ops, ref.mods, [(None, ref.drop[1][1]), ref.drop[1]], ref.fmt, ref.dx_fmt)
    far(wrong.ln1_bwd(1, dh, s['x'], s['mean1'], s['rstd1'], dxm)['dxb'][0], ref.ln1_bwd(1, dh, s['x'], s['mean1'], s['rstd1'], dxm)['dxb'],
        'sm of the wrong layer as the copy factor')


def test_mutant_T_scaled_twice(sim):
    ref, st, _, _ = sim
    s = st['layers'][0]
    for nm, X in (('qkv', s['h']), ('out', s['o_rows']), ('fc1', s['h2']), ('fc2', s['g'])):
        stage = ref.T(0, nm, X)
        far(stage[0] * ref.scaling, stage, f'T of {nm} scaled twice')


def test_mutant_last_block_reads_x_for_xm(sim):
    ref, st, _, _ = sim
    s = st['layers'][1]
    far(ref.xn(1, ref.cls_rows(s['x']), s['g'])[0], ref.xn(1, s['xm'], s['g']), 'class-row fc2 residual reads x')
