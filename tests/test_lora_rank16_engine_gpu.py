"""GPU: at LoRA rank 16 (four modalities x 16 = 64 adapter rows, Rp = 64) the vision tower's backward forms the adapter gradients of
every full-row linear with the one-pass image kernels (reid_lora_bwd_fused / reid_lora_da_fused) and gets the gradients the two-launch
path (reid_mer_gemm + reid_gemm_tn) gets.

Built as test_model_gpu.py::test_lora_rank_32_vs_oracle: the tiny_train_frozen fixture's seeds, class count and two blocks with
rank = 16, alpha = 32, two images per modality, lora_B randomised, a random cotangent, autograd through oracle.reid_oracle as the
reference -- with the tower's width set to 768 (12 heads, MLP 3072): the image kernels are built for 768-column operands, and at the
fixture's own width of 128 no path under test would run.  Gates: the ones of that test (worst LoRA-gradient rel-L2 below 4e-2 for
bf16, 8e-3 for f16), for both paths."""
import numpy as np
import pytest
import torch

from helpers import load_case, case_inputs, case_config

pytestmark = pytest.mark.gpu

LAYERS = 2


def l2rel(a, b):
    a = torch.as_tensor(np.asarray(a)).double().flatten(); b = torch.as_tensor(np.asarray(b)).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build_model(meta, state, flavor):
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    cfg = case_config(meta, device='cuda')
    cfg.compute_dtype = flavor
    model = CLIPBasedMultiModalReIDModel(cfg)
    model.set_num_classes(int(meta['num_classes']))
    model.load_state_dict(state, strict=True)
    apply_reference_freeze(model)
    model.contrastive_weight = meta['contrastive_weight']
    model.set_epoch(2)
    model.train(True)
    return model


@pytest.mark.parametrize('flavor,tol', [('bf16', 4e-2), ('f16', 8e-3)])
def test_rank16_backward_takes_image_kernels(flavor, tol, monkeypatch):
    from oracle import reid_oracle as O
    from prcv2025reid_amd import ops
    from prcv2025reid_amd.engine import VisionEncodeFn
    _, meta = load_case('tiny_train_frozen')
    meta = dict(meta); meta['rank'] = 16.0; meta['alpha'] = 32.0
    meta.update(vision_hidden_dim=768.0, vision_heads=12.0, vision_mlp_dim=3072.0, vision_layers=float(LAYERS))
    cfg, arch, state, batch, tokens = case_inputs(meta)
    model = build_model(meta, state, flavor)
    g = torch.Generator().manual_seed(11)
    imgs = {m: torch.randn(2, 3, 224, 224, generator=g) for m in ('vis', 'nir', 'sk', 'cp')}
    R = {m: torch.randn(2, 512, generator=g) for m in imgs}
    lora_keys = [k for k in state if '.loras.' in k]
    for k in lora_keys:
        if 'lora_B' in k:                               # (a zero B would leave the merged update and dA at zero)
            state[k].copy_(0.05 * torch.randn(state[k].shape, generator=g))
        state[k].requires_grad_(True)
    model.load_state_dict({k: v.detach() for k, v in state.items()}, strict=True)
    loss = sum((O.encode_vision(imgs[m], m, state, arch) * R[m]).sum() for m in imgs)
    loss.backward()
    ref = {k: state[k].grad for k in lora_keys}
    model.engine.refresh()
    mods = tuple(model.vision_modalities.index(m) for m in imgs)
    cot = torch.cat([R[m] for m in imgs]).cuda()
    dev_imgs = [imgs[m].cuda() for m in imgs]

    def run():
        model.lora_arena.grad = None
        feats = VisionEncodeFn.apply(model.engine, mods, model.lora_arena, len(imgs), *dev_imgs)
        (feats * cot).sum().backward()
        torch.cuda.synchronize()
        return {k: model.lora_grad_view(k).detach().cpu().clone() for k in lora_keys}

    calls = {'bwd': [], 'da': []}
    real_bwd, real_da = ops.lora_bwd_fused, ops.lora_da_fused

    def spy_bwd(dY, T, *a, **kw):
        calls['bwd'].append(T.shape[1])
        return real_bwd(dY, T, *a, **kw)

    def spy_da(X, U, *a, n_groups=1, **kw):
        calls['da'].append(U.shape[1] // n_groups)
        return real_da(X, U, *a, n_groups=n_groups, **kw)

    monkeypatch.setattr(ops, 'lora_bwd_fused', spy_bwd)
    monkeypatch.setattr(ops, 'lora_da_fused', spy_da)
    # (a) as shipped.  Every block: the three projections of q|k|v on full rows (three bwd calls, one dA call over three groups); every
    # block but the last (whose out-projection and MLP run on the class rows: two launches) also fc2, fc1 and the out-projection.
    ga = run()
    full = LAYERS - 1
    print(f'\n  [{flavor}] (a) lora_bwd_fused calls {len(calls["bwd"])}, lora_da_fused calls {len(calls["da"])}, Rp {sorted(set(calls["bwd"] + calls["da"]))}')
    assert set(calls['bwd']) == {64} and set(calls['da']) == {64}
    assert len(calls['bwd']) == 3 * LAYERS + 3 * full and len(calls['da']) == LAYERS + 3 * full
    # (b) the two-launch path
    calls['bwd'].clear(); calls['da'].clear()
    monkeypatch.setattr(ops, 'lora_bwd_fused_ok', lambda *a, **kw: False)
    monkeypatch.setattr(ops, 'lora_da_fused_ok', lambda *a, **kw: False)
    gb = run()
    assert not calls['bwd'] and not calls['da']
    worst_a = max(l2rel(ga[k], ref[k]) for k in lora_keys)
    worst_b = max(l2rel(gb[k], ref[k]) for k in lora_keys)
    for k in lora_keys:
        print(f'    (a) vs (b) rel-L2 {l2rel(ga[k], gb[k]):.3e}  {k}')
    print(f'  [{flavor}] rank 16: worst LoRA grad rel-L2 vs oracle: image kernels {worst_a:.3e}, two launches {worst_b:.3e}')
    assert worst_a < tol and worst_b < tol
