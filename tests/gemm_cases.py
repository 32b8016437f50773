"""The reid_mer_gemm call forms the tests share: CASES (run element-wise by test_gemm_exact_gpu.py, routed by test_gemm_plan_cpu.py)
and STEP_CASES (the training step's seven shapes at full size: routed only), plus what turns a case into arguments and a plan
into the label vocabulary of the exact tests."""
S = 197             # ViT tokens per image (rows_per_img of the vision tower)
BIG = 333 * S       # 65 601 rows: the 256-row skinny tiles (M >= 65536), ragged

# The call forms engine.py makes, plus forced tiles (GEMM_TILE 3 / 12 / 14) where the default would not reach a form.  Ragged M
# everywhere; lda / ldb / ldc / ldr / ldaux / ldc2 padded (pad 8, or 4 where the 4-aligned store forms are meant).
CASES = [
    dict(name='qkv_row_groups', groups=[3, 4, 2, 3], N=2304, K=768, bias=True),
    dict(name='lora_down_T32', M=9 * S, N=32, K=768, mask_r=8, mask_period=32, alpha=0.5),
    dict(name='lora_down_T32_big', M=BIG, N=32, K=768, mask_r=8, mask_period=32, alpha=0.5),
    dict(name='lora_down_T96', M=9 * S, N=96, K=768, mask_r=8, mask_period=32, alpha=0.5),
    dict(name='lora_down_T64', M=9 * S, N=64, K=768, mask_r=16, mask_period=64, alpha=0.5),
    dict(name='lora_down_T64_big', M=BIG, N=64, K=768, mask_r=16, mask_period=64, alpha=2.0),
    dict(name='k_extension', M=1000, N=2304, K=768, K2=32, k2_group_n=768, bias=True),
    dict(name='k_extension_pp256', M=1000, N=2304, K=768, K2=32, k2_group_n=768, bias=True, tile=12),
    dict(name='k_extension_pp224', M=1000, N=2304, K=768, K2=32, k2_group_n=768, bias=True, tile=14),
    dict(name='out_proj_f16', M=1000, N=768, K=768, bias=True, out='f16'),
    dict(name='out_proj_residual_pps', M=256 * S, N=768, K=768, bias=True, out='f32', R=True, row_scale=True),
    dict(name='out_proj_residual_groups', groups=[3, 4, 2, 3], N=768, K=768, bias=True, out='f32', R=True, row_scale=True, tile=12),
    dict(name='fc2_residual', M=1000, N=768, K=3072, bias=True, out='f32', R=True),
    dict(name='fc2_f16', M=1000, N=768, K=3072, bias=True, out='f16'),
    dict(name='plain16_pps_multi', M=5700, N=3072, K=256, bias=True, tile=12),
    dict(name='fc1_gelu_dsave', M=5700, N=3072, K=768, bias=True, act='gelu_dsave', C2=True),
    dict(name='fc1_gelu_dsave_128', M=1000, N=3072, K=768, bias=True, act='gelu_dsave', C2=True),
    dict(name='fc1_gelu_pre', M=1000, N=3072, K=768, bias=True, act='gelu', C2=True),
    dict(name='fc1_gelu_pre_pp256', M=1000, N=3072, K=768, bias=True, act='gelu', C2=True, tile=12),
    dict(name='fc1_bwd_mul_aux', M=1000, N=3072, K=768, act='mul_aux'),
    dict(name='fc1_bwd_mul_aux_pp224', M=1000, N=3072, K=768, act='mul_aux', tile=14),
    dict(name='fc1_bwd_dgelu', M=1000, N=3072, K=768, act='dgelu', tile=3),
    dict(name='text_fc1_quick_gelu', M=5 * 77, N=2048, K=512, bias=True, act='quick_gelu', C2=True),
    dict(name='text_fc1_bwd_dquick_gelu', M=5 * 77, N=2048, K=512, act='dquick_gelu'),
    dict(name='relu_f32', M=5 * 77, N=512, K=512, bias=True, act='relu', out='f32'),
    dict(name='drelu', M=5 * 77, N=512, K=512, act='drelu'),
    dict(name='patch_embed', M=6 * (S - 1), N=768, K=768, bias=True, out='f32', R=True, patch=True),
    dict(name='patch_embed_pp256', M=6 * (S - 1), N=768, K=768, bias=True, out='f32', R=True, patch=True, tile=12),
    dict(name='alpha_4col_store', M=1000, N=772, K=768, bias=True, alpha=2.0, pad=4),
    dict(name='plain_f32', M=1000, N=640, K=768, bias=True, out='f32'),
]

# The seven GEMMs of a vision block in a training step (engine.py: 256 images packed modality by modality, merged weights).
_STEP = dict(groups=[64, 64, 64, 64])
STEP_CASES = [
    dict(name='step_qkv', N=2304, K=768, bias=True, **_STEP),
    dict(name='step_out_proj_f16', N=768, K=768, bias=True, out='f16', **_STEP),
    dict(name='step_fc1_gelu_dsave', N=3072, K=768, bias=True, act='gelu_dsave', C2=True, **_STEP),
    dict(name='step_fc2_f16', N=768, K=3072, bias=True, out='f16', **_STEP),
    dict(name='step_fc2_bwd_mul_aux', N=3072, K=768, act='mul_aux', **_STEP),
    dict(name='step_fc1_bwd_plain', N=768, K=3072, **_STEP),
    dict(name='step_qkv_bwd_plain', N=768, K=2304, **_STEP),
]

for _c in CASES + STEP_CASES:
    if _c.get('groups'):
        _c['M'] = sum(_c['groups']) * S
    pad = _c.get('pad', 8)
    _c['ldc'] = _c['N'] + pad
    _c['ldr'] = _c['ldaux'] = _c['ldc2'] = _c['N'] + 8
    _c['lda'] = _c['K'] + 8


def case_call(c, t16):
    """(A, B, C, keyword arguments) of case `c`'s ops.gemm call as EMPTY CPU tensors (t16 = the flavor's 16-bit dtype): what a plan needs
    -- pointers, shapes, strides, dtypes -- and nothing a kernel could read."""
    import torch
    M, N, K, act = c['M'], c['N'], c['K'], c.get('act', 'none')

    def empty(rows, cols, ld, dtype):
        return torch.empty(rows, ld, dtype=dtype)[:, :cols]
    A = empty(M, K, c['lda'], t16)
    kw = {}
    if c.get('groups'):
        B = torch.empty(4, N, K + 8, dtype=t16)[:, :, :K]
        ends, n = [], 0
        for g in c['groups']:
            n += g * S
            ends.append(n)
        kw['row_groups'] = (ends, [2, 0, 3, 1][:len(ends)])
    else:
        B = empty(N, K, K + 8, t16)
    out = c.get('out', 't16')
    crows = (M // (S - 1)) * S if c.get('patch') else M
    C = empty(crows, N, c['ldc'], torch.float32 if out == 'f32' else (torch.float16 if out == 'f16' else t16))
    if c.get('K2'):
        G = N // c['k2_group_n']
        kw.update(A2=empty(M, G * c['K2'], G * c['K2'] + 8, t16), B2=empty(N, c['K2'], c['K2'] + 8, t16), K2=c['K2'], k2_group_n=c['k2_group_n'])
    n_img = (M + S - 1) // S
    if c.get('bias'):
        kw['bias'] = torch.empty(N)
    if c.get('row_scale'):
        kw.update(row_scale=torch.empty(n_img), rows_per_img=S)
    if c.get('patch'):
        kw.update(R=empty(S, N, c['ldr'], torch.float32)[1:], r_period=S - 1, c_group=S - 1, c_group_stride=S, c_row_off=1)
    elif c.get('R'):
        kw['R'] = empty(M, N, c['ldr'], torch.float32)
    if act in ('dgelu', 'dquick_gelu', 'mul_aux', 'drelu'):
        kw['aux'] = empty(M, N, c['ldaux'], t16)
    if act != 'none':
        kw['act'] = act
    if c.get('C2'):
        kw['C2'] = empty(M, N, c['ldc2'], t16)
    if c.get('mask_r'):
        kw.update(img_mod=torch.empty(n_img, dtype=torch.int32), mask_r=c['mask_r'], mask_period=c['mask_period'], rows_per_img=S)
    if c.get('alpha', 1.0) != 1.0:
        kw['alpha'] = c['alpha']
    return A, B, C, kw


def case_plan(ops, c, cus):
    """The plan of case `c` (its forced tile included) on `cus` compute units (0: the current device's), from the loaded library."""
    from prcv2025reid_amd import _lib
    A, B, C, kw = case_call(c, _lib.t16())
    return ops.gemm_plan(A, B, C, cus=cus, tile=c.get('tile', 0), **kw)


def plan_labels(c, plan):
    """The exact tests' labels of a plan: skinny64x32, ..., main128_lean|generic, pp256|224[_generic], pps256|224, pps_ragged (some
    group's rows are not a multiple of bm), pps_multi (more tiles than workgroups)."""
    from prcv2025reid_amd._lib import GEMM_KERNELS
    kernel, generic = GEMM_KERNELS[plan.kernel], plan.epilogue == 0
    if kernel == 'tiled':
        return {f'skinny{plan.bm}x{plan.bn}'} if plan.bn < 128 else {'main128_' + ('generic' if generic else 'lean')}
    if kernel == 'pp':
        return {f'pp{plan.bm}' + ('_generic' if generic else '')}
    labels = {f'pps{plan.bm}'}
    if any(rows % plan.bm for rows in ([n * S for n in c['groups']] if c.get('groups') else [c['M']])):
        labels.add('pps_ragged')
    if plan.tiles_m * plan.tiles_n > plan.grid:
        labels.add('pps_multi')
    return labels
