"""Thin, allocation-explicit Python wrappers over the C ABI (one function per entry point).

Every wrapper takes torch CUDA tensors only as device memory + stream handles; all
arithmetic happens inside libreid_hip.so.  Nothing here has a CPU path.
"""
import ctypes as C
from typing import Optional

import torch

from . import _lib as L
from ._lib import BF16, F32, GemmArgs, GemmPlan, check, lib, ptr, stream_ptr

ACT = {'none': L.ACT_NONE, 'gelu': L.ACT_GELU, 'quick_gelu': L.ACT_QUICK_GELU, 'relu': L.ACT_RELU,
       'dgelu': L.ACT_DGELU, 'dquick_gelu': L.ACT_DQUICK_GELU, 'drelu': L.ACT_DRELU,
       'mul_aux': L.ACT_MUL_AUX, 'gelu_dsave': L.ACT_GELU_DSAVE}


# optional per-launch timing of the dominant kernel (bench.py roofline): list of (flops, bytes, start_event, end_event)
_gemm_profile = None
def gemm_profile_begin():
    global _gemm_profile
    _gemm_profile = []


def gemm_profile_end():
    global _gemm_profile
    p, _gemm_profile = _gemm_profile, None
    return p


def gemm_args(A, B, C_out, *, A2=None, B2=None, K2=0, k2_group_n=0, bias=None, R=None, r_period=0, aux=None,
              C2=None, act='none', img_mod=None, mask_r=0, mask_period=0, rows_per_img=0,
              c_group=0, c_group_stride=0, c_row_off=0, alpha=1.0, M=None, row_scale=None, row_groups=None):
    """The reid_gemm_args of gemm(A, B, C_out, ...).  The tensors supply pointers, shapes and strides only."""
    a = GemmArgs()
    a.A, a.B, a.C = ptr(A), ptr(B), ptr(C_out)
    a.M = A.shape[0] if M is None else M
    if row_groups is not None:
        ends, widx = row_groups
        a.N, a.K = B.shape[1], B.shape[2]
        a.ldb = B.stride(1)
        a.n_row_groups = len(ends)
        for i, (e_, w_) in enumerate(zip(ends, widx)):
            a.row_group_end[i] = e_; a.row_group_b[i] = w_
        a.b_group_stride = B.stride(0)
    else:
        a.N, a.K = B.shape[0], B.shape[1]
        a.ldb = B.stride(0)
    a.lda, a.ldc = A.stride(0), C_out.stride(0)
    a.c_dtype = L.dt(C_out, allow_half=True)
    if A2 is not None:
        a.A2, a.B2 = ptr(A2), ptr(B2)
        a.K2 = K2 or B2.shape[1]
        a.lda2, a.ldb2 = A2.stride(0), B2.stride(0)
        a.k2_group_n = k2_group_n
    if bias is not None:
        a.bias = ptr(bias)
    if R is not None:
        a.R = ptr(R); a.ldr = R.stride(0); a.r_dtype = L.dt(R); a.r_period = r_period
    if aux is not None:
        a.aux = ptr(aux); a.ldaux = aux.stride(0)
    if C2 is not None:
        a.C2 = ptr(C2); a.ldc2 = C2.stride(0); a.c2_dtype = L.dt(C2)
    a.act = ACT[act]
    if mask_r:
        a.img_mod = ptr(img_mod); a.mask_r = mask_r; a.mask_period = mask_period; a.rows_per_img = rows_per_img
    a.c_group, a.c_group_stride, a.c_row_off = c_group, c_group_stride, c_row_off
    a.alpha = alpha
    if row_scale is not None:
        a.row_scale = ptr(row_scale); a.rows_per_img = rows_per_img
    return a


def gemm_plan(A, B, C_out, *, cus=0, tile=0, **kw):
    """The launch gemm(A, B, C_out, **kw) would make on a device of ``cus`` compute units (0: the current device's) with the GEMM_TILE
    knob at ``tile`` (0: not set): a GemmPlan (reid_mer_gemm_plan).  Nothing is launched or dereferenced: CPU tensors will do."""
    plan = GemmPlan()
    check(lib().reid_mer_gemm_plan(C.byref(gemm_args(A, B, C_out, **kw)), cus, tile, C.byref(plan)))
    return plan


def gemm(A, B, C_out, *, R=None, r_period=0, aux=None, C2=None, **kw):
    """C_out = epilogue(A @ B.T + A2 @ B2.T + bias); see reid_mer_gemm in include/reid_hip.h and gemm_args for the keywords.
    ``row_groups`` = (row_ends, weight_indices): B is then a stack [n_mats, N, K]; rows [row_ends[g-1], row_ends[g]) use B[weight_indices[g]]."""
    a = gemm_args(A, B, C_out, R=R, r_period=r_period, aux=aux, C2=C2, **kw)
    profiled = _gemm_profile is not None and a.N > 96   # mer_gemm_kernel<128,128,2,2> (dominant); skinny LoRA projections use other tiles
    if profiled:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib().reid_mer_gemm(C.byref(a), stream_ptr()))
    if profiled:
        e1.record()
        kk = a.K + a.K2
        flops = 2.0 * a.M * a.N * kk
        # compulsory bytes of the launch: both operands once, C once, plus every epilogue operand it must read or write
        # (residual R, saved pre-activation aux, second output C2) -- r01 left the last three out and overstated traffic / algorithmic
        nbytes = 2.0 * (a.M * kk + a.N * kk) + a.M * a.N * (4 if a.c_dtype == F32 else 2)
        if R is not None:
            nbytes += (r_period if r_period > 0 else a.M) * a.N * (2 if a.r_dtype == BF16 else 4)
        if aux is not None:
            nbytes += a.M * a.N * 2
        if C2 is not None:
            nbytes += a.M * a.N * (2 if a.c2_dtype == BF16 else 4)
        _gemm_profile.append((flops, nbytes, e0, e1))
    return C_out


def gemm_tn(X, Y, C_out, alpha=1.0, beta=0.0, M=None):
    """C_out[P,Q] = beta*C_out + alpha * X[:M].T @ Y[:M]  (fp32 out, bf16 in)."""
    M = X.shape[0] if M is None else M
    check(lib().reid_gemm_tn(ptr(X), ptr(Y), ptr(C_out), M, X.shape[1], Y.shape[1], X.stride(0), Y.stride(0),
                             C_out.stride(0), alpha, beta, stream_ptr()))
    return C_out


def layernorm_fwd(x, gamma, beta, y_bf16=None, y_f32=None, mean=None, rstd=None, row_index=None, rows=None,
                  eps=1e-5):
    rows = (row_index.shape[0] if row_index is not None else x.shape[0]) if rows is None else rows
    y = y_bf16 if y_bf16 is not None else y_f32
    check(lib().reid_layernorm_fwd(ptr(x), x.stride(0), ptr(row_index), ptr(gamma), ptr(beta), ptr(y_bf16), ptr(y_f32),
                                   y.stride(0), ptr(mean), ptr(rstd), rows, x.shape[1], eps, stream_ptr()))


def add_layernorm_fwd(x, y, x_out, gamma, beta, h, mean=None, rstd=None, row_scale=None, rows_per_img=0, eps=1e-5):
    """x_out = x + row_scale[row // rows_per_img] * y;  h = LayerNorm(x_out) (16-bit);  see reid_add_layernorm_fwd."""
    check(lib().reid_add_layernorm_fwd(ptr(x), x.stride(0), ptr(y), L.dt(y, allow_half=True), y.stride(0), ptr(row_scale), rows_per_img, ptr(x_out), x_out.stride(0),
                                       ptr(gamma), ptr(beta), ptr(h), h.stride(0), ptr(mean), ptr(rstd), x.shape[0], x.shape[1],
                                       eps, stream_ptr()))


_ln_profile = None


def ln_profile_begin():
    global _ln_profile
    _ln_profile = []


def ln_profile_end():
    global _ln_profile
    p, _ln_profile = _ln_profile, None
    return p


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dx_bf16=None, dres=None, row_index=None, dgamma=None, dbeta=None,
                  rows=None, bf16_row_scale=None, rows_per_img=0, overflow=None):
    """LayerNorm backward (include/reid_hip.h).  ``overflow``: an int32 device tensor the call ORs 1 into when a float16 ``dx``
    stored a clamped (finite, |v| >= 65520) element; the caller zeroes it."""
    rows = (row_index.shape[0] if row_index is not None else x.shape[0]) if rows is None else rows
    if dres is not None and dres.dtype != dx.dtype:
        raise ValueError('layernorm_bwd: dres and dx must have one dtype (float32 or float16)')
    if overflow is not None:
        L._req(overflow, torch.int32, 'overflow')
    profiled = _ln_profile is not None and rows >= 4096 and row_index is None
    if profiled:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib().reid_layernorm_bwd(ptr(dy), L.dt(dy), dy.stride(0), ptr(x), x.stride(0), ptr(row_index), ptr(gamma),
                                   ptr(mean), ptr(rstd), ptr(dres), ptr(dx), L.F16 if dx.dtype == torch.float16 else L.F32, ptr(dx_bf16), dx.stride(0), ptr(dgamma),
                                   ptr(dbeta), rows, x.shape[1], ptr(bf16_row_scale), rows_per_img, ptr(overflow), stream_ptr()))
    if profiled:
        e1.record()
        # algorithmic bytes per row: dy (2 or 4) + x (4) + dres (4 or 2) + dx (4 or 2) + 16-bit copy (2)
        nbytes = rows * x.shape[1] * ((2 if dy.dtype != torch.float32 else 4) + 4 + (dx.element_size() if dres is not None else 0) +
                                      dx.element_size() + (2 if dx_bf16 is not None else 0))
        _ln_profile.append((nbytes, e0, e1))


def patch_im2col(images, patches, patch, cin):
    n, _, H, W = images.shape
    check(lib().reid_patch_im2col(ptr(images), ptr(patches), n, H, W, patch, cin, stream_ptr()))


def cls_rows(cls, pos0, x, n_img, tokens):
    check(lib().reid_cls_rows(ptr(cls), ptr(pos0), ptr(x), x.stride(0), n_img, tokens, x.shape[1], stream_ptr()))


def attn_fwd(qkv, out, lse, n_seq, S, heads, causal=False, key_mask=None, q_tiles=0):
    check(lib().reid_attn_fwd(ptr(qkv), qkv.stride(0), ptr(key_mask), ptr(out), out.stride(0), ptr(lse), n_seq, S, heads,
                              int(causal), int(q_tiles), stream_ptr()))


def attn_bwd(qkv, out, dout, lse, dqkv, delta_ws, n_seq, S, heads, causal=False, key_mask=None, q_tiles=0):
    check(lib().reid_attn_bwd(ptr(qkv), qkv.stride(0), ptr(key_mask), ptr(out), ptr(dout), out.stride(0), ptr(lse),
                              ptr(dqkv), dqkv.stride(0), ptr(delta_ws), n_seq, S, heads, int(causal), int(q_tiles), stream_ptr()))


def cast_f32_bf16(src, dst):
    check(lib().reid_cast_f32_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()))
    return dst


def cast_bf16_f32(src, dst):
    """dst (f32) = the values of the flavor's 16-bit ``src``, exactly."""
    check(lib().reid_cast_bf16_f32(ptr(src), ptr(dst), src.numel(), stream_ptr()))
    return dst


def lora_bwd_fused(dY, T, BT, U, dB, img_mod, rows_per_img, mask_r, scale, u_partial=None):
    """U = mask(dY . B) * scale and dB += dY^T . T from one pass over dY (Rp = 32, or 64 with ``rows_per_img`` >= 32 and ``mask_r`` a
    divisor of 16; N = 768, or a multiple of 768 as column blocks with the fp32 scratch ``u_partial`` [M, Rp]); see reid_lora_bwd_fused."""
    N = dY.shape[1]
    nb = N // 768
    if nb > 1 and u_partial is None:
        raise ValueError('lora_bwd_fused: a cotangent wider than 768 columns needs u_partial')
    for q in range(nb):
        mode = 0 if nb == 1 else ((1 if q > 0 else 0) | (2 if q + 1 < nb else 0))
        dYq, BTq, dBq = dY[:, q * 768:(q + 1) * 768], BT[:, q * 768:(q + 1) * 768], dB[q * 768:(q + 1) * 768]
        check(lib().reid_lora_bwd_fused(ptr(dYq), dYq.stride(0), ptr(T), T.stride(0), ptr(BTq), BTq.stride(0), ptr(U), U.stride(0),
                                        ptr(dBq), dBq.stride(0), ptr(img_mod), rows_per_img, mask_r, dY.shape[0], 768, T.shape[1],
                                        scale, ptr(u_partial), mode, stream_ptr()))


def lora_da_fused(X, U, dA, img_mod, rows_per_img, mask_r, n_groups=1):
    """dA += U^T . X for the adapter groups of one MERLinear, one pass over X (one image per workgroup); see reid_lora_da_fused."""
    check(lib().reid_lora_da_fused(ptr(X), X.stride(0), ptr(U), U.stride(0), ptr(dA), dA.stride(0), ptr(img_mod), rows_per_img, mask_r,
                                   X.shape[0], X.shape[1], U.shape[1] // n_groups, n_groups, stream_ptr()))


def lora_da_fused_ok(K, Rp, rows_per_img, mask_r, n_groups):
    """Whether reid_lora_da_fused takes this shape: Rp = 32 or 64 adapter columns per group, images of at least one 32-row step."""
    return K % 768 == 0 and Rp in (32, 64) and rows_per_img >= 32 and mask_r <= 16 and 16 % mask_r == 0 and n_groups in (1, 3)


def lora_bwd_fused_ok(N, Rp, rows_per_img=None, mask_r=None):
    """Whether reid_lora_bwd_fused takes this shape.  Rp = 32: any rows_per_img / mask_r (the slab kernel takes what the image kernel
    does not).  Rp = 64: the image kernel only, which needs ``rows_per_img`` >= 32 and ``mask_r`` a divisor of 16."""
    if N % 768 != 0 or N // 768 not in (1, 2, 3, 4):
        return False
    if Rp == 32:
        return True
    return Rp == 64 and rows_per_img is not None and mask_r is not None and rows_per_img >= 32 and 0 < mask_r <= 16 and 16 % mask_r == 0


def merge_lora_table(table, n_entries, max_tiles, arena, weff, Rp, r, nmod, scaling):
    check(lib().reid_merge_lora_table(ptr(table), n_entries, max_tiles, ptr(arena), ptr(weff), Rp, r, nmod, scaling, stream_ptr()))


def to_bf16(src: torch.Tensor) -> torch.Tensor:
    """New bf16 tensor with the values of fp32 ``src`` (round-to-nearest-even, HIP kernel)."""
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=L.t16(), device=src.device)
    if src.numel():
        cast_f32_bf16(src, dst)
    return dst


def pack_bf16_table(src_arena, dst_arena, table, n_entries):
    check(lib().reid_pack_bf16_table(ptr(src_arena), ptr(dst_arena), ptr(table), n_entries, stream_ptr()))


to_t16 = to_bf16


def l2norm_rows(x, y=None, y_bf16=None, eps=1e-12, scale=1.0):
    o = y if y is not None else y_bf16
    check(lib().reid_l2norm_rows(ptr(x), x.stride(0), ptr(y), ptr(y_bf16), o.stride(0), x.shape[0], x.shape[1],
                                 eps, scale, stream_ptr()))


def sgemm(A, B, C_out, *, ta=False, tb=False, alpha=1.0, beta=0.0, bias=None, act='none'):
    """fp32 C = act(alpha * op(A) @ op(B) + bias) + beta*C on the vector ALU (small head GEMMs, exact fp32)."""
    M = A.shape[1] if ta else A.shape[0]
    K = A.shape[0] if ta else A.shape[1]
    N = B.shape[0] if tb else B.shape[1]
    sam, sak = (1, A.stride(0)) if ta else (A.stride(0), 1)
    sbk, sbn = (1, B.stride(0)) if tb else (B.stride(0), 1)
    check(lib().reid_sgemm(ptr(A), ptr(B), ptr(C_out), M, N, K, sam, sak, sbk, sbn, C_out.stride(0), alpha, beta, ptr(bias),
                           ACT[act], stream_ptr()))
    return C_out


# ----------------------------------------------------------------------------------------- head
def bnneck_stats(x, sum_, sqsum):
    check(lib().reid_bnneck_stats(ptr(x), x.stride(0), x.shape[0], x.shape[1], ptr(sum_), ptr(sqsum), stream_ptr()))


def bnneck_fwd(x, gamma, beta, running_mean, running_var, sum_, sqsum, count, training, y, y_bf16, mean, invstd, rnorm,
               eps=1e-5, momentum=0.1, scale=8.0):
    check(lib().reid_bnneck_fwd(ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(sum_),
                                ptr(sqsum), count, int(training), ptr(y), ptr(y_bf16), y.stride(0), ptr(mean),
                                ptr(invstd), ptr(rnorm), x.shape[0], x.shape[1], eps, momentum, scale, stream_ptr()))


def bnneck_bwd_p1(dy, x, gamma, beta, mean, invstd, rnorm, dz, sum_dz, sum_dz_xhat, scale=8.0):
    check(lib().reid_bnneck_bwd_p1(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                   ptr(rnorm), ptr(dz), ptr(sum_dz), ptr(sum_dz_xhat), x.shape[0], x.shape[1],
                                   scale, stream_ptr()))


def bnneck_bwd_p2(dz, x, gamma, mean, invstd, sum_dz, sum_dz_xhat, count, training, dx):
    check(lib().reid_bnneck_bwd_p2(ptr(dz), ptr(x), x.stride(0), ptr(gamma), ptr(mean), ptr(invstd), ptr(sum_dz),
                                   ptr(sum_dz_xhat), count, int(training), ptr(dx), dx.stride(0), x.shape[0],
                                   x.shape[1], stream_ptr()))


def ce_ls_fwd(logits, labels, valid, row_loss, loss_sum, smoothing=0.1):
    check(lib().reid_ce_ls_fwd(ptr(logits), logits.stride(0), ptr(labels), ptr(valid), logits.shape[0], logits.shape[1],
                               smoothing, ptr(row_loss), ptr(loss_sum), stream_ptr()))


def ce_ls_bwd(logits, labels, valid, grad_scale, dlogits, smoothing=0.1):
    check(lib().reid_ce_ls_bwd(ptr(logits), logits.stride(0), ptr(labels), ptr(valid), logits.shape[0], logits.shape[1],
                               smoothing, ptr(grad_scale), ptr(dlogits), dlogits.stride(0), stream_ptr()))


def sdm_ws_floats(P, N, Mg, D):
    return int(lib().reid_sdm_ws_floats(P, N, Mg, D))


def sdm_fwd(q, g, q_label, g_label, q_valid, g_valid, tau, ws, result, P=1):
    """q [P*N, D] (P query sides stacked), g [Mg, D]; result f32 [2*P] = (loss, contributes) per pair."""
    N = q.shape[0] // P
    check(lib().reid_sdm_fwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_label), ptr(g_label), ptr(q_valid), ptr(g_valid),
                             P, N, g.shape[0], q.shape[1], tau, ptr(ws), ptr(result), stream_ptr()))


def sdm_bwd(q, g, q_label, g_label, q_valid, g_valid, tau, ws, gscale, dq, dg, P=1):
    N = q.shape[0] // P
    check(lib().reid_sdm_bwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_label), ptr(g_label), ptr(q_valid), ptr(g_valid),
                             P, N, g.shape[0], q.shape[1], tau, ptr(ws), ptr(gscale), ptr(dq), dq.stride(0),
                             ptr(dg), dg.stride(0), stream_ptr()))


# ----------------------------------------------------------------------------------------- losses
# What the C side cannot see of a tensor (dtype, numel, contiguity) every wrapper below checks with these helpers.
f32, f64, i32, i64, u8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def _f32_matrices(who, text, *named):
    """Every (name, tensor, shape) of ``named``: a 2-d fp32 device tensor of that shape (None: any extent) with unit column stride."""
    for n, t, shape in named:
        L._req(t, f32, n)
        if t.dim() != 2 or any(want is not None and want != got for want, got in zip(shape, t.shape)):
            raise ValueError(f'{who}: {text}')


def _stacked_rows(who, text, name, t, S):
    """(N, D) of the fp32 matrix ``t`` [S*N, D] of S stacked sides."""
    _f32_matrices(who, text, (name, t, (None, None)))
    if S < 1 or t.shape[0] % S:
        raise ValueError(f'{who}: {text}')
    return t.shape[0] // S, t.shape[1]


def _vectors(who, text, *named, exact=False):
    """Every (name, tensor, dtype, numel) of ``named``: a contiguous device tensor of ``dtype`` with at least (``exact``: exactly)
    that many elements."""
    for n, t, dtype, count in named:
        L._req(t, dtype, n)
        if (t.numel() != count if exact else t.numel() < count) or not t.is_contiguous():
            raise ValueError(f'{who}: {text}')


def _valid_bytes(who, name, t, n):
    """An optional validity vector: None, or contiguous uint8 of exactly ``n`` elements."""
    if t is not None:
        _vectors(who, f'{name} has {t.numel()} elements where {n} contiguous ones are expected', (name, t, u8, n), exact=True)


def _ws_floats(fn, *dims):
    n = int(fn(*dims))
    if n < 0:
        check(n)
    return n


def _pair_grads(who, q, g, gscale, dq, dg, P):
    """What the two-sided backwards write: dq as q, dg as g, from gscale f32 [P]."""
    text = 'dq as q, dg as g, gscale [P]'
    _f32_matrices(who, text, ('dq', dq, q.shape), ('dg', dg, g.shape))
    _vectors(who, text, ('gscale', gscale, f32, P))


def _mined_saved(who, q_d, q_idx, g_d, g_idx, ws, result, P, N, Mg, ws_floats):
    """What a mining forward leaves for its backward: (d_ap | d_an), (idx_p | idx_n) of the q and of the g anchors, result [P, 4] and
    ws of the ``ws_floats`` floats the loss's *_ws_floats function asks."""
    _vectors(who, 'q_d / q_idx [2, P*N], g_d / g_idx [2, P*Mg], result [P, 4], all contiguous', ('q_d', q_d, f32, 2 * P * N),
             ('q_idx', q_idx, i32, 2 * P * N), ('g_d', g_d, f32, 2 * P * Mg), ('g_idx', g_idx, i32, 2 * P * Mg), ('result', result, f32, 4 * P))
    _vectors(who, f'ws holds fewer than the {ws_floats} floats of its *_ws_floats', ('ws', ws, f32, ws_floats))


def _triplet_hard_checks(who, text, x, d_ap, d_an, idx_p, idx_n, result):
    _f32_matrices(who, text, ('x', x, (None, None)))
    B = x.shape[0]
    _vectors(who, text, ('d_ap', d_ap, f32, B), ('d_an', d_an, f32, B), ('idx_p', idx_p, i32, B), ('idx_n', idx_n, i32, B), ('result', result, f32, 2))
    return B


def triplet_hard_fwd(x, labels, valid, margin, d_ap, d_an, idx_p, idx_n, row_loss, result):
    """Batch-hard triplet loss of x [B, D] f32; margin < 0 selects the soft-margin form; result f32 [2] = (loss, n_active)."""
    who, text = 'triplet_hard_fwd', 'x [B, D], labels [B], per-row outputs [B], result [2]'
    B = _triplet_hard_checks(who, text, x, d_ap, d_an, idx_p, idx_n, result)
    _vectors(who, text, ('labels', labels, i64, B), exact=True)
    _vectors(who, text, ('row_loss', row_loss, f32, B))
    _valid_bytes(who, 'valid', valid, B)
    check(lib().reid_triplet_hard_fwd(ptr(x), x.stride(0), ptr(labels), ptr(valid), B, x.shape[1], margin, ptr(d_ap), ptr(d_an),
                                      ptr(idx_p), ptr(idx_n), ptr(row_loss), ptr(result), stream_ptr()))


def triplet_hard_bwd(x, margin, d_ap, d_an, idx_p, idx_n, result, dloss, dx):
    """dx [B, D] = dloss * d loss / dx from the arrays triplet_hard_fwd saved (overwritten, one launch); dloss a device scalar."""
    who, text = 'triplet_hard_bwd', 'x and dx [B, D], per-row arrays [B], result [2], dloss [1]'
    B = _triplet_hard_checks(who, text, x, d_ap, d_an, idx_p, idx_n, result)
    _f32_matrices(who, text, ('dx', dx, x.shape))
    _vectors(who, text, ('dloss', dloss, f32, 1))
    check(lib().reid_triplet_hard_bwd(ptr(x), x.stride(0), B, x.shape[1], margin, ptr(d_ap), ptr(d_an), ptr(idx_p), ptr(idx_n),
                                      ptr(result), ptr(dloss), ptr(dx), dx.stride(0), stream_ptr()))


def cross_triplet_ws_floats(P, N, Mg, D):
    return _ws_floats(lib().reid_cross_triplet_ws_floats, P, N, Mg, D)


def hc_triplet_ws_floats(P, N, Mg, D):
    return _ws_floats(lib().reid_hc_triplet_ws_floats, P, N, Mg, D)


def _pair_batch(who, q, g, q_valid, g_valid, P):
    """q [P*N, D] (P query sides stacked) against g [Mg, D] with their optional validity vectors; returns (N, Mg, D)."""
    text = 'q [P*N, D], g [Mg, D]'
    N, D = _stacked_rows(who, text, 'q', q, P)
    _f32_matrices(who, text, ('g', g, (None, D)))
    _valid_bytes(who, 'q_valid', q_valid, P * N); _valid_bytes(who, 'g_valid', g_valid, g.shape[0])
    return N, g.shape[0], D


def cross_triplet_fwd(q, g, q_label, g_label, q_valid, g_valid, margin, normalize, eps, q_d, q_idx, g_d, g_idx, ws, result, P=1):
    """Cross-modal batch-hard triplet loss: q [P*N, D] (P query sides stacked) against g [Mg, D], mined in both directions; margin < 0
    selects the soft-margin form.  q_d / q_idx [2, P*N] = (d_ap | d_an), (idx_p | idx_n) of the q anchors, g_d / g_idx [2, P*Mg] of the
    g anchors (indices pair-local); result f32 [P, 4] = (L_p, flag_p, n_qg, n_gq); ws is kept for cross_triplet_bwd."""
    N, Mg, D = _pair_batch('cross_triplet_fwd', q, g, q_valid, g_valid, P)
    _mined_saved('cross_triplet_fwd', q_d, q_idx, g_d, g_idx, ws, result, P, N, Mg, cross_triplet_ws_floats(P, N, Mg, D))
    _vectors('cross_triplet_fwd', 'q_label [N], g_label [Mg]', ('q_label', q_label, i64, N), ('g_label', g_label, i64, Mg), exact=True)
    check(lib().reid_cross_triplet_fwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_label), ptr(g_label), ptr(q_valid), ptr(g_valid),
                                       P, N, Mg, D, margin, int(normalize), eps, ptr(q_d), ptr(q_idx), ptr(g_d), ptr(g_idx),
                                       ptr(ws), ptr(result), stream_ptr()))


def cross_triplet_bwd(q, g, q_valid, g_valid, margin, normalize, eps, q_d, q_idx, g_d, g_idx, ws, result, gscale, dq, dg, P=1):
    """dq [P*N, D], dg [Mg, D] (both overwritten, one launch) from what cross_triplet_fwd saved; gscale f32 [P] on the device."""
    N, Mg, D = _pair_batch('cross_triplet_bwd', q, g, q_valid, g_valid, P)
    _mined_saved('cross_triplet_bwd', q_d, q_idx, g_d, g_idx, ws, result, P, N, Mg, cross_triplet_ws_floats(P, N, Mg, D))
    _pair_grads('cross_triplet_bwd', q, g, gscale, dq, dg, P)
    check(lib().reid_cross_triplet_bwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_valid), ptr(g_valid), P, N, Mg, D, margin,
                                       int(normalize), eps, ptr(q_d), ptr(q_idx), ptr(g_d), ptr(g_idx), ptr(ws), ptr(result), ptr(gscale),
                                       ptr(dq), dq.stride(0), ptr(dg), dg.stride(0), stream_ptr()))


def _hc_triplet_saved(who, lead, count, ws, result, P, N, Mg, D):
    _vectors(who, 'lead / count [P*N + Mg], result [P, 4], all contiguous', ('lead', lead, i32, P * N + Mg), ('count', count, i32, P * N + Mg),
             ('result', result, f32, 4 * P))
    _vectors(who, 'ws holds fewer than hc_triplet_ws_floats(P, N, Mg, D) floats', ('ws', ws, f32, hc_triplet_ws_floats(P, N, Mg, D)))


def hc_triplet_fwd(q, g, q_label, g_label, q_valid, g_valid, margin, normalize, eps, lead, count, clabel, d, idx, ws, result, P=1):
    """Hetero-center triplet loss: q [P*N, D] (P query sides stacked) against g [Mg, D], the triplet on the per-identity centres of
    every side; margin < 0 selects the soft-margin form.  lead i32 [P*N + Mg] per row, count i32 / clabel i64 [P*N + Mg] per centre
    slot; d f32 / idx i32 [2, P, N + Mg] = (d_ap | d_an), (idx_p | idx_n) in the index space (q centre s -> s, g centre t -> N + t);
    result f32 [P, 4] = (L_p, flag_p, n_q, n_g); ws is kept for hc_triplet_bwd."""
    N, Mg, D = _pair_batch('hc_triplet_fwd', q, g, q_valid, g_valid, P)
    _hc_triplet_saved('hc_triplet_fwd', lead, count, ws, result, P, N, Mg, D)
    _vectors('hc_triplet_fwd', 'q_label [N], g_label [Mg]', ('q_label', q_label, i64, N), ('g_label', g_label, i64, Mg), exact=True)
    _vectors('hc_triplet_fwd', 'clabel [P*N + Mg], d / idx [2, P, N + Mg], all contiguous', ('clabel', clabel, i64, P * N + Mg),
             ('d', d, f32, 2 * P * (N + Mg)), ('idx', idx, i32, 2 * P * (N + Mg)))
    check(lib().reid_hc_triplet_fwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_label), ptr(g_label), ptr(q_valid), ptr(g_valid),
                                    P, N, Mg, D, margin, int(normalize), eps, ptr(lead), ptr(count), ptr(clabel), ptr(d), ptr(idx),
                                    ptr(ws), ptr(result), stream_ptr()))


def hc_triplet_bwd(q, g, margin, normalize, eps, lead, count, ws, result, gscale, dq, dg, P=1):
    """dq [P*N, D], dg [Mg, D] (both overwritten, two launches) from what hc_triplet_fwd saved; gscale f32 [P] on the device."""
    N, Mg, D = _pair_batch('hc_triplet_bwd', q, g, None, None, P)
    _hc_triplet_saved('hc_triplet_bwd', lead, count, ws, result, P, N, Mg, D)
    _pair_grads('hc_triplet_bwd', q, g, gscale, dq, dg, P)
    check(lib().reid_hc_triplet_bwd(ptr(q), q.stride(0), ptr(g), g.stride(0), P, N, Mg, D, margin, int(normalize), eps,
                                    ptr(lead), ptr(count), ptr(ws), ptr(result), ptr(gscale), ptr(dq), dq.stride(0), ptr(dg), dg.stride(0),
                                    stream_ptr()))


def xbm_ws_floats(P, N, M, D):
    return _ws_floats(lib().reid_xbm_ws_floats, P, N, M, D)


def _xbm_batch(who, q, g, q_valid, g_valid, P):
    """q [P*N, D] against g [N, D], the SAME N instances, with their optional validity vectors; returns (N, D)."""
    N, Mg, D = _pair_batch(who, q, g, q_valid, g_valid, P)
    if N != Mg:
        raise ValueError(f'{who}: q [P*N, D], g [N, D]')
    return N, D


def _xbm_memory(who, rows, mem_labels, mem_valid, P, N, D):
    """A cross-batch memory against a batch: rows f32 [P+1, M, D], mem_labels i64 [M], mem_valid u8 [P+1, M], all contiguous, with
    room for the N rows.  Returns M."""
    L._req(rows, f32, 'rows')
    if rows.dim() != 3 or rows.shape[0] != P + 1 or rows.shape[2] != D:
        raise L.ReidHipError(f'{who}: the memory holds rows {tuple(rows.shape)}, the batch needs [{P + 1}, M, {D}]')
    M, text = rows.shape[1], 'rows [P+1, M, D], mem_labels [M], mem_valid [P+1, M], all contiguous'
    _vectors(who, text, ('rows', rows, f32, 0), ('mem_labels', mem_labels, i64, M), ('mem_valid', mem_valid, u8, (P + 1) * M))
    if mem_labels.shape != (M,) or mem_valid.shape != (P + 1, M):
        raise ValueError(f'{who}: {text}')
    if N > M:
        raise ValueError(f'{who}: a batch of N={N} rows does not fit a memory of M={M} slots')
    return M


def xbm_enqueue(q, g, labels, q_valid, g_valid, normalize, eps, rows, mem_labels, mem_valid, cursor, P=1):
    """Files the batch q [P*N, D], g [N, D], labels [N] into the cross-batch memory (rows [P+1, M, D], mem_labels [M], mem_valid
    [P+1, M], cursor i32 [2], side 0 = g) at the device-side cursor and advances it by N; unit rows when ``normalize``."""
    N, D = _xbm_batch('xbm_enqueue', q, g, q_valid, g_valid, P)
    M = _xbm_memory('xbm_enqueue', rows, mem_labels, mem_valid, P, N, D)
    _vectors('xbm_enqueue', 'labels [N], cursor [2]', ('labels', labels, i64, N), ('cursor', cursor, i32, 2), exact=True)
    check(lib().reid_xbm_enqueue(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(labels), ptr(q_valid), ptr(g_valid), P, N, M, D,
                                 int(normalize), eps, ptr(rows), ptr(mem_labels), ptr(mem_valid), ptr(cursor), stream_ptr()))


def xbm_triplet_fwd(q, g, labels, q_valid, g_valid, margin, normalize, eps, rows, mem_labels, mem_valid, q_d, q_idx, g_d, g_idx, ws,
                    result, P=1):
    """Cross-modal batch-hard triplet loss of the batch against the cross-batch memory as it stands: the q rows of pair p against the
    slots of side 0, the g rows against the slots of side p + 1; margin < 0 selects the soft-margin form.  q_d / q_idx, g_d / g_idx
    [2, P*N] = (d_ap | d_an), (idx_p | idx_n) as SLOT numbers; result f32 [P, 4] = (L_p, flag_p, n_q, n_g); ws is kept for
    xbm_triplet_bwd, with copies of the kept rows."""
    N, D = _xbm_batch('xbm_triplet_fwd', q, g, q_valid, g_valid, P)
    M = _xbm_memory('xbm_triplet_fwd', rows, mem_labels, mem_valid, P, N, D)
    _mined_saved('xbm_triplet_fwd', q_d, q_idx, g_d, g_idx, ws, result, P, N, N, xbm_ws_floats(P, N, M, D))
    _vectors('xbm_triplet_fwd', 'labels [N]', ('labels', labels, i64, N), exact=True)
    check(lib().reid_xbm_triplet_fwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(labels), ptr(q_valid), ptr(g_valid), P, N, M, D,
                                     margin, int(normalize), eps, ptr(rows), ptr(mem_labels), ptr(mem_valid), ptr(q_d), ptr(q_idx),
                                     ptr(g_d), ptr(g_idx), ptr(ws), ptr(result), stream_ptr()))


def xbm_triplet_bwd(q, g, q_valid, g_valid, margin, normalize, eps, q_d, q_idx, g_d, g_idx, ws, result, gscale, dq, dg, P=1):
    """dq [P*N, D], dg [N, D] (both overwritten, one launch) from what xbm_triplet_fwd saved -- the memory itself is not read;
    gscale f32 [P] on the device."""
    N, D = _xbm_batch('xbm_triplet_bwd', q, g, q_valid, g_valid, P)
    _mined_saved('xbm_triplet_bwd', q_d, q_idx, g_d, g_idx, ws, result, P, N, N, xbm_ws_floats(P, N, N, D))
    _pair_grads('xbm_triplet_bwd', q, g, gscale, dq, dg, P)
    check(lib().reid_xbm_triplet_bwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_valid), ptr(g_valid), P, N, D, margin, int(normalize),
                                     eps, ptr(q_d), ptr(q_idx), ptr(g_d), ptr(g_idx), ptr(ws), ptr(result), ptr(gscale), ptr(dq),
                                     dq.stride(0), ptr(dg), dg.stride(0), stream_ptr()))


def center_ws_floats(S, N, D):
    return _ws_floats(lib().reid_center_ws_floats, S, N, D)


def _center_batch(who, labels, valid, S, N):
    _vectors(who, 'labels [N], contiguous', ('labels', labels, i64, N), exact=True)
    _valid_bytes(who, 'valid', valid, S * N)


def _center_table(who, centers, D=None):
    """centers f32 [C, D], contiguous; a table of another D than the batch's is refused.  Returns its D."""
    text = 'centers [C, D], contiguous'
    _f32_matrices(who, text, ('centers', centers, (None, None)))
    _vectors(who, text, ('centers', centers, f32, 0))
    if D is not None and centers.shape[1] != D:
        raise L.ReidHipError(f'{who}: the table holds centres of D={centers.shape[1]}, the batch has D={D}')
    return centers.shape[1]


def center_fwd(x, labels, valid, centers, ws, d2, result, S=1):
    """Center loss of x [S*N, D] (S sides stacked, labels [N] shared) against the table centers [C, D]: ws receives diff = x - c_y (kept
    for center_update and center_bwd), d2 [S*N] the squared distances, result f32 [2] = (0.5 * mean d2 over the used rows, n_used)."""
    N, D = _stacked_rows('center_fwd', 'x [S*N, D]', 'x', x, S)
    _center_batch('center_fwd', labels, valid, S, N)
    _center_table('center_fwd', centers, D)
    _vectors('center_fwd', 'ws [center_ws_floats(S, N, D)], d2 [S*N], result [2], all contiguous', ('ws', ws, f32, center_ws_floats(S, N, D)),
             ('d2', d2, f32, S * N), ('result', result, f32, 2))
    check(lib().reid_center_fwd(ptr(x), x.stride(0), ptr(labels), ptr(valid), S, N, D, ptr(centers), centers.shape[0], ptr(ws), ptr(d2),
                                ptr(result), stream_ptr()))


def center_update(labels, valid, d2, ws, centers, alpha, S=1):
    """Wen's update of the centres center_fwd has just used, in place: c_j -= alpha * sum(c_j - x_r) / (1 + n_j) over the rows of class
    j that are used and have a finite d2 (one launch, no atomics); rows of classes not in the batch keep their bits."""
    N = labels.numel()
    _center_batch('center_update', labels, valid, S, N)
    D = _center_table('center_update', centers)
    _vectors('center_update', 'ws [center_ws_floats(S, N, D)], d2 [S*N], all contiguous', ('ws', ws, f32, center_ws_floats(S, N, D)), ('d2', d2, f32, S * N))
    check(lib().reid_center_update(ptr(labels), ptr(valid), S, N, D, ptr(d2), ptr(ws), ptr(centers), centers.shape[0], float(alpha),
                                   stream_ptr()))


def center_bwd(ws, result, dloss, dx, S=1):
    """dx [S*N, D] = dloss / max(1, n_used) * diff from what center_fwd saved (overwritten, one launch) -- the table itself is not read;
    dloss a device scalar."""
    N, D = _stacked_rows('center_bwd', 'dx [S*N, D]', 'dx', dx, S)
    _vectors('center_bwd', 'ws [center_ws_floats(S, N, D)], result [2], dloss [1], all contiguous', ('ws', ws, f32, center_ws_floats(S, N, D)),
             ('result', result, f32, 2), ('dloss', dloss, f32, 1))
    check(lib().reid_center_bwd(S, N, D, ptr(ws), ptr(result), ptr(dloss), ptr(dx), dx.stride(0), stream_ptr()))


def cluster_nce_ws_floats(S, N, D, K):
    return _ws_floats(lib().reid_cluster_nce_ws_floats, S, N, D, K)


def cluster_nce_plan(R, K, D):
    """(row tile, class tile, splits, class tiles per split) of the forward of R rows against K centroids of D columns: the rule
    depends on the shape only.  Nothing is launched."""
    plan = (C.c_int32 * 4)()
    check(lib().reid_cluster_nce_plan(R, K, D, C.cast(plan, C.c_void_p)))
    return tuple(plan)


def _cluster_table(who, table, D=None):
    """table f32 [K, D], contiguous; a table of another D than the batch's is refused.  Returns its D."""
    text = 'table [K, D], contiguous'
    _f32_matrices(who, text, ('table', table, (None, None)))
    _vectors(who, text, ('table', table, f32, 0))
    if D is not None and table.shape[1] != D:
        raise L.ReidHipError(f'{who}: the memory holds centroids of D={table.shape[1]}, the batch has D={D}')
    return table.shape[1]


def cluster_nce_fwd(x, labels, valid, table, tau, with_grad, ws, row_loss, target_cos, result, S=1):
    """ClusterNCE of x [S*N, D] (S sides stacked, labels [N] shared) against the unit centroids table [K, D]: row_loss / target_cos
    [S*N] = lse - l_y and x^ . C_y of the used rows (others 0), result f32 [2] = (mean row loss over the used rows, n_used).
    ``with_grad``: the table is streamed a second time and ws keeps what cluster_nce_bwd needs; ws also holds x^ for cluster_nce_update."""
    N, D = _stacked_rows('cluster_nce_fwd', 'x [S*N, D]', 'x', x, S)
    _center_batch('cluster_nce_fwd', labels, valid, S, N)
    _cluster_table('cluster_nce_fwd', table, D)
    K = table.shape[0]
    _vectors('cluster_nce_fwd', 'ws [cluster_nce_ws_floats(S, N, D, K)], row_loss / target_cos [S*N], result [2], all contiguous',
             ('ws', ws, f32, cluster_nce_ws_floats(S, N, D, K)), ('row_loss', row_loss, f32, S * N), ('target_cos', target_cos, f32, S * N),
             ('result', result, f32, 2))
    check(lib().reid_cluster_nce_fwd(ptr(x), x.stride(0), ptr(labels), ptr(valid), S, N, D, ptr(table), K, float(tau), int(bool(with_grad)),
                                     ptr(ws), ptr(row_loss), ptr(target_cos), ptr(result), stream_ptr()))


def cluster_nce_update(labels, valid, row_loss, target_cos, ws, table, momentum, mode='mean', S=1):
    """The momentum update of the centroids cluster_nce_fwd has just used, in place (one launch, no atomics): mode 'mean' blends a
    label's contributing rows in ascending row order, 'hard' its row of the smallest target cosine; absent labels keep their bits."""
    if mode not in L.CLUSTER_NCE_MODES:
        raise ValueError(f"cluster_nce_update: mode must be 'mean' or 'hard', not {mode!r}")
    N = labels.numel()
    _center_batch('cluster_nce_update', labels, valid, S, N)
    D = _cluster_table('cluster_nce_update', table)
    _vectors('cluster_nce_update', 'ws [cluster_nce_ws_floats(S, N, D, K)], row_loss / target_cos [S*N], all contiguous',
             ('ws', ws, f32, cluster_nce_ws_floats(S, N, D, table.shape[0])), ('row_loss', row_loss, f32, S * N),
             ('target_cos', target_cos, f32, S * N))
    check(lib().reid_cluster_nce_update(ptr(labels), ptr(valid), S, N, D, ptr(row_loss), ptr(target_cos), ptr(ws), ptr(table), table.shape[0],
                                        float(momentum), L.CLUSTER_NCE_MODES[mode], stream_ptr()))


def cluster_nce_bwd(ws, result, dloss, dx, S=1):
    """dx [S*N, D] = dloss / max(1, n_used) * H from what cluster_nce_fwd(with_grad=True) saved (overwritten, one launch) -- the table
    itself is not read; dloss a device scalar."""
    N, D = _stacked_rows('cluster_nce_bwd', 'dx [S*N, D]', 'dx', dx, S)
    _vectors('cluster_nce_bwd', 'ws [cluster_nce_ws_floats(S, N, D, K)], result [2], dloss [1], all contiguous',
             ('ws', ws, f32, cluster_nce_ws_floats(S, N, D, 1)), ('result', result, f32, 2), ('dloss', dloss, f32, 1))
    check(lib().reid_cluster_nce_bwd(S, N, D, ptr(ws), ptr(result), ptr(dloss), ptr(dx), dx.stride(0), stream_ptr()))


def cluster_centroids(feats, order, offsets, table):
    """table [K, D] = the normalised fp32 mean of the rows order[offsets[k] : offsets[k + 1]] of feats [rows, D], summed in that order
    (order i64: row indices grouped by label, offsets i64 [K + 1]); one launch, one wave per cluster."""
    text = 'feats [rows, D], table [K, D] fp32; order [n], offsets [K + 1] int64'
    _f32_matrices('cluster_centroids', text, ('feats', feats, (None, None)))
    D = _cluster_table('cluster_centroids', table, feats.shape[1])
    K = table.shape[0]
    _vectors('cluster_centroids', text, ('order', order, i64, 0), ('offsets', offsets, i64, K + 1))
    if offsets.numel() != K + 1:
        raise ValueError(f'cluster_centroids: {text}')
    check(lib().reid_cluster_centroids(ptr(feats), feats.stride(0), feats.shape[0], ptr(order), ptr(offsets), K, D, ptr(table), stream_ptr()))


def _hybrid_memory(who, entries, order, offsets, table):
    """The hybrid memory as the kernels see it: entries f32 [M, D] (unit column stride), order i64 [M] and offsets i64 [C + 1]
    contiguous (the members of every class, ascending), table f32 [C, D] contiguous.  Returns (M, C, D)."""
    text = 'entries [M, D], table [C, D] fp32; order [M], offsets [C + 1] int64, contiguous'
    _f32_matrices(who, text, ('entries', entries, (None, None)))
    D = _cluster_table(who, table, entries.shape[1])
    M, C_ = entries.shape[0], table.shape[0]
    _vectors(who, text, ('order', order, i64, M), ('offsets', offsets, i64, C_ + 1), exact=True)
    return M, C_, D


def class_means(entries, order, offsets, table):
    """table [C, D] = the fp32 mean of the rows order[offsets[c] : offsets[c + 1]] of entries [M, D], added one by one in that order
    and divided by their count -- not renormalised (the hybrid memory's class vectors); one launch, one workgroup per class."""
    M, C_, D = _hybrid_memory('class_means', entries, order, offsets, table)
    check(lib().reid_class_means(ptr(entries), entries.stride(0), M, ptr(order), ptr(offsets), C_, D, ptr(table), stream_ptr()))


def hybrid_update_instances(index, valid, row_loss, ws, entries, momentum, S=1):
    """The momentum update of the instance entries [M, D] of the rows cluster_nce_fwd has just used (``index`` [N]: the dataset row
    of each instance), in place: v <- m v + (1 - m) x^_r, renormalised, over an instance's contributing rows in ascending row order
    (one launch, no atomics); other entries keep their bits."""
    N = index.numel()
    _center_batch('hybrid_update_instances', index, valid, S, N)
    _f32_matrices('hybrid_update_instances', 'entries [M, D]', ('entries', entries, (None, None)))
    M, D = entries.shape
    _vectors('hybrid_update_instances', 'ws [cluster_nce_ws_floats(S, N, D, C)], row_loss [S*N], all contiguous',
             ('ws', ws, f32, cluster_nce_ws_floats(S, N, D, 1)), ('row_loss', row_loss, f32, S * N))
    check(lib().reid_hybrid_update_instances(ptr(index), ptr(valid), S, N, D, ptr(row_loss), ptr(ws), ptr(entries), entries.stride(0), M,
                                             float(momentum), stream_ptr()))


def hybrid_refresh_classes(labels, valid, row_loss, entries, order, offsets, table, S=1):
    """Re-forms, from the entries as they stand, the class means of the classes with a contributing row (``labels`` [N]: the gathered
    class labels cluster_nce_fwd had), in place (one launch, no atomics); the other rows of the table keep their bits."""
    N = labels.numel()
    _center_batch('hybrid_refresh_classes', labels, valid, S, N)
    M, C_, D = _hybrid_memory('hybrid_refresh_classes', entries, order, offsets, table)
    _vectors('hybrid_refresh_classes', 'row_loss [S*N], contiguous', ('row_loss', row_loss, f32, S * N))
    check(lib().reid_hybrid_refresh_classes(ptr(labels), ptr(valid), S, N, D, ptr(row_loss), ptr(entries), entries.stride(0), M, ptr(order),
                                            ptr(offsets), ptr(table), C_, stream_ptr()))


def smooth_ap_ws_floats(P, N, Mg, D, Ga, Gb, with_grad):
    return _ws_floats(lib().reid_smooth_ap_ws_floats, P, N, Mg, D, Ga, Gb, int(bool(with_grad)))


def smooth_ap_fwd(q, g, q_label, g_label, q_valid, g_valid, tau, normalize, eps, with_grad, q_ap, q_npos, g_ap, g_npos, ws, result, P=1,
                  ring=None):
    """Cross-modal Smooth-AP: q [P*N, D] (P query sides stacked) against g [Mg, D], ranked in both directions.  ``ring`` None: inside the
    batch (the galleries are g and pair p's q rows, and get a gradient); ``ring`` = (rows [P+1, M, D], mem_labels [M], mem_valid
    [P+1, M]) of a cross-batch memory: the q rows rank the slots of side 0, the g rows those of side p + 1, as constants (then Mg = N).
    q_ap / q_npos [P*N], g_ap / g_npos [P*Mg] = AP_a (-1: inactive), |P_a|; result f32 [P, 4] = (L_p, flag_p, n_qg, n_gq).  With
    ``with_grad`` ws keeps the projected gradients for smooth_ap_bwd."""
    who = 'smooth_ap_fwd'
    N, Mg, D = _pair_batch(who, q, g, q_valid, g_valid, P)
    _vectors(who, 'q_label [N], g_label [Mg]', ('q_label', q_label, i64, N), ('g_label', g_label, i64, Mg), exact=True)
    if ring is None:
        ga, gb = (g, g.stride(0), g_label, g_valid, Mg), (q, q.stride(0), q_label, q_valid, N)
    else:
        if N != Mg:
            raise ValueError(f'{who}: q [P*N, D], g [N, D] against a memory')
        rows, mem_labels, mem_valid = ring
        M = _xbm_memory(who, rows, mem_labels, mem_valid, P, 1, D)
        ga, gb = (rows[0], D, mem_labels, mem_valid[0], M), (rows[1:], D, mem_labels, mem_valid[1:], M)
    n_ws = smooth_ap_ws_floats(P, N, Mg, D, ga[4], gb[4], with_grad)
    _vectors(who, 'q_ap / q_npos [P*N], g_ap / g_npos [P*Mg], result [P, 4], all contiguous', ('q_ap', q_ap, f32, P * N),
             ('q_npos', q_npos, i32, P * N), ('g_ap', g_ap, f32, P * Mg), ('g_npos', g_npos, i32, P * Mg), ('result', result, f32, 4 * P))
    _vectors(who, f'ws holds fewer than the {n_ws} floats of smooth_ap_ws_floats', ('ws', ws, f32, n_ws))
    check(lib().reid_smooth_ap_fwd(ptr(q), q.stride(0), ptr(g), g.stride(0), ptr(q_label), ptr(g_label), ptr(q_valid), ptr(g_valid), P, N, Mg, D,
                                   float(tau), int(normalize), eps, ptr(ga[0]), ga[1], ptr(ga[2]), ptr(ga[3]), ga[4],
                                   ptr(gb[0]), gb[1], ptr(gb[2]), ptr(gb[3]), gb[4], int(ring is None), int(bool(with_grad)),
                                   ptr(q_ap), ptr(q_npos), ptr(g_ap), ptr(g_npos), ptr(ws), ptr(result), stream_ptr()))


def smooth_ap_bwd(q_valid, g_valid, ws, gscale, dq, dg, P=1):
    """dq [P*N, D] = gscale[p] * Hq, dg [Mg, D] = sum_p gscale[p] * Hg[p] (both overwritten, one launch) from the projected gradients
    smooth_ap_fwd(with_grad=True) left at the head of ws -- neither the batch nor a memory is read; gscale f32 [P] on the device."""
    who = 'smooth_ap_bwd'
    N, Mg, D = _pair_batch(who, dq, dg, q_valid, g_valid, P)
    _vectors(who, 'gscale [P]', ('gscale', gscale, f32, P))
    _vectors(who, 'ws holds fewer floats than the projected gradients of smooth_ap_fwd(with_grad=True)', ('ws', ws, f32, (P * N + P * Mg) * D))
    check(lib().reid_smooth_ap_bwd(ptr(q_valid), ptr(g_valid), P, N, Mg, D, ptr(ws), ptr(gscale), ptr(dq), dq.stride(0), ptr(dg), dg.stride(0),
                                   stream_ptr()))


def cos_logits_fwd(x, W, scale, eps, rx, rw, logits):
    """logits [B, C] = scale * cos(x_b, W_c) of x [B, D], W [C, D] (fp32, any leading dimension); rx f64 [B], rw f64 [C] receive the
    inverse norms 1 / max(|row|, eps) and are kept for the backward.  Two launches."""
    text = 'x [B, D], W [C, D], logits [B, C] fp32; rx [B], rw [C] fp64'
    if x.dim() != 2 or W.dim() != 2:
        raise ValueError(f'cos_logits_fwd: {text}')
    (B, D), C = x.shape, W.shape[0]
    _f32_matrices('cos_logits_fwd', text, ('x', x, (B, D)), ('W', W, (C, D)), ('logits', logits, (B, C)))
    _vectors('cos_logits_fwd', text, ('rx', rx, f64, B), ('rw', rw, f64, C))
    check(lib().reid_cos_logits_fwd(ptr(x), x.stride(0), ptr(W), W.stride(0), B, C, D, scale, eps, ptr(rx), ptr(rw), ptr(logits),
                                    logits.stride(0), stream_ptr()))


def cos_logits_bwd_prep(g, x, W, rx, rw, G, H):
    """From g = dL/dlogits [B, C]: G f64 [B, D] = sum_c g_bc rw_c W_c (None: dx is not wanted) and H f64 [C, D] = sum_b g_bc rx_b x_b
    (None: dW is not wanted), fp64 sums in a fixed order.  One launch."""
    text = 'g [B, C], x [B, D], W [C, D] fp32; rx [B], rw [C], G [B, D], H [C, D] fp64, contiguous; G or H'
    if g.dim() != 2 or x.dim() != 2 or W.dim() != 2 or (G is None and H is None):
        raise ValueError(f'cos_logits_bwd_prep: {text}')
    (B, C), D = g.shape, x.shape[1]
    _f32_matrices('cos_logits_bwd_prep', text, ('g', g, (B, C)), ('x', x, (B, D)), ('W', W, (C, D)))
    _vectors('cos_logits_bwd_prep', text, ('rx', rx, f64, B), ('rw', rw, f64, C), *([('G', G, f64, B * D)] if G is not None else []),
             *([('H', H, f64, C * D)] if H is not None else []))
    check(lib().reid_cos_logits_bwd_prep(ptr(g), g.stride(0), ptr(x), x.stride(0), ptr(W), W.stride(0), ptr(rx), ptr(rw), B, C, D, ptr(G),
                                         ptr(H), stream_ptr()))


def cos_logits_bwd_fix(x, rx, G, dx, W, rw, H, dW, scale, eps):
    """dx [B, D] = scale * rx_b * (G_b - xh_b (xh_b . G_b)) and dW [C, D] = scale * rw_c * (H_c - wh_c (wh_c . H_c)): the products of
    cos_logits_bwd_prep projected through the two normalisations (rows below eps have no projection); dx or dW may be None (its
    inputs are then not looked at).  One launch."""
    text = 'x and dx [B, D], W and dW [C, D] fp32; rx [B], G [B, D], rw [C], H [C, D] fp64, contiguous; dx or dW'
    if x.dim() != 2 or W.dim() != 2 or (dx is None and dW is None):
        raise ValueError(f'cos_logits_bwd_fix: {text}')
    (B, D), C = x.shape, W.shape[0]
    _f32_matrices('cos_logits_bwd_fix', text, ('x', x, (B, D)), ('W', W, (C, D)))
    if dx is not None:
        _f32_matrices('cos_logits_bwd_fix', text, ('dx', dx, (B, D)))
        _vectors('cos_logits_bwd_fix', text, ('rx', rx, f64, B), ('G', G, f64, B * D))
    if dW is not None:
        _f32_matrices('cos_logits_bwd_fix', text, ('dW', dW, (C, D)))
        _vectors('cos_logits_bwd_fix', text, ('rw', rw, f64, C), ('H', H, f64, C * D))
    no = dx is None, dW is None
    check(lib().reid_cos_logits_bwd_fix(ptr(x), x.stride(0), None if no[0] else ptr(rx), None if no[0] else ptr(G), ptr(dx),
                                        0 if no[0] else dx.stride(0), ptr(W), W.stride(0), None if no[1] else ptr(rw),
                                        None if no[1] else ptr(H), ptr(dW), 0 if no[1] else dW.stride(0), B, C, D, scale, eps, stream_ptr()))


def _margin_ce_shapes(who, logits, labels, valid):
    _f32_matrices(who, 'logits [rows, C], labels [rows]', ('logits', logits, (None, None)))
    _vectors(who, 'logits [rows, C], labels [rows]', ('labels', labels, i64, logits.shape[0]), exact=True)
    _valid_bytes(who, 'valid', valid, logits.shape[0])
    return logits.shape


def margin_ce_fwd(logits, labels, valid, kind, scale, margin, smoothing, row_loss, result):
    """Label-smoothed CE of the margin logits of ``kind`` ('cosine' | 'cosface' | 'arcface' | 'circle') of logits [rows, C] =
    scale * cos: row_loss f32 [rows], result f32 [3] = (sum over the used rows, their count, the mean).  Two launches."""
    rows, C = _margin_ce_shapes('margin_ce_fwd', logits, labels, valid)
    _vectors('margin_ce_fwd', 'row_loss [rows], result [3]', ('row_loss', row_loss, f32, rows), ('result', result, f32, 3))
    check(lib().reid_margin_ce_fwd(ptr(logits), logits.stride(0), ptr(labels), ptr(valid), rows, C, L.MARGIN_KINDS[kind], scale, margin,
                                   smoothing, ptr(row_loss), ptr(result), stream_ptr()))


def margin_ce_bwd(logits, labels, valid, kind, scale, margin, smoothing, result, dloss, dlogits):
    """dlogits [rows, C] (overwritten, one launch) of the mean margin_ce_fwd returned; dloss a device scalar."""
    rows, C = _margin_ce_shapes('margin_ce_bwd', logits, labels, valid)
    _f32_matrices('margin_ce_bwd', 'dlogits [rows, C]', ('dlogits', dlogits, (rows, C)))
    _vectors('margin_ce_bwd', 'result [3], dloss [1]', ('result', result, f32, 3), ('dloss', dloss, f32, 1))
    check(lib().reid_margin_ce_bwd(ptr(logits), logits.stride(0), ptr(labels), ptr(valid), rows, C, L.MARGIN_KINDS[kind], scale, margin,
                                   smoothing, ptr(result), ptr(dloss), ptr(dlogits), dlogits.stride(0), stream_ptr()))


# ----------------------------------------------------------------------------------------- retrieval
def topk_ws_bytes(Nq, Ng, k):
    return int(lib().reid_topk_ws_bytes(Nq, Ng, k))


def cosine_topk(Qb, Gb, Qf, Gf, k, ws, out_idx, out_score, exclude_q=None, exclude_g=None):
    check(lib().reid_cosine_topk(ptr(Qb), ptr(Gb), ptr(Qf), ptr(Gf), Qf.shape[0], Gf.shape[0], Qf.shape[1], k,
                                 ptr(exclude_q), ptr(exclude_g), ptr(ws), ptr(out_idx), ptr(out_score), stream_ptr()))


def topk_stream_ok(Nq, Ng, D, k) -> bool:
    return bool(lib().reid_topk_stream_ok(Nq, Ng, D, k))


def topk_scan_ok(Nq, Ng, D, k):
    return bool(lib().reid_topk_scan_ok(Nq, Ng, D, k))


def topk_stream_ws_bytes(k):
    return int(lib().reid_topk_stream_ws_bytes(k))


def cosine_topk_stream(Qf, Gf, k, ws, out_idx, out_score, exclude_q=None, exclude_g=None):
    check(lib().reid_cosine_topk_stream(ptr(Qf), ptr(Gf), Qf.shape[0], Gf.shape[0], Qf.shape[1], k, ptr(exclude_q), ptr(exclude_g),
                                        ptr(ws), ptr(out_idx), ptr(out_score), stream_ptr()))


def cosine_topk_exact(Qf, Gf, k, scratch, out_idx, out_score, exclude_q=None, exclude_g=None):
    check(lib().reid_cosine_topk_exact(ptr(Qf), ptr(Gf), Qf.shape[0], Gf.shape[0], Qf.shape[1], k, ptr(exclude_q),
                                       ptr(exclude_g), ptr(scratch), ptr(out_idx), ptr(out_score), stream_ptr()))


def cosine_topk_exact_slots(Qf, Gf, k, n_slots, slots, scratch, out_idx, out_score, exclude_q=None, exclude_g=None):
    check(lib().reid_cosine_topk_exact_slots(ptr(Qf), ptr(Gf), Qf.shape[0], Gf.shape[0], Qf.shape[1], k, ptr(exclude_q), ptr(exclude_g),
                                             n_slots, ptr(slots), ptr(scratch), ptr(out_idx), ptr(out_score), stream_ptr()))


# ----------------------------------------------------------------------------------------- small fp32 head pieces
ELT = {'add': 0, 'relu': 1, 'relu_bwd': 2, 'gelu': 3, 'gelu_bwd': 4, 'mul': 5, 'nan_to_num': 6, 'keep_mask': 7}


def eltwise(op, x, y=None, out=None, alpha=1.0):
    out = torch.empty_like(x) if out is None else out
    check(lib().reid_eltwise_f32(ELT[op], ptr(x), ptr(y), ptr(out), x.numel(), alpha, stream_ptr()))
    return out


def small_attn_fwd(qkv, key_mask, out, probs, n_seq, S, heads, drop=None):
    check(lib().reid_small_attn_fwd(ptr(qkv), qkv.stride(0), ptr(key_mask), ptr(drop), ptr(out), out.stride(0), ptr(probs), n_seq, S,
                                    heads, stream_ptr()))


def small_attn_bwd(qkv, probs, dout, dqkv, n_seq, S, heads, drop=None):
    check(lib().reid_small_attn_bwd(ptr(qkv), qkv.stride(0), ptr(probs), ptr(drop), ptr(dout), dout.stride(0), ptr(dqkv),
                                    dqkv.stride(0), n_seq, S, heads, stream_ptr()))


def masked_mean(x, mask, out, B, M, D, backward=False):
    check(lib().reid_masked_mean(ptr(x), ptr(mask), ptr(out), B, M, D, int(backward), stream_ptr()))
    return out


def rank_metrics(scores, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx, Ng, max_pos, ap, rank1, npos):
    """Per-query AP / first-positive rank / #positives from fp32 score rows (reid_rank_metrics, include/reid_hip.h)."""
    check(lib().reid_rank_metrics(ptr(scores), scores.stride(0), ptr(g_pid), ptr(g_img), ptr(q_pid), ptr(q_slot),
                                  ptr(q_excl), ptr(csr_off), ptr(csr_idx), scores.shape[0], Ng, max_pos, ptr(ap), ptr(rank1), ptr(npos),
                                  stream_ptr()))


ROWS_TOPK_MAX_K = 1024        # REID_ROWS_TOPK_MAX_K: the longest list reid_rows_topk writes
METRICS_MAX_CUTOFFS = 8       # REID_METRICS_MAX_CUTOFFS
LIST_BAD_NEGATIVE, LIST_BAD_RANGE, LIST_BAD_ORDER = 1, 2, 4      # REID_LIST_BAD_*: bits of reid_list_metrics' status word


def check_cutoffs(ks, limit=None):
    """The cutoffs as a ctypes i32 array for the host side of a call: 1 .. METRICS_MAX_CUTOFFS integers >= 1, strictly ascending
    (and <= ``limit`` when one is given); anything else raises ValueError before a launch."""
    try:
        ks = [int(k) for k in ks]
    except TypeError:
        raise ValueError(f'cutoffs: expected a sequence of integers, got {ks!r}') from None
    if not 1 <= len(ks) <= METRICS_MAX_CUTOFFS:
        raise ValueError(f'cutoffs: {len(ks)} given, 1..{METRICS_MAX_CUTOFFS} supported')
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f'cutoffs: expected integers >= 1 in strictly ascending order, got {tuple(ks)}')
    if limit is not None and ks[-1] > limit:
        raise ValueError(f'cutoffs: {ks[-1]} is beyond the list length {limit}')
    return (C.c_int32 * len(ks))(*ks)


def _req_ids(nq, Ng, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx):
    """The id tensors ``rank_metrics_at`` and ``list_metrics`` share: i32, contiguous, of the lengths the kernels index."""
    for name, t, n in (('g_pid', g_pid, Ng), ('g_img', g_img, Ng), ('q_pid', q_pid, nq), ('q_slot', q_slot, nq), ('csr_idx', csr_idx, Ng),
                       ('csr_off', csr_off, 2)):
        if t is None and name == 'g_img':
            continue
        L._req(t, torch.int32, name)
        if t.dim() != 1 or t.numel() < n or not t.is_contiguous():
            raise ValueError(f'{name}: expected contiguous [>= {n}], got {tuple(t.shape)}')
    if q_excl is not None:
        L._req(q_excl, torch.int32, 'q_excl')
        if tuple(q_excl.shape) != (nq, 4) or not q_excl.is_contiguous():
            raise ValueError(f'q_excl: expected contiguous [{nq}, 4], got {tuple(q_excl.shape)}')


def _req_out(t, dtype, shape, name):
    L._req(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f'{name}: expected contiguous {list(shape)}, got {tuple(t.shape)}')


def rank_metrics_at(scores, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx, Ng, max_pos, ks, ap, rank1, npos, rank_last, hits,
                    sum_at):
    """``rank_metrics`` with cutoffs ``ks`` (reid_rank_metrics_at, include/reid_hip.h): also writes rank_last i32 [nq], hits i32
    [nq, len(ks)] and sum_at f64 [nq, len(ks)]; ap, rank1 and npos are those of ``rank_metrics`` bit for bit."""
    cut = check_cutoffs(ks)
    L._req(scores, torch.float32, 'scores')
    if scores.dim() != 2 or Ng > scores.shape[1]:
        raise ValueError(f'scores: expected [nq, ld >= {Ng}], got {tuple(scores.shape)}')
    nq = scores.shape[0]
    _req_ids(nq, Ng, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx)
    _req_out(ap, torch.float64, (nq,), 'ap'); _req_out(rank1, torch.int32, (nq,), 'rank1'); _req_out(npos, torch.int32, (nq,), 'npos')
    _req_out(rank_last, torch.int32, (nq,), 'rank_last')
    _req_out(hits, torch.int32, (nq, len(cut)), 'hits'); _req_out(sum_at, torch.float64, (nq, len(cut)), 'sum_at')
    check(lib().reid_rank_metrics_at(ptr(scores), scores.stride(0), ptr(g_pid), ptr(g_img), ptr(q_pid), ptr(q_slot), ptr(q_excl),
                                     ptr(csr_off), ptr(csr_idx), nq, Ng, max_pos, C.addressof(cut), len(cut), ptr(ap), ptr(rank1),
                                     ptr(npos), ptr(rank_last), ptr(hits), ptr(sum_at), stream_ptr()))


def list_metrics(idx, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx, Ng, ks, out=None):
    """(npos i32 [nq], rank1 i32 [nq], hits i32 [nq, len(ks)], sum_at f64 [nq, len(ks)], status i32 [nq]) of ranked lists ``idx``
    i32 [nq, k] (reid_list_metrics, include/reid_hip.h): -1 = no entry (trailing only); an excluded gallery row is skipped and the
    positions behind it move up.  Every cutoff must be <= k.  ``out``: the five tensors to write into."""
    L._req(idx, torch.int32, 'idx')
    if idx.dim() != 2 or not idx.is_contiguous() or not 1 <= idx.shape[1] <= ROWS_TOPK_MAX_K or idx.shape[0] < 1:
        raise ValueError(f'idx: expected contiguous [nq >= 1, 1 <= k <= {ROWS_TOPK_MAX_K}], got {tuple(idx.shape)}')
    nq, k = idx.shape
    cut = check_cutoffs(ks, limit=k)
    _req_ids(nq, Ng, g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx)
    if out is None:
        i32 = dict(dtype=torch.int32, device=idx.device)
        out = (torch.empty(nq, **i32), torch.empty(nq, **i32), torch.empty(nq, len(cut), **i32),
               torch.empty(nq, len(cut), dtype=torch.float64, device=idx.device), torch.empty(nq, **i32))
    npos, rank1, hits, sum_at, status = out
    _req_out(npos, torch.int32, (nq,), 'npos'); _req_out(rank1, torch.int32, (nq,), 'rank1'); _req_out(status, torch.int32, (nq,), 'status')
    _req_out(hits, torch.int32, (nq, len(cut)), 'hits'); _req_out(sum_at, torch.float64, (nq, len(cut)), 'sum_at')
    check(lib().reid_list_metrics(ptr(idx), nq, k, ptr(g_pid), ptr(g_img), ptr(q_pid), ptr(q_slot), ptr(q_excl), ptr(csr_off),
                                  ptr(csr_idx), Ng, C.addressof(cut), len(cut), ptr(npos), ptr(rank1), ptr(hits), ptr(sum_at),
                                  ptr(status), stream_ptr()))
    return npos, rank1, hits, sum_at, status


def rows_topk(scores, n, k, g_img=None, q_excl=None, out=None):
    """(idx i32 [nq, k], score f32 [nq, k]): the first k entries of a stable descending sort of scores[:, :n] per row, without the
    sort (reid_rows_topk, include/reid_hip.h); n <= scores.shape[1].  ``g_img`` [n] and ``q_excl`` [nq, 4] together drop a row's excluded images as
    ``rank_metrics`` does; positions past the eligible columns hold -1 / -inf.  ``out``: the (idx, score) pair to write into."""
    L._req(scores, torch.float32, 'scores')
    if scores.dim() != 2:
        raise ValueError(f'scores: expected [nq, ld], got {tuple(scores.shape)}')
    nq = scores.shape[0]
    if n > scores.shape[1]:
        raise ValueError(f'scores: n={n} columns asked of a [{nq}, {scores.shape[1]}] tensor')
    if g_img is not None:
        L._req(g_img, torch.int32, 'g_img')
        if g_img.numel() < n or not g_img.is_contiguous():
            raise ValueError(f'g_img: expected contiguous [>= {n}], got {tuple(g_img.shape)}')
    if q_excl is not None:
        L._req(q_excl, torch.int32, 'q_excl')
        if tuple(q_excl.shape) != (nq, 4) or not q_excl.is_contiguous():
            raise ValueError(f'q_excl: expected contiguous [{nq}, 4], got {tuple(q_excl.shape)}')
    if out is None:
        out = (torch.empty(nq, max(k, 0), dtype=torch.int32, device=scores.device),
               torch.empty(nq, max(k, 0), dtype=torch.float32, device=scores.device))
    idx, score = out
    L._req(idx, torch.int32, 'out idx'); L._req(score, torch.float32, 'out score')
    if not (tuple(idx.shape) == tuple(score.shape) == (nq, k) and idx.is_contiguous() and score.is_contiguous()):
        raise ValueError(f'out: expected two contiguous [{nq}, {k}] tensors, got {tuple(idx.shape)}, {tuple(score.shape)}')
    check(lib().reid_rows_topk(ptr(scores), scores.stride(0), nq, n, k, ptr(g_img), ptr(q_excl), ptr(idx), ptr(score), stream_ptr()))
    return idx, score


EXPAND_MAX_LIST = 64          # REID_EXPAND_MAX_LIST: the longest ranked list reid_expand_rows walks
EXPAND_MAX_ALPHA = 16         # REID_EXPAND_MAX_ALPHA


def expand_rows(x, table, nbr, score, k, alpha, self_base=-1, normalize=True, eps=1e-12, out=None):
    """out[i] = x[i] + sum of w * table[nbr[i, t]] over the first k eligible entries of row i's list, L2-normalised unless
    ``normalize`` is false (reid_expand_rows, include/reid_hip.h: query expansion with ``self_base`` = -1, database-side augmentation
    of the rows ``self_base`` .. of the table otherwise).  ``nbr`` i32 / ``score`` f32 [rows, kl] as ``rows_topk`` and
    ``GalleryIndex.topk`` return them; w = 1 for ``alpha`` = 0, else max(score, 0) ** alpha.  ``out``: the [rows, D] tensor to write."""
    L._req(x, torch.float32, 'x'); L._req(table, torch.float32, 'table')
    L._req(nbr, torch.int32, 'nbr'); L._req(score, torch.float32, 'score')
    if x.dim() != 2 or table.dim() != 2 or table.shape[1] != x.shape[1]:
        raise ValueError(f'x, table: expected [rows, D] and [M, D], got {tuple(x.shape)}, {tuple(table.shape)}')
    rows, D = x.shape
    if nbr.dim() != 2 or nbr.shape[0] != rows or tuple(score.shape) != tuple(nbr.shape) or (rows > 1 and score.stride(0) != nbr.stride(0)):
        raise ValueError(f'nbr, score: expected two [{rows}, kl] tensors of one row stride, got {tuple(nbr.shape)}, {tuple(score.shape)}')
    if out is None:
        out = torch.empty(rows, D, dtype=torch.float32, device=x.device)
    L._req(out, torch.float32, 'out')
    if tuple(out.shape) != (rows, D):
        raise ValueError(f'out: expected [{rows}, {D}], got {tuple(out.shape)}')
    ld = lambda t: t.stride(0) if t.shape[0] > 1 else t.shape[1]           # (the row stride of a one-row tensor says nothing)
    check(lib().reid_expand_rows(ptr(x), ld(x), ptr(table), ld(table), table.shape[0], ptr(nbr), ptr(score), ld(nbr),
                                 nbr.shape[1], k, alpha, self_base, int(bool(normalize)), eps, ptr(out), ld(out), rows, D,
                                 stream_ptr()))
    return out


def rerank_weights(nbr, X, V, k1):
    """V[i, :N] = k-reciprocal weights of pooled row i (reid_rerank_weights, include/reid_hip.h); zero-fills V[:, :N] first."""
    check(lib().reid_rerank_weights(ptr(nbr), nbr.stride(0), ptr(X), X.stride(0), ptr(V), V.stride(0), X.shape[0], X.shape[1], k1,
                                    stream_ptr()))


def rerank_expand(V, nbr, V2, k1, k2):
    """V2[i, :N] = mean of V[nbr[i, :k2], :N] (reid_rerank_expand)."""
    check(lib().reid_rerank_expand(ptr(V), V.stride(0), ptr(nbr), nbr.stride(0), ptr(V2), V2.stride(0), V.shape[0], k1, k2, stream_ptr()))


def rerank_jaccard(A, B, cos, out, Ng, N, lambda_value):
    """out[q, :Ng] = (1 - lambda) J + lambda cos, J from sum_j min(A[q, j], B[g, j]) over N columns (reid_rerank_jaccard)."""
    check(lib().reid_rerank_jaccard(ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(cos), cos.stride(0), ptr(out), out.stride(0),
                                    A.shape[0], Ng, N, lambda_value, stream_ptr()))


def rerank_weights_sparse(nbr, X, vcols, vvals, vcnt, k1):
    """Padded rows of V: vcols / vvals[i, :vcnt[i]] = members of R*(i) and their weights (reid_rerank_weights_sparse)."""
    check(lib().reid_rerank_weights_sparse(ptr(nbr), nbr.stride(0), ptr(X), X.stride(0), ptr(vcols), ptr(vvals), ptr(vcnt), vvals.stride(0),
                                           X.shape[0], X.shape[1], k1, stream_ptr()))


def rerank_expand_count(vcols, vvals, vcnt, nbr, cnt, k1, k2):
    """cnt[i] = non-zeros of row i of V2 (reid_rerank_expand_count)."""
    check(lib().reid_rerank_expand_count(ptr(vcols), ptr(vvals), ptr(vcnt), vvals.stride(0), ptr(nbr), nbr.stride(0), ptr(cnt), vcnt.shape[0],
                                         k1, k2, stream_ptr()))


def rerank_expand_sparse(vcols, vvals, vcnt, nbr, rowptr, cols, vals, k1, k2):
    """CSR rows of V2 at rowptr (int64 [N + 1]): columns ascending, the dense values (reid_rerank_expand_sparse)."""
    check(lib().reid_rerank_expand_sparse(ptr(vcols), ptr(vvals), ptr(vcnt), vvals.stride(0), ptr(nbr), nbr.stride(0), ptr(rowptr), ptr(cols),
                                          ptr(vals), vcnt.shape[0], k1, k2, stream_ptr()))


def rerank_jaccard_sparse(rowptr, cols, vals, colptr, rows, cvals, cos, out, Ng, lambda_value):
    """out[q, :Ng] = (1 - lambda) J + lambda cos for the len(rowptr) - 1 CSR rows at rowptr (absolute offsets into cols / vals)
    against the gallery's CSC arrays (reid_rerank_jaccard_sparse)."""
    check(lib().reid_rerank_jaccard_sparse(ptr(rowptr), ptr(cols), ptr(vals), cols.shape[0], ptr(colptr), ptr(rows), ptr(cvals), rows.shape[0],
                                           ptr(cos), cos.stride(0), ptr(out), out.stride(0), rowptr.shape[0] - 1, Ng, colptr.shape[0] - 1,
                                           lambda_value, stream_ptr()))


def _req_sim_rows(scores, n, row0):
    """The similarity-row chunk ``dbscan_count`` and ``dbscan_fill`` share: f32 [nr >= 1, >= n], rows row0 .. row0 + nr - 1 of n."""
    L._req(scores, torch.float32, 'scores')
    if scores.dim() != 2 or scores.shape[0] < 1:
        raise ValueError(f'scores: expected [nr >= 1, ld], got {tuple(scores.shape)}')
    nr = scores.shape[0]
    if n > scores.shape[1]:
        raise ValueError(f'scores: n={n} columns asked of a [{nr}, {scores.shape[1]}] tensor')
    if row0 < 0 or row0 + nr > n:
        raise ValueError(f'scores: rows {row0}..{row0 + nr - 1} are not rows of an [{n}, {n}] matrix')
    return nr


def dbscan_count(scores, n, row0, thr, min_samples, count, core):
    """count[r] = |N(row0 + r)| = the columns j < n of row r with scores[r, j] >= thr, the row's own column row0 + r always among them,
    and core[r] = count[r] >= min_samples (reid_dbscan_count, include/reid_hip.h).  ``count`` i32 [nr], ``core`` u8 [nr]."""
    nr = _req_sim_rows(scores, n, row0)
    _req_out(count, torch.int32, (nr,), 'count'); _req_out(core, torch.uint8, (nr,), 'core')
    check(lib().reid_dbscan_count(ptr(scores), scores.stride(0), nr, n, row0, thr, min_samples, ptr(count), ptr(core), stream_ptr()))


def dbscan_fill(scores, n, row0, thr, rowptr, cols):
    """cols[rowptr[r] : rowptr[r + 1]] = the columns of N(row0 + r), ascending (reid_dbscan_fill); ``rowptr`` i64 [nr + 1] is the
    exclusive prefix sum of ``dbscan_count``'s counts for the same rows and threshold, ``cols`` i32 [>= rowptr[nr]]."""
    nr = _req_sim_rows(scores, n, row0)
    _req_out(rowptr, torch.int64, (nr + 1,), 'rowptr')
    L._req(cols, torch.int32, 'cols')
    if cols.dim() != 1 or not cols.is_contiguous():
        raise ValueError(f'cols: expected a contiguous vector, got {tuple(cols.shape)}')
    check(lib().reid_dbscan_fill(ptr(scores), scores.stride(0), nr, n, row0, thr, ptr(rowptr), ptr(cols), cols.shape[0], stream_ptr()))


def _req_csr(rowptr, cols, core):
    """The neighbour CSR of N rows and their core flags, as the component passes read them; returns N."""
    L._req(rowptr, torch.int64, 'rowptr'); L._req(cols, torch.int32, 'cols'); L._req(core, torch.uint8, 'core')
    N = core.shape[0]
    if core.dim() != 1 or N < 1 or tuple(rowptr.shape) != (N + 1,) or cols.dim() != 1 or not (rowptr.is_contiguous() and cols.is_contiguous()
                                                                                               and core.is_contiguous()):
        raise ValueError(f'expected contiguous core [N >= 1], rowptr [N + 1], cols [nnz], got {tuple(core.shape)}, {tuple(rowptr.shape)}, '
                         f'{tuple(cols.shape)}')
    return N


def dbscan_hook(rowptr, cols, core, parent, changed):
    """One hook pass over the directed core-core edges of the CSR: atomicMin(parent[max(pi, pj)], min(pi, pj)); ``changed`` (an i32
    scalar on the device) grows when, and only when, an edge saw two different parents (reid_dbscan_hook)."""
    N = _req_csr(rowptr, cols, core)
    _req_out(parent, torch.int32, (N,), 'parent')
    L._req(changed, torch.int32, 'changed')
    if changed.numel() != 1:
        raise ValueError(f'changed: expected one i32, got {tuple(changed.shape)}')
    check(lib().reid_dbscan_hook(ptr(rowptr), ptr(cols), cols.shape[0], ptr(core), ptr(parent), N, ptr(changed), stream_ptr()))


def dbscan_compress(parent):
    """parent[x] = the root of x's pointer chain (reid_dbscan_compress)."""
    _req_out(parent, torch.int32, (parent.shape[0],), 'parent')
    check(lib().reid_dbscan_compress(ptr(parent), parent.shape[0], stream_ptr()))


def dbscan_border(rowptr, cols, core, parent, label):
    """label[j] = min(label[j], parent[i]) over the cores i with the non-core j in N(i) (reid_dbscan_border); ``label`` i32 [N]."""
    N = _req_csr(rowptr, cols, core)
    _req_out(parent, torch.int32, (N,), 'parent'); _req_out(label, torch.int32, (N,), 'label')
    check(lib().reid_dbscan_border(ptr(rowptr), ptr(cols), cols.shape[0], ptr(core), ptr(parent), ptr(label), N, stream_ptr()))


def gather_rows(src, index, dst):
    """dst[r] = src[index[r]] (f32 rows, cols % 4 == 0; int32 index)."""
    check(lib().reid_gather_rows_f32(ptr(src), src.stride(0), ptr(index), ptr(dst), dst.stride(0), index.shape[0], dst.shape[1],
                                     stream_ptr()))
    return dst


def scatter_add_rows(src, index, out):
    """out[index[r]] += src[r] (f32 rows; int32 index)."""
    check(lib().reid_scatter_add_rows_f32(ptr(src), src.stride(0), ptr(index), ptr(out), out.stride(0), src.shape[0], src.shape[1],
                                          out.shape[0], stream_ptr()))


def embed_tokens(tok, pos, ids, out):
    """out[b*T + t] = tok[ids[b, t]] + pos[t]  (text-tower input, f32)."""
    B, T = ids.shape
    check(lib().reid_embed_tokens(ptr(tok), ptr(pos), ptr(ids), ptr(out), B, T, tok.shape[1], tok.shape[0], stream_ptr()))
    return out


# ----------------------------------------------------------------------------------------- image transforms of the input
def augment_ws_bytes(n, S):
    return int(lib().reid_augment_ws_bytes(n, S))


def augment_images(src, src_bytes, table, host_table, n, S, lut, ws, out):
    """uint8 RGB HWC images packed in ``src`` -> normalised fp32 ``out`` [n, 3, S, S] by the int32 entries of ``table`` (device) /
    ``host_table`` (host, validated before the launch); see reid_augment_images in include/reid_hip.h."""
    check(lib().reid_augment_images(ptr(src), src_bytes, ptr(table), ptr(host_table), n, S, ptr(lut), ptr(ws), ws.numel(), ptr(out),
                                    stream_ptr()))
    return out
