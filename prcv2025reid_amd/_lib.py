"""ctypes binding of libreid_hip.so (include/reid_hip.h).  No CPU fallback exists:
if the library is missing or a call fails this module raises."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATHS = {'bf16': os.path.join(_HERE, 'csrc', 'libreid_hip.so'), 'f16': os.path.join(_HERE, 'csrc', 'libreid_hip_f16.so')}
if os.environ.get('REID_LIB_BF16'):                 # experiment builds (tools/): another bf16-flavor library file
    LIB_PATHS['bf16'] = os.environ['REID_LIB_BF16']
LIB_PATH = LIB_PATHS['bf16']
T16_DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
_flavor = os.environ.get('REID_T16', 'bf16')


def set_flavor(name: str):
    """Select the 16-bit MFMA operand format for everything launched afterwards ('bf16' or 'f16')."""
    global _flavor
    if name not in LIB_PATHS:
        raise ValueError(f'unknown 16-bit flavor {name!r}')
    _flavor = name


def flavor() -> str:
    return _flavor


def t16() -> torch.dtype:
    return T16_DTYPES[_flavor]


ABI_VERSION = 201                 # REID_ABI_VERSION of include/reid_hip.h: a library that reports anything else is a stale build
BF16, F32, F16 = 0, 1, 2          # reid_dtype: BF16 = the flavor's 16-bit format, F16 = IEEE half whatever the flavor
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_DGELU, ACT_DQUICK_GELU, ACT_DRELU, ACT_MUL_AUX, ACT_GELU_DSAVE = range(9)
MARGIN_KINDS = {'cosine': 0, 'cosface': 1, 'arcface': 2, 'circle': 3}      # REID_MARGIN_*
CLUSTER_NCE_MODES = {'mean': 0, 'hard': 1}                                  # REID_CLUSTER_NCE_*


class GemmArgs(C.Structure):
    _fields_ = [('A', C.c_void_p), ('B', C.c_void_p), ('A2', C.c_void_p), ('B2', C.c_void_p),
                ('bias', C.c_void_p), ('R', C.c_void_p), ('aux', C.c_void_p), ('C', C.c_void_p), ('C2', C.c_void_p),
                ('img_mod', C.c_void_p),
                ('M', C.c_int32), ('N', C.c_int32), ('K', C.c_int32), ('K2', C.c_int32),
                ('lda', C.c_int32), ('ldb', C.c_int32), ('lda2', C.c_int32), ('ldb2', C.c_int32),
                ('ldr', C.c_int32), ('ldaux', C.c_int32), ('ldc', C.c_int32), ('ldc2', C.c_int32),
                ('k2_group_n', C.c_int32),
                ('act', C.c_int32), ('c_dtype', C.c_int32), ('c2_dtype', C.c_int32), ('r_dtype', C.c_int32),
                ('r_period', C.c_int32),
                ('mask_r', C.c_int32), ('mask_period', C.c_int32), ('rows_per_img', C.c_int32),
                ('c_group', C.c_int32), ('c_group_stride', C.c_int32), ('c_row_off', C.c_int32),
                ('alpha', C.c_float), ('row_scale', C.c_void_p),
                ('n_row_groups', C.c_int32), ('row_group_end', C.c_int32 * 8), ('row_group_b', C.c_int32 * 8),
                ('b_group_stride', C.c_int64)]


GEMM_KERNELS = ('tiled', 'pp', 'pps')                                                               # REID_GEMM_*
GEMM_EPILOGUES = ('generic', 'plain16', 'res32', 'gelu2', 'dgelu', 'gelu2d', 'mulaux', 'plain16h')  # REID_EPI_*


class GemmPlan(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('bm', C.c_int32), ('bn', C.c_int32), ('epilogue', C.c_int32),
                ('tiles_m', C.c_int32), ('tiles_n', C.c_int32), ('grid', C.c_int32)]


# Every entry point of include/reid_hip.h in header order, name -> (restype, argtypes): ctypes then refuses a call with too few
# arguments and converts each plain Python value (int or None for a pointer, int for an integer, float for a float) itself.
_P, _I, _I64, _F, _S = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_char_p   # T*; int, int32_t, enum; int64_t; float; const char*
_GEMM, _PLAN = C.POINTER(GemmArgs), C.POINTER(GemmPlan)
SIGNATURES = {
    'reid_last_error': (_S, []),
    'reid_version': (_I, []),
    'reid_flavor': (_I, []),
    'reid_check_device': (_I, [_I]),
    'reid_set_knob': (_I, [_S, _I]),
    'reid_mer_gemm': (_I, [_GEMM, _P]),
    'reid_mer_gemm_plan': (_I, [_GEMM, _I, _I, _PLAN]),
    'reid_gemm_tn': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _P]),
    'reid_layernorm_fwd': (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P]),
    'reid_add_layernorm_fwd': (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P]),
    'reid_layernorm_bwd': (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _P, _I, _P, _P]),
    'reid_patch_im2col': (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    'reid_cls_rows': (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    'reid_attn_fwd': (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'reid_attn_bwd': (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'reid_cast_f32_bf16': (_I, [_P, _P, _I64, _P]),
    'reid_cast_bf16_f32': (_I, [_P, _P, _I64, _P]),
    'reid_pack_bf16_table': (_I, [_P, _P, _P, _I, _P]),
    'reid_lora_bwd_fused': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _F, _P, _I, _P]),
    'reid_lora_da_fused': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    'reid_merge_lora_table': (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _F, _P]),
    'reid_gather_rows_f32': (_I, [_P, _I, _P, _P, _I, _I, _I, _P]),
    'reid_embed_tokens': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'reid_scatter_add_rows_f32': (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P]),
    'reid_bnneck_stats': (_I, [_P, _I, _I, _I, _P, _P, _P]),
    'reid_bnneck_fwd': (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _I, _P, _P, _I, _P, _P, _P, _I, _I, _F, _F, _F, _P]),
    'reid_bnneck_bwd_p1': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
    'reid_bnneck_bwd_p2': (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _F, _I, _P, _I, _I, _I, _P]),
    'reid_ce_ls_fwd': (_I, [_P, _I, _P, _P, _I, _I, _F, _P, _P, _P]),
    'reid_ce_ls_bwd': (_I, [_P, _I, _P, _P, _I, _I, _F, _P, _P, _I, _P]),
    'reid_sdm_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P]),
    'reid_sdm_bwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _I, _P, _I, _P]),
    'reid_sdm_ws_floats': (_I64, [_I, _I, _I, _I]),
    'reid_triplet_hard_fwd': (_I, [_P, _I, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P]),
    'reid_triplet_hard_bwd': (_I, [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    'reid_cross_triplet_ws_floats': (_I64, [_I, _I, _I, _I]),
    'reid_cross_triplet_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P]),
    'reid_cross_triplet_bwd': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    'reid_hc_triplet_ws_floats': (_I64, [_I, _I, _I, _I]),
    'reid_hc_triplet_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    'reid_hc_triplet_bwd': (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _F, _I, _F, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    'reid_xbm_ws_floats': (_I64, [_I, _I, _I, _I]),
    'reid_xbm_enqueue': (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    'reid_xbm_triplet_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'reid_xbm_triplet_bwd': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _F, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    'reid_center_ws_floats': (_I64, [_I, _I, _I]),
    'reid_center_fwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    'reid_center_update': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _F, _P]),
    'reid_center_bwd': (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _P]),
    'reid_cluster_nce_ws_floats': (_I64, [_I, _I, _I, _I]),
    'reid_cluster_nce_plan': (_I, [_I, _I, _I, _P]),
    'reid_cluster_nce_fwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _I, _F, _I, _P, _P, _P, _P, _P]),
    'reid_cluster_nce_update': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _F, _I, _P]),
    'reid_cluster_nce_bwd': (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _P]),
    'reid_cluster_centroids': (_I, [_P, _I, _I64, _P, _P, _I, _I, _P, _P]),
    'reid_smooth_ap_ws_floats': (_I64, [_I, _I, _I, _I, _I, _I, _I]),
    'reid_smooth_ap_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _F, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I,
                                _P, _P, _P, _P, _P, _P, _P]),
    'reid_smooth_ap_bwd': (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P]),
    'reid_class_means': (_I, [_P, _I, _I64, _P, _P, _I, _I, _P, _P]),
    'reid_hybrid_update_instances': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _I64, _F, _P]),
    'reid_hybrid_refresh_classes': (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _I64, _P, _P, _P, _I, _P]),
    'reid_topk_ws_bytes': (_I64, [_I, _I, _I]),
    'reid_topk_scan_ok': (_I, [_I, _I, _I, _I]),
    'reid_cosine_topk': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    'reid_cosine_topk_exact': (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    'reid_cosine_topk_exact_slots': (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P]),
    'reid_topk_stream_ok': (_I, [_I, _I, _I, _I]),
    'reid_topk_stream_ws_bytes': (_I64, [_I]),
    'reid_cosine_topk_stream': (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    'reid_sgemm': (_I, [_P, _P, _P, _I, _I, _I, _I64, _I64, _I64, _I64, _I, _F, _F, _P, _I, _P]),
    'reid_eltwise_f32': (_I, [_I, _P, _P, _P, _I64, _F, _P]),
    'reid_small_attn_fwd': (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    'reid_small_attn_bwd': (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    'reid_masked_mean': (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    'reid_l2norm_rows': (_I, [_P, _I, _P, _P, _I, _I, _I, _F, _F, _P]),
    'reid_opt_entry_bytes': (_I, []),
    'reid_opt_ws_floats': (_I, [_I]),
    'reid_opt_state_floats': (_I, []),
    'reid_opt_sumsq': (_I, [_P, _I, _P, _P]),
    'reid_opt_clip': (_I, [_P, _I, _P, _I, _F, _I, _P]),
    'reid_opt_adamw': (_I, [_P, _I, _P, _F, _F, _F, _I, _I, _P, _P]),
    'reid_ema_entry_bytes': (_I, []),
    'reid_ema_update': (_I, [_P, _I, _F, _I, _I, _P, _P]),
    'reid_ema_swap': (_I, [_P, _I, _P]),
    'reid_rank_metrics': (_I, [_P, _I64, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    'reid_rank_metrics_at': (_I, [_P, _I64, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    'reid_rows_topk': (_I, [_P, _I64, _I, _I, _I, _P, _P, _P, _P, _P]),
    'reid_list_metrics': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    'reid_augment_ws_bytes': (_I64, [_I, _I]),
    'reid_augment_images': (_I, [_P, _I64, _P, _P, _I, _I, _P, _P, _I64, _P, _P]),
    'reid_expand_rows': (_I, [_P, _I64, _P, _I64, _I, _P, _P, _I, _I, _I, _I, _I64, _I, _F, _P, _I64, _I, _I, _P]),
    'reid_cos_logits_fwd': (_I, [_P, _I, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _I, _P]),
    'reid_cos_logits_bwd_prep': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P]),
    'reid_cos_logits_bwd_fix': (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P]),
    'reid_margin_ce_fwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P]),
    'reid_margin_ce_bwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _I, _P]),
    'reid_dbscan_count': (_I, [_P, _I64, _I, _I, _I64, _F, _I, _P, _P, _P]),
    'reid_dbscan_fill': (_I, [_P, _I64, _I, _I, _I64, _F, _P, _P, _I64, _P]),
    'reid_dbscan_hook': (_I, [_P, _P, _I64, _P, _P, _I, _P, _P]),
    'reid_dbscan_compress': (_I, [_P, _I, _P]),
    'reid_dbscan_border': (_I, [_P, _P, _I64, _P, _P, _P, _I, _P]),
    'reid_rerank_weights_sparse': (_I, [_P, _I, _P, _I, _P, _P, _P, _I64, _I, _I, _I, _P]),
    'reid_rerank_expand_count': (_I, [_P, _P, _P, _I64, _P, _I, _P, _I, _I, _I, _P]),
    'reid_rerank_expand_sparse': (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    'reid_rerank_jaccard_sparse': (_I, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _I64, _I, _I, _I, _F, _P]),
    'reid_rerank_weights': (_I, [_P, _I, _P, _I, _P, _I64, _I, _I, _I, _P]),
    'reid_rerank_expand': (_I, [_P, _I64, _P, _I, _P, _I64, _I, _I, _I, _P]),
    'reid_rerank_jaccard': (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _I, _I, _F, _P]),
}
EXPORTS = list(SIGNATURES)


_libs = {}


class ReidHipError(RuntimeError):
    pass


def lib():
    """The loaded library of the current flavor; raises (never falls back) when it is absent."""
    h = _libs.get(_flavor)
    if h is None:
        path = LIB_PATHS[_flavor]
        if not os.path.exists(path):
            raise ReidHipError(f'{path} not found: build it with `python -m prcv2025reid_amd.build` '
                               '(there is no CPU or PyTorch fallback for the hot path)')
        h = _checked(C.CDLL(path), path)
        _libs[_flavor] = h
    return h


def _checked(h, path):
    """Refuses a library whose exports, ABI version or flavor differ from what this module binds; then binds SIGNATURES."""
    missing = [n for n in EXPORTS if not hasattr(h, n)]
    if missing:
        raise ReidHipError(f'{path} lacks symbols {missing}: stale build, run `python -m prcv2025reid_amd.build --force`')
    v = h.reid_version()
    if v != ABI_VERSION:
        raise ReidHipError(f'{path} has ABI version {v}, this package binds {ABI_VERSION}: stale build, '
                           'run `python -m prcv2025reid_amd.build --force`')
    if h.reid_flavor() != (1 if _flavor == 'f16' else 0):
        raise ReidHipError(f'{path} was built for the other 16-bit flavor')
    return bind(h)


def bind(h):
    """Sets restype and argtypes of every entry point of ``h`` (a loaded library) from SIGNATURES; returns ``h``."""
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(h, name)
        f.restype, f.argtypes = restype, argtypes
    return h


def check(rc: int):
    if rc != 0:
        raise ReidHipError(f'libreid_hip: rc={rc}: {lib().reid_last_error().decode()}')


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dt(t, allow_half: bool = False) -> int:
    if t.dtype == torch.bfloat16 or t.dtype == torch.float16:
        if t.dtype != t16():
            if allow_half and t.dtype == torch.float16:          # an IEEE-half tensor in the bf16 flavor (REID_F16: not an MFMA operand)
                return F16
            raise TypeError(f'{t.dtype} tensor passed to the {_flavor} flavor of libreid_hip')
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f'unsupported dtype {t.dtype}')


def _req(t, dtype=None, name='tensor'):
    if not t.is_cuda:
        raise ReidHipError(f'{name} must be a CUDA(HIP) tensor')
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f'{name}: last dim must be contiguous')


def ld(t) -> int:
    return t.stride(0) if t.dim() == 2 else t.shape[-1]
