"""Shared test helpers: rebuild golden cases from their seeds."""
import math
import os

import numpy as np
import torch

from prcv2025reid_amd.config import TrainingConfig, arch_of
from prcv2025reid_amd.synthetic import synthetic_batch
from prcv2025reid_amd.tokenizer import HashTokenizer
from prcv2025reid_amd.weights import seeded_state, fingerprint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = {k[5:]: float(z[k]) for k in z.files if k.startswith('meta.')}
    return z, meta


def case_config(meta, device='cpu'):
    return TrainingConfig(
        device=device, mer_lora_rank=int(meta['rank']), mer_lora_alpha=meta['alpha'],
        contrastive_weight=meta['contrastive_weight'], ce_weight=meta['ce_weight'],
        sdm_temperature=meta['tau'], vision_hidden_dim=int(meta['vision_hidden_dim']),
        vision_layers=int(meta['vision_layers']), vision_heads=int(meta['vision_heads']),
        vision_mlp_dim=int(meta['vision_mlp_dim']), text_layers=int(meta['text_layers']),
        text_mlp_dim=int(meta['text_mlp_dim']), text_vocab=int(meta['text_vocab']),
        text_eos_id=int(meta['text_eos_id']), text_bos_id=int(meta['text_bos_id']),
        drop_path=0.0, modality_dropout=0.0, dropout_rate=0.0, fusion_dropout=0.0, sdm_dropout=0.0)


def case_inputs(meta):
    cfg = case_config(meta)
    arch = arch_of(cfg)
    C = int(meta['num_classes'])
    state = seeded_state(arch, C, int(meta['wseed']))
    batch = synthetic_batch(int(meta['P']), int(meta['K']), arch, seed=int(meta['dseed']),
                            mask_drop=meta['mask_drop'], num_classes=C)
    tok = HashTokenizer(arch['text_vocab'], arch['text_bos_id'], arch['text_eos_id'], arch['text_max_len'])
    tokens = tok(batch['texts'], padding=True, truncation=True, max_length=77)
    return cfg, arch, state, batch, tokens


def edge_inputs(batch, variant):
    """(images, texts, masks) of the reference call for an edge-case ``variant`` (model.py:367,386-389 no masks; :125-126,
    479-480 single modality; :141-149 all-masked row; :417-418 text default mask).  Shared with the tests."""
    images, texts, masks = batch['images'], batch['texts'], batch['modality_mask']
    if variant == 'nomask':
        return images, texts, None
    if variant == 'single':
        return {'vis': images['vis']}, None, {'vis': masks['vis']}
    if variant == 'textonly':
        return None, texts, None
    if variant == 'novis03':                      # rows 0 and 3 have no RGB image (their other modalities stay)
        masks = {m: t.clone() for m, t in masks.items()}
        images = {m: t.clone() for m, t in images.items()}
        for i in (0, 3):
            masks['vis'][i] = 0.0; images['vis'][i] = 0.0
            masks['nir'][i] = 1.0
        return images, texts, masks
    if variant == 'deadrow':                      # sample 1 has no valid modality at all
        masks = {m: t.clone() for m, t in masks.items()}
        images = {m: t.clone() for m, t in images.items()}
        texts = list(texts)
        for m in masks:
            masks[m][1] = 0.0
        for m in images:
            images[m][1] = 0.0
        texts[1] = ''
        return images, texts, masks
    return images, texts, masks



# fixed modality-dropout draws of the reference-generated fixtures: name -> (forced torch.rand(1) values in the order
# nir, sk, cp, text -- keep iff value > p = 0.5 --, mask_drop of the batch, input variant); epoch 5 > warm-up 3
MODDROP_CASES = {
    'tiny_moddrop_a': ((0.1, 0.9, 0.2, 0.8), 0.0, None),        # nir and cp dropped
    'tiny_moddrop_b': ((0.1, 0.2, 0.3, 0.4), 0.0, None),        # everything but vis dropped -> unfused vis feature
    'tiny_moddrop_c': ((0.1, 0.2, 0.3, 0.4), 0.3, 'novis03'),   # would leave rows 0 and 3 empty -> the draw is cancelled
    'tiny_moddrop_d': ((0.9, 0.2, 0.8, 0.1), 0.3, None),        # sk and text dropped from a 30 % masked batch
}


def check_fingerprint(z, state):
    got = fingerprint(state)
    want = float(z['weights_fingerprint'])
    assert abs(got - want) <= 1e-9 * abs(want), (
        f'seeded weights differ from the ones the golden file was made with ({got} vs {want}): '
        'torch RNG drift -- regenerate tests/golden with make_golden.py')


def maxdiff(a, b):
    a = torch.as_tensor(np.asarray(a)).double(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max())


def reference_trainable_groups(tag='tiny_frozen'):
    """The reference's optimiser groups after train.py:1418-1458 -- get_learnable_params() filtered to requires_grad -- from the
    inventory the reference itself produced (tests/golden/learnable_params.json: names, learning rates, trainable flags)."""
    import json
    groups = json.load(open(os.path.join(GOLDEN, 'learnable_params.json')))[tag]
    out = []
    for g in groups:
        keys = [k for k, t in zip(g['params'], g['trainable']) if t]
        if keys:
            out.append(dict(name=g['name'], lr=g['lr'], params=keys))
    return out


# ---- exact-operand tests (test_gemm_exact_gpu.py) ------------------------------------------------------------------------------
# Operands that are small integers times a power of two make every product and every partial sum of a GEMM a multiple of one
# quantum; while the largest possible partial sum stays below 2^24 quanta, fp32 represents all of them exactly, so a kernel's
# accumulator equals the fp64 reference whatever the order of the sum (tiling, split K, atomics).
FMT16 = {'bf16': (8, -126), 'f16': (11, -14), 'f32': (24, -126)}   # significant bits, exponent of the smallest normal
SENTINEL16 = {'bf16': 0x7F9D, 'f16': 0x7DAD}                         # signalling-NaN patterns: no arithmetic produces them
SENTINEL32 = 0x7FBADBAD


def exact_ints(shape, lo, hi, exp, gen, device='cuda'):
    """float64 tensor of integers in [lo, hi] times 2**exp."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=device, dtype=torch.int64).double() * 2.0 ** exp


def assert_bit_budget(abs_sum, quantum):
    """`abs_sum` bounds every partial sum (the sum of the absolute values of the terms), and every term is a multiple of `quantum`:
    then every partial sum is exact in fp32 iff it needs at most 24 significant bits."""
    worst = float(abs_sum.max()) / quantum
    assert worst < 2.0 ** 24, f'operands exceed the fp32 bit budget: {worst:.4g} quanta >= 2^24'


def quantum16(x, fmt):
    """Spacing of the `fmt` grid (FMT16) at |x| (float64): 2^(e - p) for |x| in [2^(e-1), 2^e), the subnormal spacing below."""
    p, emin = FMT16[fmt]
    xc = x.cpu()                                      # (evaluated on the host: plain IEEE fp64 arithmetic, no device math library)
    _, e = torch.frexp(xc)
    e = torch.where(xc == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(xc), torch.clamp(e, min=emin + 1) - p).to(x.device)


def round16(x, fmt):
    """Round-to-nearest-even of float64 `x` into `fmt`, independent of any conversion routine; IEEE half saturates finite overflow
    to +-65504 (what the kernels' MODE.FP16_OVFL conversions do)."""
    xc = x.cpu()
    q = quantum16(xc, fmt)
    y = torch.round(xc / q) * q                      # torch.round: ties to even
    if fmt == 'f16':
        y = torch.where(y.abs() > 65504.0, torch.copysign(torch.full_like(y, 65504.0), y), y)
    return y.to(x.device)


def count_ties16(x, fmt):
    """Elements of `x` that lie exactly half-way between two neighbours of the `fmt` grid (where only ties-to-even decides)."""
    xc = x.cpu()
    s = xc / quantum16(xc, fmt)
    return int(((s - torch.floor(s)) == 0.5).sum())


def sentinel_buffer(rows, cols, dtype, fmt=None, device='cuda'):
    """[rows, cols] buffer whose every element holds the sentinel NaN pattern of its type."""
    if dtype == torch.float32:
        return torch.full((rows, cols), SENTINEL32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full((rows, cols), SENTINEL16[fmt], dtype=torch.int16, device=device).view(dtype)


def is_sentinel(t, fmt=None):
    """Bool tensor: the element still holds the sentinel of sentinel_buffer."""
    if t.dtype == torch.float32:
        return t.view(torch.int32) == SENTINEL32
    return t.view(torch.int16) == SENTINEL16[fmt]


# ---- transcendental epilogues (reid_mer_gemm, reid_sgemm, reid_eltwise_f32): derived error bounds ---------------------------------------------------------------------------
# The kernel applies f to an EXACT fp32 input x, so its error is that of its own evaluation of f, then one rounding to the output
# format.  u = 2^-24 (fp32 unit roundoff).
#   * Phi(x) (common.h gauss_cdf_pdf / gelu_both_x2): Abramowitz-Stegun 7.1.26 has |erf error| <= 1.5e-7, so Phi is off by <= 7.5e-8
#     absolutely; the two-lane form gelu_both_x2 (the lean GELU epilogues) adds <= 6e-8 (its comment: cdf = 0.5 + copysign(0.5 - q)).
#     fp32 evaluation of q = 0.5 erfc: t = rcp(1 + p z) (v_rcp_f32 1 ulp, z and den rounded, the constants rounded: <= 4u relative),
#     Horner on five alternating coefficients (sum |a_i| t^i <= 4.5 P(t), d log P / d log t <= 16: <= 11 * 4.5 u + 16 * 4u <= 114u),
#     exp2 (v_exp_f32 1 ulp = 2u) of xs = -x^2 log2(e)/2 whose own rounding (two products, a rounded constant: 3u relative) moves the
#     result by ln2 |xs| 3u, two more products: |dq| <= q (130 + 3 ln2 |xs|) u; cdf = 1 - q or 0.5 + (0.5 - q): <= 2u more.
#   * Phi'(x) x term: x * 0.3989f * e: e as above ((4 + 3 ln2 |xs|) u relative), three roundings.
#   * quick GELU x / (1 + __expf(-1.702 x)): the exponent a = 1.702 |x| (rounded constant, two products: 2u relative) moves
#     E = exp(-1.702 x) by a 2u, exp 4u, so s = 1 / (1 + E) has relative error eps_s <= (2a + 4) u (1 - s) + 4u (sum, division).
#     Where E overflows (x < -52) the kernel returns -0 for a value below 1e-36: an absolute 2^-100 covers it.
AS_PHI = 7.5e-8
X2_EXTRA = 6.0e-8
U = 2.0 ** -24
LN2 = math.log(2.0)
FLOOR = 2.0 ** -100


def _phi(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def _cdf_err(x, lean):
    q = 0.5 * torch.special.erfc(x.abs() / math.sqrt(2.0))
    xs = x * x * (0.5 / LN2)
    return AS_PHI + (X2_EXTRA if lean else 0.0) + q * (130.0 + 3.0 * LN2 * xs) * U + 2.0 * U, xs


def f_gelu(x, lean):
    f = x * _phi(x)
    ec, _ = _cdf_err(x, lean)
    return f, x.abs() * ec + 2.0 * U * f.abs()


def f_dgelu(x, lean):
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    d = _phi(x) + x * pdf
    ec, xs = _cdf_err(x, lean)
    return d, ec + (x * pdf).abs() * (7.0 + 3.0 * LN2 * xs) * U + 2.0 * U * d.abs()


def _sig_err(x):
    s = torch.sigmoid(1.702 * x)
    return s, (2.0 * 1.702 * x.abs() + 4.0) * U * (1.0 - s) + 4.0 * U


def f_quick(x):
    s, es = _sig_err(x)
    f = x * s
    return f, f.abs() * (es + U) + FLOOR


def f_dquick(x):
    s, es = _sig_err(x)
    k = 1.702 * x
    d = s + k * s * (1.0 - s)
    return d, s * es + k.abs() * s * (s * es + 2.0 * U) + (k * s * (1.0 - s)).abs() * (es + 4.0 * U) + U * d.abs() + FLOOR


def check_bounded(out, f, err, fmt):
    """|out - f| <= err + half a `fmt` spacing at the output (the final rounding).  Returns the worst share of the evaluation bound
    `err` that an element uses beyond that half spacing, (|out - f| - spacing / 2) / err, which must be <= 1."""
    o = out.double()
    assert not bool(torch.isnan(o).any())
    half = 0.5 * quantum16(torch.maximum(o.abs(), f.abs() + err), fmt)
    ratio = float((((o - f).abs() - half) / err).max())
    assert ratio <= 1.0, f'worst (error - rounding) / evaluation bound = {ratio:.3f}'
    return ratio
