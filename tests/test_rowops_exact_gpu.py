"""GPU: the row movers of csrc/rowops.hip element-wise against fp64 -- reid_layernorm_fwd, reid_add_layernorm_fwd, reid_patch_im2col,
reid_cls_rows, reid_cast_f32_bf16, reid_cast_bf16_f32, reid_gather_rows_f32, reid_scatter_add_rows_f32, reid_embed_tokens,
reid_l2norm_rows and reid_pack_bf16_table -- and the arguments they refuse.

Method of test_gemm_exact_gpu.py.  Permutations, copies and sums get operands that are small integers times a power of two (16-bit
representable where the output is 16-bit, a checked bit budget where terms are added): fp32 outputs must EQUAL the fp64 reference,
16-bit outputs its round-to-nearest-even (helpers.round16).  LayerNorm and the L2 norm round: every element is held to its own
allowance derived from the operation count (rowops_refs.py; the statistics against fp64, y against fp64 built from the kernel's own
statistics, a 16-bit output one more half spacing), never to a global maximum.  Outputs live in sentinel buffers with 8 padding columns
and 32 guard rows that must keep the sentinel; a second identical call gives the same bits; refused calls leave the outputs untouched."""
import pytest
import torch

import rowops_refs as R
from helpers import U, assert_bit_budget, count_ties16, exact_ints, is_sentinel, quantum16, round16, sentinel_buffer

pytestmark = pytest.mark.gpu

GUARD = 32
COLS = (4, 8, 64, 260, 512, 768, 772, 1024)      # 260 / 772: one lane reaches into the next float4 vector of the lanes


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    """Every test runs once per build flavor (libreid_hip.so = bf16 operands, libreid_hip_f16.so = f16)."""
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


def padded(vals, dtype=torch.float32, fmt=None, pad=8):
    """Device operand with the values of float64 `vals` [rows, cols], exactly, in the first columns of a [rows, cols + pad] sentinel buffer."""
    rows, cols = vals.shape
    buf = sentinel_buffer(rows, cols + pad, dtype, fmt)
    v = vals.to(dtype)
    assert torch.equal(v.double(), vals), f'operand not representable in {dtype}'
    buf[:, :cols] = v
    return buf[:, :cols]


def guarded(rows, cols, dtype=torch.float32, fmt=None):
    """(buffer, view): [rows + GUARD, cols + 8] sentinel buffer and its leading [rows, cols] block."""
    buf = sentinel_buffer(rows + GUARD, cols + 8, dtype, fmt)
    return buf, buf[:rows, :cols]


def untouched(buf, rows, cols, fmt=None):
    s = is_sentinel(buf, fmt)
    return bool(s[rows:].all() and s[:rows, cols:].all())


def flat_guarded(n, dtype=torch.float32, fmt=None):
    buf = sentinel_buffer(1, n + 64, dtype, fmt)[0]
    return buf, buf[:n]


def bits_of(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).clone()


def half_spacing(got, ref, allow, fmt):
    return 0.5 * quantum16(torch.maximum(got.double().abs(), ref.abs() + allow), fmt)


def assert_refused(fn, outputs):
    """`fn` must raise the argument error before any launch: every output (buffer, fmt) still holds its sentinel."""
    from prcv2025reid_amd._lib import ReidHipError
    with pytest.raises(ReidHipError):
        fn()
    torch.cuda.synchronize()
    for buf, fmt in outputs:
        assert bool(is_sentinel(buf, fmt).all())


# ------------------------------------------------------------------------------------------------------------- LayerNorm forward
def _ln_run(ops, x, gamma, beta, rows, cols, fmt, want_b=True, want_f=True, want_stats=True, row_index=None, eps=1e-5):
    bb, yb = guarded(rows, cols, T16(), fmt)
    fb, yf = guarded(rows, cols)
    mb, mean = flat_guarded(rows)
    rb, rstd = flat_guarded(rows)
    ops.layernorm_fwd(x, gamma, beta, y_bf16=yb if want_b else None, y_f32=yf if want_f else None, mean=mean if want_stats else None,
                      rstd=rstd if want_stats else None, row_index=row_index, eps=eps)
    torch.cuda.synchronize()
    return dict(bb=bb, yb=yb, fb=fb, yf=yf, mb=mb, mean=mean, rb=rb, rstd=rstd)


def _ln_check(o, x64, gamma, beta, rows, cols, fmt, what, eps=1e-5):
    g64, b64 = gamma.double(), beta.double()
    mu, dm, rstd, dr = R.ln_stats_ref(x64, R.f32(eps))
    R.assert_within(o['mean'], mu, dm, f'{what} mean')
    R.assert_within(o['rstd'], rstd, dr, f'{what} rstd')
    y, allow = R.ln_y_ref(x64, o['mean'].double(), o['rstd'].double(), g64, b64)
    R.assert_within(o['yf'], y, allow, f'{what} y_f32')
    R.assert_within(o['yb'], y, allow, f'{what} y_16', half_spacing(o['yb'], y, allow, fmt))
    assert untouched(o['fb'], rows, cols) and untouched(o['bb'], rows, cols, fmt), what
    assert bool(is_sentinel(o['mb'][rows:]).all() and is_sentinel(o['rb'][rows:]).all()), what


def _same_bits(a, b, keys):
    return all(torch.equal(bits_of(a[k]), bits_of(b[k])) for k in keys)


@pytest.mark.parametrize('cols', COLS)
def test_layernorm_fwd_per_element(ops, cols):
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(cols)
    gamma = torch.randn(cols, generator=gen, device='cuda') + 1.0
    beta = torch.randn(cols, generator=gen, device='cuda')
    for rows in (1, 3, 5):
        for fam in R.LN_FAMILIES:
            x = R.ln_family(fam, rows, cols, gen)
            xv = padded(x.double())
            o = _ln_run(ops, xv, gamma, beta, rows, cols, fmt)
            _ln_check(o, x.double(), gamma, beta, rows, cols, fmt, f'{fam} rows={rows}')
            assert _same_bits(o, _ln_run(ops, xv, gamma, beta, rows, cols, fmt), ('bb', 'fb', 'mb', 'rb')), fam
        # a constant row of an exactly summable value: mean = the value, the centred pass sees zeros: rstd = rsqrt(eps), y = beta
        c = torch.full((rows, cols), 3.0, dtype=torch.float64, device='cuda')
        o = _ln_run(ops, padded(c), gamma, beta, rows, cols, fmt)
        _ln_check(o, c, gamma, beta, rows, cols, fmt, f'constant rows={rows}')
        assert bool((o['mean'] == 3.0).all())
        e32 = R.f32(1e-5)
        assert float((o['rstd'].double() - e32 ** -0.5).abs().max()) <= 5 * U * e32 ** -0.5
        assert torch.equal(o['yf'], beta.expand(rows, cols))
        assert torch.equal(o['yb'].double(), round16(beta.double(), fmt).expand(rows, cols))
    # output combinations: each must give the bits of the call that writes everything, and leave the rest alone
    x = R.ln_family('mean10', 5, cols, gen)
    xv = padded(x.double())
    full = _ln_run(ops, xv, gamma, beta, 5, cols, fmt)
    only_b = _ln_run(ops, xv, gamma, beta, 5, cols, fmt, want_f=False)
    assert _same_bits(full, only_b, ('bb', 'mb', 'rb')) and bool(is_sentinel(only_b['fb']).all())
    only_f = _ln_run(ops, xv, gamma, beta, 5, cols, fmt, want_b=False)
    assert _same_bits(full, only_f, ('fb', 'mb', 'rb')) and bool(is_sentinel(only_f['bb'], fmt).all())
    no_stats = _ln_run(ops, xv, gamma, beta, 5, cols, fmt, want_stats=False)
    assert _same_bits(full, no_stats, ('bb', 'fb')) and bool(is_sentinel(no_stats['mb']).all() and is_sentinel(no_stats['rb']).all())


@pytest.mark.parametrize('cols', [260, 768])
def test_layernorm_fwd_row_index(ops, cols):
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(cols + 1)
    gamma = torch.randn(cols, generator=gen, device='cuda') + 1.0
    beta = torch.randn(cols, generator=gen, device='cuda')
    x = R.ln_family('outlier', 36, cols, gen) + torch.arange(36, device='cuda')[:, None]       # every row its own mean
    xv = padded(x.double())
    for name, idx in (('repeated', [3, 3, 0, 3, 35]), ('descending', [6, 5, 4, 3, 2, 1, 0]), ('every 7th', [0, 7, 14, 21, 28, 35])):
        ri = torch.tensor(idx, dtype=torch.int32, device='cuda')
        o = _ln_run(ops, xv, gamma, beta, len(idx), cols, fmt, row_index=ri)
        _ln_check(o, x.double()[ri.long()], gamma, beta, len(idx), cols, fmt, name)
        assert _same_bits(o, _ln_run(ops, xv, gamma, beta, len(idx), cols, fmt, row_index=ri), ('bb', 'fb', 'mb', 'rb')), name


def _ln_refusal_args(cols, ldx_of):
    x = torch.zeros(4, max(cols, 8) + 16, device='cuda')
    return torch.as_strided(x, (4, cols), (ldx_of, 1))


def test_layernorm_fwd_refusals(ops):
    fmt = flavor()
    for cols, ldx, ldy in ((6, 8, 8), (1028, 1028, 1028), (64, 66, 72), (64, 72, 66), (64, 60, 72), (64, 72, 60)):
        x = _ln_refusal_args(cols, ldx)
        g = torch.ones(cols, device='cuda')
        fb = sentinel_buffer(4, max(cols, ldy) + 16, torch.float32); bb = sentinel_buffer(4, max(cols, ldy) + 16, T16(), fmt)
        yf = torch.as_strided(fb, (4, cols), (ldy, 1)); yb = torch.as_strided(bb, (4, cols), (ldy, 1))
        mb, mean = flat_guarded(4)
        assert_refused(lambda: ops.layernorm_fwd(x, g, g, y_bf16=yb, y_f32=yf, mean=mean, rstd=None), [(fb, None), (bb, fmt), (mb, None)])


# --------------------------------------------------------------------------------------------------- residual add + LayerNorm
ADD_LN_ROWS = [(1, None), (3, 1), (5, 2), (200, 197)]       # (rows, rows_per_img of row_scale or None)


@pytest.mark.parametrize('cols', COLS)
def test_add_layernorm_fwd_exact_sum_and_per_element_norm(ops, cols):
    """x_out = fma(scale[row / rows_per_img], y, x) EXACTLY on exact operands (y in the flavor's format and, in the bf16 flavor, as
    IEEE half: the Y_HALF instantiation), then the LayerNorm of it like reid_layernorm_fwd's."""
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(cols + 2)
    gamma = torch.randn(cols, generator=gen, device='cuda') + 1.0
    beta = torch.randn(cols, generator=gen, device='cuda')
    ydtypes = [(T16(), fmt)] + ([(torch.float16, 'f16')] if fmt == 'bf16' else [])
    for rows, rpi in ADD_LN_ROWS:
        for fam in ('plain', 'offset1000', 'outlier'):
            x64 = exact_ints((rows, cols), -8, 8, -2, gen)
            if fam == 'offset1000':
                x64 = x64 + 1000.0
            elif fam == 'outlier':
                x64[:, cols // 3] *= 128.0
            y64 = exact_ints((rows, cols), -4, 4, -2, gen)
            if rpi is None:
                scale, sc_rows = None, torch.ones(rows, dtype=torch.float64, device='cuda')
            else:
                n_img = (rows + rpi - 1) // rpi
                scale = torch.tensor([0.0, 0.5, 2.0, 1.0], device='cuda')[torch.arange(n_img, device='cuda') % 4].contiguous()
                sc_rows = scale.double().repeat_interleave(rpi)[:rows]
            xo64 = x64 + sc_rows[:, None] * y64
            assert_bit_budget(x64.abs() + 2.0 * y64.abs(), 2.0 ** -3)
            xv = padded(x64)
            for ydt, yfmt in ydtypes:
                what = f'{fam} rows={rows} y={ydt}'
                yv = padded(y64, ydt, yfmt)
                outs = []
                for rep in range(2):
                    xb, xo = guarded(rows, cols)
                    hb, h = guarded(rows, cols, T16(), fmt)
                    mb, mean = flat_guarded(rows)
                    rb, rstd = flat_guarded(rows)
                    ops.add_layernorm_fwd(xv, yv, xo, gamma, beta, h, mean=mean, rstd=rstd, row_scale=scale, rows_per_img=rpi or 0)
                    torch.cuda.synchronize()
                    outs.append(dict(xb=xb, hb=hb, mb=mb, rb=rb))
                assert torch.equal(xo.double(), xo64), what
                mu, dm, rs, dr = R.ln_stats_ref(xo64, R.f32(1e-5))
                R.assert_within(mean, mu, dm, f'{what} mean')
                R.assert_within(rstd, rs, dr, f'{what} rstd')
                yr, allow = R.ln_y_ref(xo64, mean.double(), rstd.double(), gamma.double(), beta.double())
                R.assert_within(h, yr, allow, f'{what} h', half_spacing(h, yr, allow, fmt))
                assert untouched(xb, rows, cols) and untouched(hb, rows, cols, fmt), what
                assert bool(is_sentinel(mb[rows:]).all() and is_sentinel(rb[rows:]).all()), what
                assert _same_bits(outs[0], outs[1], ('xb', 'hb', 'mb', 'rb')), what
        # mean / rstd not wanted: the same x_out and h
        xb2, xo2 = guarded(rows, cols); hb2, h2 = guarded(rows, cols, T16(), fmt)
        ops.add_layernorm_fwd(xv, yv, xo2, gamma, beta, h2, row_scale=scale, rows_per_img=rpi or 0)
        torch.cuda.synchronize()
        assert torch.equal(bits_of(xb2), bits_of(xb)) and torch.equal(bits_of(hb2), bits_of(hb))


def test_add_layernorm_fwd_refusals(ops):
    fmt = flavor()
    for cols, ldx, ldo in ((6, 8, 8), (1028, 1028, 1028), (64, 66, 72), (64, 72, 66), (64, 60, 72), (64, 72, 60)):
        x = _ln_refusal_args(cols, ldx)
        y = torch.zeros(4, max(cols, 8) + 16, dtype=T16(), device='cuda')[:, :cols]
        g = torch.ones(cols, device='cuda')
        xb = sentinel_buffer(4, max(cols, ldo) + 16, torch.float32); hb = sentinel_buffer(4, max(cols, ldo) + 16, T16(), fmt)
        xo = torch.as_strided(xb, (4, cols), (ldo, 1)); h = torch.as_strided(hb, (4, cols), (ldo, 1))
        assert_refused(lambda: ops.add_layernorm_fwd(x, y, xo, g, g, h), [(xb, None), (hb, fmt)])
    x = torch.zeros(4, 64, device='cuda'); y = torch.zeros(4, 64, dtype=T16(), device='cuda'); g = torch.ones(64, device='cuda')
    xb, xo = guarded(4, 64); hb, h = guarded(4, 64, T16(), fmt)
    assert_refused(lambda: ops.add_layernorm_fwd(x, y, xo, g, g, h, row_scale=torch.ones(4, device='cuda'), rows_per_img=0), [(xb, None), (hb, fmt)])


# ------------------------------------------------------------------------------------------------------------------- im2col
def _pixels(n, H, W, gen, mean_exact):
    """fp32 images [n, 3, H, W] of 16-bit-representable pixels (integers up to 100 times 2^-4); `mean_exact`: the third channel makes
    every channel sum a multiple of three whose third is such a pixel too."""
    img = torch.randint(-60, 61, (n, 3, H, W), generator=gen, device='cuda', dtype=torch.int32)
    if mean_exact:
        m = torch.randint(-40, 41, (n, H, W), generator=gen, device='cuda', dtype=torch.int32)
        img[:, 2] = 3 * m - img[:, 0] - img[:, 1]
    return img.float() * 2.0 ** -4


@pytest.mark.parametrize('cin', [3, 1])
@pytest.mark.parametrize('n,H,W,P', [(2, 224, 224, 16), (3, 32, 64, 16), (1, 16, 16, 8)])
def test_patch_im2col_exact(ops, n, H, W, P, cin):
    """A permutation (cin = 3) or an exact channel mean (cin = 1) of 16-bit-representable pixels: EQUAL to the unfold reference."""
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(H + W + P + cin)
    img = _pixels(n, H, W, gen, cin == 1)
    want = R.im2col_ref(img.double(), P, cin)
    assert torch.equal(round16(want, fmt), want)
    rows, kc = want.shape
    bits = []
    for rep in range(2):
        buf = sentinel_buffer(rows + GUARD, kc, T16(), fmt)
        ops.patch_im2col(img, buf[:rows], P, cin)
        torch.cuda.synchronize()
        bits.append(bits_of(buf))
    assert torch.equal(buf[:rows].double(), want)
    assert bool(is_sentinel(buf[rows:], fmt).all()) and torch.equal(bits[0], bits[1])


def test_patch_im2col_channel_mean_rounds_once(ops):
    """cin = 1 on arbitrary pixels: the sum of three is two fp32 additions (2u of sum|c| / 3), the division one (u), then one 16-bit rounding."""
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(5)
    img = torch.randn(3, 3, 32, 64, generator=gen, device='cuda')
    want = R.im2col_ref(img.double(), 16, 1)
    allow = 2 * U * R.im2col_ref(img.double().abs(), 16, 1) + U * want.abs()
    buf = sentinel_buffer(want.shape[0] + GUARD, 256, T16(), fmt)
    ops.patch_im2col(img, buf[:want.shape[0]], 16, 1)
    torch.cuda.synchronize()
    got = buf[:want.shape[0]]
    R.assert_within(got, want, allow, 'channel mean', half_spacing(got, want, allow, fmt))
    assert bool(is_sentinel(buf[want.shape[0]:], fmt).all())


def test_patch_im2col_grid_stride_tail(ops):
    """112 images of 224 x 224, cin = 3: 2 107 392 chunks of eight pixels, more than the 8192 x 256 threads of the capped grid."""
    fmt = flavor()
    n, H, P = 112, 224, 16
    assert n * (H // P) ** 2 * (3 * P * P // 8) > 8192 * 256
    gen = torch.Generator(device='cuda').manual_seed(9)
    img = torch.randint(-100, 101, (n, 3, H, H), generator=gen, device='cuda', dtype=torch.int16).float() * 2.0 ** -4
    rows, kc = n * (H // P) ** 2, 3 * P * P
    want = R.im2col_ref(img, P, 3).to(T16())                                                  # exact: the pixels are 16-bit numbers
    assert torch.equal(want.float(), R.im2col_ref(img, P, 3))
    buf = sentinel_buffer(rows + GUARD, kc, T16(), fmt)
    ops.patch_im2col(img, buf[:rows], P, 3)
    torch.cuda.synchronize()
    assert torch.equal(bits_of(buf[:rows]), bits_of(want))
    assert bool(is_sentinel(buf[rows:], fmt).all())


def test_patch_im2col_refusals(ops):
    fmt = flavor()
    img = torch.zeros(1, 3, 48, 48, device='cuda')
    buf = sentinel_buffer(64, 768, T16(), fmt)
    assert_refused(lambda: ops.patch_im2col(img, buf, 16, 2), [(buf, fmt)])                   # cin = 2
    assert_refused(lambda: ops.patch_im2col(img, buf, 12, 3), [(buf, fmt)])                   # patch = 12
    assert_refused(lambda: ops.patch_im2col(img[:, :, :40], buf, 16, 3), [(buf, fmt)])        # H = 40 is no multiple of 16


# ------------------------------------------------------------------------------------------------------------------- cls rows
@pytest.mark.parametrize('cols', [4, 768])
@pytest.mark.parametrize('tokens', [1, 50, 197])
def test_cls_rows_exact(ops, tokens, cols):
    n_img = 3
    gen = torch.Generator(device='cuda').manual_seed(tokens + cols)
    cls64 = exact_ints((1, cols), -64, 64, -3, gen); pos64 = exact_ints((1, cols), -64, 64, -3, gen)
    bits = []
    for rep in range(2):
        buf, x = guarded(n_img * tokens, cols)
        ops.cls_rows(cls64.float()[0], pos64.float()[0], x, n_img, tokens)
        torch.cuda.synchronize()
        bits.append(bits_of(buf))
    first = torch.arange(n_img, device='cuda') * tokens
    assert torch.equal(x[first].double(), (cls64 + pos64).expand(n_img, cols))
    other = torch.ones(n_img * tokens, dtype=torch.bool, device='cuda'); other[first] = False
    assert bool(is_sentinel(x[other]).all()) and untouched(buf, n_img * tokens, cols)
    assert torch.equal(bits[0], bits[1])


def test_cls_rows_refusals(ops):
    from prcv2025reid_amd import _lib as L
    v = torch.zeros(64, device='cuda')
    buf = sentinel_buffer(8, 72, torch.float32)
    for ldx, cols in ((60, 64), (66, 64), (72, 6)):                                          # ldx < cols, ldx % 4, cols % 4
        assert_refused(lambda: L.check(L.lib().reid_cls_rows(L.ptr(v), L.ptr(v), L.ptr(buf), ldx, 2, 2, cols, L.stream_ptr())), [(buf, None)])


# ------------------------------------------------------------------------------------------------------------------- casts
CAST_SIZES = [1, 7, 8, 9, 2047, 8192 * 256 * 8 + 5]       # the last: more 8-element vectors than the capped grid has threads, and a tail


def _cast_input(n, fmt, gen):
    """fp32 values with, at the front, ties of the 16-bit grid (both directions of ties-to-even), an fp32 subnormal, a value that is
    subnormal in IEEE half, one that saturates half, infinities and a NaN."""
    x = torch.randn(n, generator=gen, device='cuda') * 4.0
    g = torch.tensor([1.0, 1.0 + 2.0 ** (-7 if fmt == 'bf16' else -10), -3.0, 0.15625], dtype=torch.float64)
    ties = g + torch.copysign(0.5 * quantum16(g, fmt), g)
    special = torch.cat([ties, torch.tensor([1e-40, 3.1e-6, 65520.0, float('inf'), float('-inf'), float('nan'), -1e38], dtype=torch.float64)]).float()
    k = min(n, special.numel())
    x[:k] = special[:k].cuda()
    return x


@pytest.mark.parametrize('n', CAST_SIZES)
def test_cast_f32_to_16_is_round_to_nearest_even(ops, n):
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(n)
    x = _cast_input(n, fmt, gen)
    bits = []
    for rep in range(2):
        buf, dst = flat_guarded(n, T16(), fmt)
        ops.cast_f32_bf16(x, dst)
        torch.cuda.synchronize()
        bits.append(bits_of(buf))
    x64, got = x.double().cpu(), dst.double().cpu()
    fin = torch.isfinite(x64)
    assert count_ties16(x64[fin], fmt) >= 1
    assert torch.equal(got[fin], round16(x64[fin], fmt))
    assert torch.equal(got[torch.isinf(x64)], x64[torch.isinf(x64)]) and bool(torch.isnan(got[torch.isnan(x64)]).all())
    assert bool(is_sentinel(buf[n:], fmt).all()) and torch.equal(bits[0], bits[1])


@pytest.mark.parametrize('n', CAST_SIZES)
def test_cast_16_to_f32_exact(ops, n):
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(n + 1)
    src = torch.randint(-32768, 32768, (n,), generator=gen, device='cuda', dtype=torch.int32).to(torch.int16).view(T16())    # every bit pattern
    bits = []
    for rep in range(2):
        buf, dst = flat_guarded(n)
        ops.cast_bf16_f32(src, dst)
        torch.cuda.synchronize()
        bits.append(bits_of(buf))
    want = src.double()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(dst), nan) and torch.equal(dst.double()[~nan], want[~nan])
    assert torch.equal(torch.signbit(dst[~nan]), torch.signbit(want[~nan]))
    assert bool(is_sentinel(buf[n:]).all()) and torch.equal(bits[0], bits[1])


# ---------------------------------------------------------------------------------------------------- gather / scatter-add rows
@pytest.mark.parametrize('cols', [4, 768])
@pytest.mark.parametrize('rows', [1, 5, 300])
def test_gather_rows_exact(ops, rows, cols):
    gen = torch.Generator(device='cuda').manual_seed(rows + cols)
    src64 = exact_ints((40, cols), -1000, 1000, -5, gen)
    src = padded(src64)
    idx = torch.randint(0, 40, (rows,), generator=gen, device='cuda', dtype=torch.int32)
    if rows >= 5:
        idx[:5] = torch.tensor([39, 7, 7, 0, 7], dtype=torch.int32)                           # repeated, out of order, both ends
    bits = []
    for rep in range(2):
        buf, dst = guarded(rows, cols)
        ops.gather_rows(src, idx, dst)
        torch.cuda.synchronize()
        bits.append(bits_of(buf))
    assert torch.equal(dst.double(), src64[idx.long()])
    assert untouched(buf, rows, cols) and torch.equal(bits[0], bits[1])


@pytest.mark.parametrize('cols', [5, 768, 770])
def test_scatter_add_rows_exact(ops, cols):
    """out[index[r]] += src[r] with fp32 atomics on exact operands: EQUAL to fp64 and bit-identical on a second call whatever the order
    of the atomics; indices -1 and out_rows are skipped; padding columns, guard rows and untargeted rows keep their contents."""
    rows, out_rows = 300, 12
    gen = torch.Generator(device='cuda').manual_seed(cols)
    src64 = exact_ints((rows, cols), -16, 16, -3, gen)
    src = padded(src64)
    out064 = exact_ints((out_rows, cols), -64, 64, -3, gen)
    out064 = torch.where(out064 == 0, torch.full_like(out064, 0.125), out064)                 # a non-zero start everywhere
    one = torch.full((rows,), 2, dtype=torch.int32, device='cuda')
    heavy = torch.randint(1, out_rows, (rows,), generator=gen, device='cuda', dtype=torch.int32)
    heavy[torch.rand(rows, generator=gen, device='cuda') < 0.8] = 0                          # the pad id takes four rows of five
    skips = heavy.clone(); skips[::7] = -1; skips[3::7] = out_rows
    assert_bit_budget(out064.abs().max() + src64.abs().sum(0), 2.0 ** -3)
    for name, idx in (('one target', one), ('pad-heavy', heavy), ('skipped', skips)):
        ok = (idx >= 0) & (idx < out_rows)
        want = out064.clone().index_add_(0, idx[ok].long(), src64[ok])
        bits = []
        for rep in range(2):
            buf, out = guarded(out_rows, cols)
            out.copy_(out064.float())
            ops.scatter_add_rows(src, idx, out)
            torch.cuda.synchronize()
            bits.append(bits_of(buf))
        assert torch.equal(out.double(), want), name
        hit = torch.zeros(out_rows, dtype=torch.bool, device='cuda'); hit[idx[ok].long()] = True
        assert torch.equal(bits_of(out[~hit]), bits_of(out064.float()[~hit])), name
        assert untouched(buf, out_rows, cols) and torch.equal(bits[0], bits[1]), name


# ------------------------------------------------------------------------------------------------------------------- embed tokens
@pytest.mark.parametrize('D', [4, 512])
@pytest.mark.parametrize('T', [1, 77])
@pytest.mark.parametrize('B', [1, 3])
def test_embed_tokens_exact_and_clamped(ops, B, T, D):
    """out[b T + t] = tok[clamp(ids[b, t], 0, vocab - 1)] + pos[t] exactly; the clamp is the documented one (ids below 0 read row 0, ids
    at or above vocab -- an int64 beyond 2^31 among them -- read the last row)."""
    vocab = 50
    gen = torch.Generator(device='cuda').manual_seed(B * 100 + T + D)
    tok64 = exact_ints((vocab, D), -512, 512, -4, gen); pos64 = exact_ints((T, D), -512, 512, -4, gen)
    ids = torch.randint(0, vocab, (B, T), generator=gen, device='cuda', dtype=torch.int64)
    flat = ids.view(-1)
    special = torch.tensor([2 ** 31 + 7, -5, vocab, -2 ** 40, vocab - 1, 0], dtype=torch.int64, device='cuda')
    k = min(flat.numel(), special.numel())
    flat[-k:] = special[:k]
    bits = []
    for rep in range(2):
        buf = sentinel_buffer(B * T + GUARD, D, torch.float32)
        ops.embed_tokens(tok64.float(), pos64.float(), ids, buf[:B * T])
        torch.cuda.synchronize()
        bits.append(bits_of(buf))
    want = tok64[ids.clamp(0, vocab - 1).view(-1)] + pos64.repeat(B, 1)
    assert torch.equal(buf[:B * T].double(), want)
    assert bool(is_sentinel(buf[B * T:]).all()) and torch.equal(bits[0], bits[1])


# ------------------------------------------------------------------------------------------------------------------- l2norm rows
@pytest.mark.parametrize('D', [4, 512, 1024])
@pytest.mark.parametrize('rows', [1, 5])
def test_l2norm_rows_per_element(ops, rows, D):
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(rows * 7 + D)
    x = torch.randn(rows, D, generator=gen, device='cuda') * 3.0
    if rows == 5:
        x[1] = 0.0                                                                            # a zero row gives 0
        x[2] *= 2.0 ** -50                                                                    # norm below eps: y = x scale / eps
        x[3, 1:] = 0.0                                                                        # one non-zero element: y = +-scale
    xv = padded(x.double())
    eps = R.f32(1e-12)
    for scale in (1.0, 8.0):
        want, allow = R.l2norm_ref(x.double(), eps, scale)
        if rows == 5:
            assert float((want[2] - x[2].double() * scale / eps).abs().max()) <= 1e-15 * float(want[2].abs().max())
        res = {}
        for combo in ('both', 'both', 'f32', '16'):
            fb, y = guarded(rows, D)
            bb, yb = guarded(rows, D, T16(), fmt)
            ops.l2norm_rows(xv, y=y if combo != '16' else None, y_bf16=yb if combo != 'f32' else None, eps=1e-12, scale=scale)
            torch.cuda.synchronize()
            if combo in res:
                assert torch.equal(bits_of(fb), res[combo][0]) and torch.equal(bits_of(bb), res[combo][1])      # repeat call
            res[combo] = (bits_of(fb), bits_of(bb))
            if combo != '16':
                R.assert_within(y, want, allow, f'y scale={scale} {combo}')
                assert untouched(fb, rows, D)
                if rows == 5:
                    assert float(y[1].abs().max()) == 0.0
            else:
                assert bool(is_sentinel(fb).all())
            if combo != 'f32':
                R.assert_within(yb, want, allow, f'y16 scale={scale} {combo}', half_spacing(yb, want, allow, fmt))
                assert untouched(bb, rows, D, fmt)
                if rows == 5:
                    assert float(yb[1].double().abs().max()) == 0.0
            else:
                assert bool(is_sentinel(bb, fmt).all())
        assert torch.equal(res['both'][0], res['f32'][0]) and torch.equal(res['both'][1], res['16'][1])


def test_l2norm_rows_refusals(ops):
    fmt = flavor()
    for D, ldx, ldy in ((64, 66, 72), (64, 72, 66), (64, 60, 72), (64, 72, 60), (6, 8, 8), (1028, 1028, 1028)):
        x = _ln_refusal_args(D, ldx)
        fb = sentinel_buffer(4, max(D, ldy) + 16, torch.float32); bb = sentinel_buffer(4, max(D, ldy) + 16, T16(), fmt)
        y = torch.as_strided(fb, (4, D), (ldy, 1)); yb = torch.as_strided(bb, (4, D), (ldy, 1))
        assert_refused(lambda: ops.l2norm_rows(x, y=y, y_bf16=yb), [(fb, None), (bb, fmt)])


# ------------------------------------------------------------------------------------------------------------------- pack table
PACK_SHAPES = [(1, 1), (1, 3072), (8, 3072), (768, 8), (64, 768)]       # 8 x 3072 = 24 576 elements: three trips of the 32 x 256 threads
GAP = 16


def _pack_case(ops, entries, fmt, exact, seed):
    """entries: [(rows, cols, plain, transposed)].  Sources and destinations are laid out one after another with GAP sentinel elements
    between the destination regions; returns nothing, asserts everything."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    table, so, do = [], 3, GAP
    for rows, cols, plain, transposed in entries:
        n = rows * cols
        d0 = dT = -1
        if plain:
            d0, do = do, do + n + GAP
        if transposed:
            dT, do = do, do + n + GAP
        table.append([so, rows, cols, d0, dT])
        so += n + 5
    if exact:
        src64 = exact_ints((so,), -100, 100, -4, gen)
    else:
        src64 = (torch.randn(so, generator=gen, device='cuda') * 3.0).double()
    src = src64.float()
    tab = torch.tensor(table, dtype=torch.int64, device='cuda')
    bits = []
    for rep in range(2):
        dst = sentinel_buffer(1, do + 64, T16(), fmt)[0]
        ops.pack_bf16_table(src, dst, tab, len(entries))
        torch.cuda.synchronize()
        bits.append(bits_of(dst))
    owned = torch.zeros(do + 64, dtype=torch.bool, device='cuda')
    for s0, rows, cols, d0, dT in table:
        n = rows * cols
        want = round16(src64[s0:s0 + n], fmt)
        if exact:
            assert torch.equal(want, src64[s0:s0 + n])
        if d0 >= 0:
            assert torch.equal(dst[d0:d0 + n].double(), want), (rows, cols, 'plain')
            owned[d0:d0 + n] = True
        if dT >= 0:
            assert torch.equal(dst[dT:dT + n].double().view(cols, rows), want.view(rows, cols).t()), (rows, cols, 'transposed')
            owned[dT:dT + n] = True
    assert bool(is_sentinel(dst[~owned], fmt).all())                                           # the gaps, and everything after the last region
    assert int((~owned).sum()) >= GAP * (len(entries) + 1)
    assert torch.equal(bits[0], bits[1])


@pytest.mark.parametrize('mode', ['plain', 'transposed', 'both'])
@pytest.mark.parametrize('rows,cols', PACK_SHAPES)
def test_pack_bf16_table_single_entry_exact(ops, rows, cols, mode):
    _pack_case(ops, [(rows, cols, mode != 'transposed', mode != 'plain')], flavor(), True, rows + cols)


def test_pack_bf16_table_five_entries(ops):
    fmt = flavor()
    entries = [(1, 1, True, True), (1, 3072, False, True), (8, 3072, True, True), (768, 8, True, False), (64, 768, True, True)]
    _pack_case(ops, entries, fmt, True, 1)
    _pack_case(ops, entries, fmt, False, 2)                                                   # arbitrary fp32 values: round-to-nearest-even


def test_pack_bf16_table_refusals(ops):
    fmt = flavor()
    dst = sentinel_buffer(1, 64, T16(), fmt)[0]
    src = torch.zeros(16, device='cuda'); tab = torch.tensor([[0, 2, 2, 0, -1]], dtype=torch.int64, device='cuda')
    assert_refused(lambda: ops.pack_bf16_table(src, dst, tab, 0), [(dst, fmt)])
    assert_refused(lambda: ops.pack_bf16_table(src, dst, None, 1), [(dst, fmt)])
