"""GPU: the non-loss kernels of csrc/head.hip element-wise against fp64 -- reid_sgemm (both instantiations), reid_eltwise_f32,
reid_small_attn_fwd / bwd and reid_masked_mean -- and the arguments the entry points refuse.

Method of test_gemm_exact_gpu.py.  Where the operation is a sum of products, the operands are small integers times a power of two with
a checked bit budget: every partial sum is exact in fp32 in any order (K split over 4 or 8 waves, the in-LDS reduction), fp32 outputs
must EQUAL the fp64 reference.  Where roundings are unavoidable (GELU, softmax, one division) every element has its own allowance,
derived from the operation count (helpers.f_gelu / f_quick, rowops_refs.attn_fwd_allow / attn_bwd_ref); never a global maximum.
Outputs live in sentinel buffers with 8 padding columns and 32 guard rows, which must keep the sentinel; a second identical call
gives the same bits; refused calls leave every output untouched."""
import pytest
import torch

import rowops_refs as R
from helpers import U, assert_bit_budget, check_bounded, exact_ints, f_dgelu, f_gelu, f_quick, is_sentinel, sentinel_buffer

pytestmark = pytest.mark.gpu

GUARD = 32


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    """Every test runs once per build flavor (libreid_hip.so = bf16 operands, libreid_hip_f16.so = f16)."""
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


def padded32(vals, pad=8, off=0):
    """fp32 device operand with the values of float64 `vals` [rows, cols] as a column block of a [rows, cols + pad] sentinel buffer."""
    rows, cols = vals.shape
    buf = sentinel_buffer(rows, cols + pad, torch.float32)
    v = vals.float()
    assert torch.equal(v.double(), vals), 'operand not representable in fp32'
    buf[:, off:off + cols] = v
    return buf[:, off:off + cols]


def guarded(rows, cols, off=0):
    """(buffer, view): [rows + GUARD, cols + 8] fp32 sentinel buffer and its [rows, cols] block at column `off`."""
    buf = sentinel_buffer(rows + GUARD, cols + 8, torch.float32)
    return buf, buf[:rows, off:off + cols]


def untouched(buf, rows, cols, off=0):
    """Everything of `buf` outside the [rows, cols] block at column `off` still holds the sentinel."""
    s = is_sentinel(buf)
    return bool(s[rows:].all() and s[:rows, :off].all() and s[:rows, off + cols:].all())


def flat_guarded(n):
    buf = sentinel_buffer(1, n + 64, torch.float32)[0]
    return buf, buf[:n]


# ------------------------------------------------------------------------------------------------------------------- reid_sgemm
# tiles = ceil(M / 32) ceil(N / 32): at most 256 -> sgemm_kernel<8> (K split over 8 waves), more -> sgemm_kernel<4>
def _tiles(M, N):
    return ((M + 31) // 32) * ((N + 31) // 32)


SGEMM_CASES = [
    # name, M, N, K, kwargs
    ('NN', 70, 130, 100, {}), ('NT', 70, 130, 100, dict(tb=True)), ('TN', 70, 130, 100, dict(ta=True)), ('TT', 70, 130, 100, dict(ta=True, tb=True)),
] + [(f'w8-K{K}', 33, 33, K, dict(tb=bool(K & 1))) for K in (1, 15, 16, 17, 33, 127, 128, 129, 2048)] + [
    ('w8-256tiles', 512, 512, 16, {}), ('w4-272tiles', 513, 512, 16, {}),
] + [(f'w4-ones-K{K}', 1, 8229, K, dict(bias=False)) for K in (1, 7, 64, 65)] + [
    ('w4-545', 545, 545, 48, dict(tb=True)), ('w4-545-TT-K65', 545, 545, 65, dict(ta=True, tb=True)), ('w4-545-K128', 545, 545, 128, dict(ta=True)),
    ('views', 70, 130, 100, dict(views=True)), ('views-TT', 70, 130, 100, dict(views=True, ta=True, tb=True)),
    ('w4-views', 1, 8229, 65, dict(views=True, bias=False)),
    ('alpha', 70, 130, 100, dict(alpha=0.5)), ('beta2', 70, 130, 100, dict(beta=2.0)), ('alpha-beta2-nobias', 33, 33, 129, dict(alpha=0.5, beta=2.0, bias=False)),
    ('nobias', 70, 130, 100, dict(bias=False)), ('w4-beta2', 545, 545, 48, dict(beta=2.0)),
    ('relu', 70, 130, 100, dict(act='relu')), ('relu-beta2', 70, 130, 100, dict(act='relu', beta=2.0)), ('w4-relu', 1, 8229, 65, dict(act='relu')),
    ('gelu', 70, 130, 100, dict(act='gelu')), ('quick_gelu', 70, 130, 100, dict(act='quick_gelu')),
    ('w4-gelu', 545, 545, 48, dict(act='gelu')), ('w4-quick_gelu', 545, 545, 48, dict(act='quick_gelu', bias=False)),
]


def test_sgemm_cases_reach_both_instantiations():
    t = {c[0]: _tiles(c[1], c[2]) for c in SGEMM_CASES}
    assert t['w8-256tiles'] == 256 and t['w4-272tiles'] == 272 and t['w4-ones-K1'] == 258 and t['w4-545'] == 324 and t['NN'] == 15
    assert all((n.startswith('w4')) == (v > 256) for n, v in t.items())


@pytest.mark.parametrize('name,M,N,K,kw', SGEMM_CASES, ids=[c[0] for c in SGEMM_CASES])
def test_sgemm_exact(ops, name, M, N, K, kw):
    """C = act(alpha op(A) op(B) + bias) + beta C0 EQUALS fp64 (none, relu) or lies inside the GELU budget of the exact pre-activation;
    beta = 0 runs over a sentinel-filled C (a NaN pattern: reading it would show); padding and guard rows keep the sentinel."""
    ta, tb, views = kw.get('ta', False), kw.get('tb', False), kw.get('views', False)
    alpha, beta, act, has_bias = kw.get('alpha', 1.0), kw.get('beta', 0.0), kw.get('act', 'none'), kw.get('bias', True)
    gen = torch.Generator(device='cuda').manual_seed(M * 7 + N * 3 + K)
    A64 = exact_ints((K, M) if ta else (M, K), -4, 4, -2, gen)
    B64 = exact_ints((N, K) if tb else (K, N), -4, 4, -2, gen)
    bias64 = exact_ints((N,), -4, 4, -2, gen) if has_bias else None
    C064 = exact_ints((M, N), -4, 4, -2, gen)
    opA, opB = (A64.t() if ta else A64), (B64.t() if tb else B64)
    budget = alpha * (opA.abs() @ opB.abs()) + abs(beta) * C064.abs()
    if has_bias:
        budget = budget + bias64.abs()
    assert_bit_budget(budget, 2.0 ** -5)
    pre = alpha * (opA @ opB)
    if has_bias:
        pre = pre + bias64
    A = padded32(A64, 24, 8) if views else A64.float()
    B = padded32(B64, 24, 8) if views else B64.float()
    bias = bias64.float() if has_bias else None
    off = 4 if views else 0
    bits = []
    for rep in range(2):
        buf, C = guarded(M, N, off)
        if beta != 0.0:
            C.copy_(C064.float())
        ops.sgemm(A, B, C, ta=ta, tb=tb, alpha=alpha, beta=beta, bias=bias, act=act)
        torch.cuda.synchronize()
        bits.append(buf.view(torch.int32).clone())
    got = C.double()
    if act in ('none', 'relu'):
        want = (pre.clamp_min(0.0) if act == 'relu' else pre) + beta * C064
        assert torch.equal(got, want), f'{int((got != want).sum())} of {M * N} elements differ'
    else:
        assert beta == 0.0
        f, err = f_gelu(pre, False) if act == 'gelu' else f_quick(pre)
        check_bounded(C, f, err, 'f32')
    assert untouched(buf, M, N, off)
    assert torch.equal(bits[0], bits[1])


def test_sgemm_relu_passes_nan_like_torch(ops):
    """torch.relu(NaN) is NaN (fmaxf(NaN, 0) would be 0): the epilogue must not hide a diverged activation (models/model.py:42)."""
    gen = torch.Generator(device='cuda').manual_seed(1)
    A = exact_ints((40, 20), -4, 4, -2, gen).float(); B = exact_ints((20, 50), -4, 4, -2, gen).float()
    A[3, 5] = float('nan'); A[7, 0] = float('inf')
    buf, C = guarded(40, 50)
    ops.sgemm(A, B, C, act='relu')
    torch.cuda.synchronize()
    want = torch.relu((A.cpu().double()[:, :, None] * B.cpu().double()[None]).sum(1))       # products and sums written out: no BLAS shortcuts
    got = C.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got[3]).all())
    assert torch.equal(got[~torch.isnan(want)], want[~torch.isnan(want)])
    assert untouched(buf, 40, 50)


def test_sgemm_refusals(ops):
    from prcv2025reid_amd import _lib as L
    A = torch.zeros(8, 8, device='cuda'); B = torch.zeros(8, 8, device='cuda')
    buf, C = guarded(8, 8)

    def raw(M, N, K, ldc, act):
        return L.lib().reid_sgemm(L.ptr(A), L.ptr(B), L.ptr(C), M, N, K, 8, 1, 8, 1, ldc, 1.0, 0.0, None, act, L.stream_ptr())
    for args in ((8, 8, 8, 16, 9), (8, 8, 8, 16, -1), (8, 8, 8, 7, 0), (8, 8, 0, 16, 0)):     # act out of range, ldc < N, K = 0
        with pytest.raises(L.ReidHipError):
            L.check(raw(*args))
    torch.cuda.synchronize()
    assert bool(is_sentinel(buf).all())
    L.check(raw(8, 8, 8, 16, 0))                                                              # the same call with good arguments runs
    torch.cuda.synchronize()
    assert float(C.abs().max()) == 0.0 and untouched(buf, 8, 8)


# ------------------------------------------------------------------------------------------------------------- reid_eltwise_f32
ELT_SIZES = [1, 255, 256, 257, 4096 * 256 + 3]          # the last exceeds the grid cap of 4096 workgroups: the stride loop runs


def _elt(ops, op, x, y, n, alpha=1.0):
    """Run op twice into guarded buffers; returns the result after the tail-sentinel and repeat checks."""
    bits = []
    for rep in range(2):
        buf, out = flat_guarded(n)
        ops.eltwise(op, x, y, out=out, alpha=alpha)
        torch.cuda.synchronize()
        bits.append(buf.view(torch.int32).clone())
    assert bool(is_sentinel(buf[n:]).all()), op
    assert torch.equal(bits[0], bits[1]), op
    return out


@pytest.mark.parametrize('n', ELT_SIZES)
def test_eltwise_exact_ops(ops, n):
    gen = torch.Generator(device='cuda').manual_seed(n)
    x64 = exact_ints((n,), -24, 24, -2, gen); y64 = exact_ints((n,), -24, 24, -2, gen)
    x, y = x64.float(), y64.float()
    assert torch.equal(_elt(ops, 'add', x, y, n, alpha=0.5).double(), x64 + 0.5 * y64)
    assert torch.equal(_elt(ops, 'mul', x, y, n).double(), x64 * y64)
    assert torch.equal(_elt(ops, 'relu', x, None, n).double(), x64.clamp_min(0.0))
    assert torch.equal(_elt(ops, 'relu_bwd', x, y, n).double(), torch.where(x64 > 0, y64, torch.zeros_like(y64)))


@pytest.mark.parametrize('n', ELT_SIZES)
def test_eltwise_gelu_within_budget(ops, n):
    gen = torch.Generator(device='cuda').manual_seed(n + 1)
    x64 = exact_ints((n,), -24, 24, -2, gen); y64 = exact_ints((n,), -24, 24, -2, gen)      # x in [-6, 6]
    f, err = f_gelu(x64, False)
    check_bounded(_elt(ops, 'gelu', x64.float(), None, n), f, err, 'f32')
    d, derr = f_dgelu(x64, False)
    f = y64 * d
    check_bounded(_elt(ops, 'gelu_bwd', x64.float(), y64.float(), n), f, y64.abs() * derr + U * f.abs() + 2.0 ** -100, 'f32')


@pytest.mark.parametrize('n', ELT_SIZES)
def test_eltwise_keep_mask_and_nan_to_num(ops, n):
    gen = torch.Generator(device='cuda').manual_seed(n + 2)
    u64 = exact_ints((n,), 0, 7, -3, gen)                                                     # uniform draws on a grid that contains p
    u64[0] = 0.25
    u = u64.float()
    keep = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(0.75, dtype=torch.float32)   # the kernel's 1.0f / (1.0f - p)
    want = torch.where(u64 >= 0.25, keep.double().cuda(), torch.zeros_like(u64))               # u == p is kept
    got = _elt(ops, 'keep_mask', u, None, n, alpha=0.25)
    assert torch.equal(got.double(), want) and float(got[0]) == float(keep)
    assert torch.equal(_elt(ops, 'keep_mask', u, None, n, alpha=0.0).double(), torch.ones_like(u64))
    inplace = u.clone()                                                                       # model.py: out is x
    ops.eltwise('keep_mask', inplace, out=inplace, alpha=0.25)
    torch.cuda.synchronize()
    assert torch.equal(inplace.double(), want)
    special = torch.tensor([float('nan'), float('inf'), float('-inf'), 3e38, -3e38, 1e-40, -1e-45, 0.0, -0.0, 1.5], dtype=torch.float32)
    x = special.repeat((n + 9) // 10)[:n].cuda()
    want = torch.nan_to_num(x.cpu(), nan=0.0, posinf=1e4, neginf=-1e4)
    got = _elt(ops, 'nan_to_num', x, None, n).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))                         # bit for bit: subnormals, 3e38 and -0 stay
    if n >= 10:
        assert float(got[0]) == 0.0 and float(got[1]) == 1e4 and float(got[2]) == -1e4 and float(got[3]) == float(special[3])
        assert float(got[5]) == float(special[5]) != 0.0


def test_eltwise_relu_non_finite_is_torch(ops):
    """relu and its backward on NaN / inf: what torch does (relu(NaN) = NaN; the gradient passes where x is NaN or +inf)."""
    xc = torch.tensor([float('nan'), float('inf'), float('-inf'), -1.0, 2.0, 0.0, float('nan')], dtype=torch.float32, requires_grad=True)
    dyc = torch.tensor([3.0, 3.0, 3.0, 3.0, float('nan'), float('nan'), float('inf')], dtype=torch.float32)
    yc = torch.relu(xc)
    yc.backward(dyc)
    n = xc.numel()
    got = _elt(ops, 'relu', xc.detach().cuda(), None, n).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(yc.detach())) and bool(torch.isnan(got[0]))
    assert torch.equal(got[~torch.isnan(got)], yc.detach()[~torch.isnan(got)])
    gb = _elt(ops, 'relu_bwd', xc.detach().cuda(), dyc.cuda(), n).cpu()
    assert torch.equal(torch.isnan(gb), torch.isnan(xc.grad))
    assert torch.equal(gb[~torch.isnan(gb)], xc.grad[~torch.isnan(gb)]) and float(gb[0]) == 3.0


def test_eltwise_refusals(ops):
    from prcv2025reid_amd import _lib as L
    x = torch.zeros(16, device='cuda')
    buf, out = flat_guarded(16)
    for op, y, n in ((8, x, 16), (-1, x, 16), (0, None, 16), (2, None, 16), (1, None, 0)):    # op out of range, missing operand, n = 0
        with pytest.raises(L.ReidHipError):
            L.check(L.lib().reid_eltwise_f32(op, L.ptr(x), L.ptr(y), L.ptr(out), n, 1.0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool(is_sentinel(buf).all())


# ---------------------------------------------------------------------------------------------------------- reid_small_attn
def _attn_buffers(qkv64, n_seq, S, heads):
    """qkv as a column block (offset 4) of a wider sentinel buffer; guarded out / dqkv and a guarded probs [items + GUARD, 8, 8]."""
    d = heads * 64
    qkv = padded32(qkv64, 8, 4)
    obuf, out = guarded(n_seq * S, d, 4)
    pbuf = sentinel_buffer(n_seq * heads + GUARD, 64, torch.float32)
    return qkv, obuf, out, pbuf, pbuf[:n_seq * heads].view(n_seq * heads, 8, 8)


def _structure_masks(n_seq, S, gen):
    masks = [('none', None)]
    if S > 1:
        rnd = torch.rand(n_seq, S, generator=gen, device='cuda') < 0.5
        rnd[:, S - 1] |= ~rnd.any(1)
        key0 = torch.ones(n_seq, S, dtype=torch.bool, device='cuda'); key0[:, 0] = False
        last = torch.zeros(n_seq, S, dtype=torch.bool, device='cuda'); last[:, S - 1] = True
        masks += [('random', rnd), ('key0', key0), ('last', last)]
    return masks


@pytest.mark.parametrize('heads', [1, 8])
@pytest.mark.parametrize('S', [1, 2, 5, 8])
def test_small_attn_structure_exact(ops, S, heads):
    """All keys of a sequence identical: every score of a row is the same number, exp(0) = 1 exactly, so probs = fp32(1 / n_valid) on the
    valid keys and +0 on masked keys and for j >= S (rows i >= S are not written), and out is the dropout-weighted mean of the valid v
    rows: EQUAL to fp64 where n_valid is a power of two (the multipliers are 0 and 2), else within the two products and the 8-term chain
    (10u sum|p m v|) of the reference built from fp32(1 / n_valid)."""
    d = heads * 64
    for n_seq in (1, 3, 9):
        items = n_seq * heads
        gen = torch.Generator(device='cuda').manual_seed(100 * S + 10 * heads + n_seq)
        q64 = exact_ints((n_seq * S, d), -4, 4, -2, gen)
        k64 = exact_ints((n_seq, 1, d), -4, 4, -2, gen).expand(n_seq, S, d).reshape(n_seq * S, d)
        v64 = exact_ints((n_seq * S, d), -4, 4, -2, gen)
        qkv64 = torch.cat([q64, k64, v64], 1)
        drop_rnd = (torch.rand(items, 8, 8, generator=gen, device='cuda') < 0.6).float() * 2.0
        drop_row = drop_rnd.clone(); drop_row[0, 0, :] = 0.0                                  # a row whose kept keys are all dropped
        for mname, km in _structure_masks(n_seq, S, gen):
            valid = torch.ones(n_seq, S, dtype=torch.bool, device='cuda') if km is None else km
            nv = valid.sum(1)
            p32 = (torch.tensor(1.0, device='cuda') / nv.float())                             # fp32 division, correctly rounded
            P = (p32.double()[:, None] * valid.double())[:, None, None, :].expand(n_seq, heads, S, S)
            vh = v64.reshape(n_seq, S, heads, 64).permute(0, 2, 1, 3)
            for dname, drop in (('none', None), ('random', drop_rnd), ('row', drop_row)):
                what = (n_seq, mname, dname)
                m = torch.ones(n_seq, heads, S, S, device='cuda', dtype=torch.float64) if drop is None else \
                    drop.double()[:, :S, :S].reshape(n_seq, heads, S, S)
                want = ((P * m) @ vh).permute(0, 2, 1, 3).reshape(n_seq * S, d)
                mag = ((P * m) @ vh.abs()).permute(0, 2, 1, 3).reshape(n_seq * S, d)
                bits = []
                for rep in range(2):
                    qkv, obuf, out, pbuf, probs = _attn_buffers(qkv64, n_seq, S, heads)
                    ops.small_attn_fwd(qkv, None if km is None else km.to(torch.uint8), out, probs, n_seq, S, heads, drop=drop)
                    torch.cuda.synchronize()
                    bits.append((obuf.view(torch.int32).clone(), pbuf.view(torch.int32).clone()))
                assert torch.equal(probs[:, :S, :S].double(), P.reshape(items, S, S)), what
                assert bool((probs[:, :S, S:].view(torch.int32) == 0).all()), what           # j >= S: +0
                assert bool((probs[:, :S, :S][~valid[:, None, None, :].expand(n_seq, heads, S, S).reshape(items, S, S)].view(torch.int32) == 0).all()), what
                assert bool(is_sentinel(probs[:, S:, :]).all() and is_sentinel(pbuf[items:]).all()), what
                pow2 = ((nv & (nv - 1)) == 0).repeat_interleave(S)
                got = out.double()
                assert torch.equal(got[pow2], want[pow2]), what
                R.assert_within(got, want, 10 * U * mag, str(what))
                if dname == 'row':
                    assert float(got[0, :64].abs().max()) == 0.0, what
                assert untouched(obuf, n_seq * S, d, 4), what
                assert torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1]), what


@pytest.mark.parametrize('heads', [1, 8])
@pytest.mark.parametrize('S', [1, 2, 5, 8])
def test_small_attn_numerics(ops, S, heads):
    """Random q / k with scores spread to +-30 against fp64 softmax attention, forward (out, probs) and backward (dqkv from the kernel's
    own saved probs), every element inside its derived allowance; the exponential's share is rowops_refs.ATTN_EXPF_REL = 4 x the fp32
    oracle's worst normalised error, 4 x 2.5e-6 = 1.0e-5 of the condition term (test_rowops_refs_cpu.py measures 2.464e-6)."""
    d = heads * 64
    for n_seq in (1, 3, 9):
        items = n_seq * heads
        qkv_c, dout_c, km_c = R.attn_inputs(n_seq, S, heads, R.attn_seed(n_seq, S, heads))
        qkv64, dout64, km = qkv_c.cuda(), dout_c.cuda(), km_c.cuda()
        gen = torch.Generator(device='cuda').manual_seed(S + heads)
        keep = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(0.9, dtype=torch.float32)
        drop = (torch.rand(items, 8, 8, generator=gen, device='cuda') < 0.9).float() * float(keep)
        for mask, dr in ((None, None), (km, None), (km, drop)):
            what = (n_seq, mask is not None, dr is not None)
            dr64 = None if dr is None else dr.double()[:, :S, :S]
            o_ref, p_ref, t = R.attn_fwd_ref(qkv64, mask, dr64, n_seq, S, heads)
            allow_o, allow_p, _ = R.attn_fwd_allow(t, R.ATTN_EXPF_REL)
            bits = []
            for rep in range(2):
                qkv, obuf, out, pbuf, probs = _attn_buffers(qkv64, n_seq, S, heads)
                dout = padded32(dout64, 8, 4)
                assert dout.stride(0) == out.stride(0)
                gbuf, dqkv = guarded(n_seq * S, 3 * d, 4)
                ops.small_attn_fwd(qkv, None if mask is None else mask.to(torch.uint8), out, probs, n_seq, S, heads, drop=dr)
                ops.small_attn_bwd(qkv, probs, dout, dqkv, n_seq, S, heads, drop=dr)
                torch.cuda.synchronize()
                bits.append((obuf.view(torch.int32).clone(), pbuf.view(torch.int32).clone(), gbuf.view(torch.int32).clone()))
            R.assert_within(probs[:, :S, :S], p_ref, allow_p, f'{what} probs')
            assert bool((probs[:, :S, S:].view(torch.int32) == 0).all()) and bool(is_sentinel(probs[:, S:, :]).all() and is_sentinel(pbuf[items:]).all())
            R.assert_within(out, o_ref, allow_o, f'{what} out')
            g_ref, g_allow = R.attn_bwd_ref(qkv64, probs[:, :S, :S].double(), dr64, dout64, n_seq, S, heads)
            R.assert_within(dqkv, g_ref, g_allow, f'{what} dqkv')
            assert untouched(obuf, n_seq * S, d, 4) and untouched(gbuf, n_seq * S, 3 * d, 4), what
            assert all(torch.equal(a, b) for a, b in zip(*bits)), what


@pytest.mark.parametrize('heads', [1, 8])
def test_small_attn_fully_masked_sequence_is_nan(ops, heads):
    """A sequence without a valid key: softmax over nothing.  torch / fp64 give NaN in exactly its rows; so must the kernel, and the
    other sequences served by the same workgroup (heads = 1: all three items share one) must be what they are without it."""
    n_seq, S, d = 3, 5, heads * 64
    qkv_c, _, km_c = R.attn_inputs(n_seq, S, heads, 7)
    km_c[1] = False
    qkv64, km = qkv_c.cuda(), km_c.cuda()
    o_ref, p_ref, t = R.attn_fwd_ref(qkv64, km, None, n_seq, S, heads)
    allow_o, allow_p, _ = R.attn_fwd_allow(t, R.ATTN_EXPF_REL)
    qkv, obuf, out, pbuf, probs = _attn_buffers(qkv64, n_seq, S, heads)
    ops.small_attn_fwd(qkv, km.to(torch.uint8), out, probs, n_seq, S, heads)
    torch.cuda.synchronize()
    nan = torch.isnan(out)
    assert torch.equal(nan, torch.isnan(o_ref)) and bool(nan[S:2 * S].all()) and int(nan.sum()) == S * d
    live = torch.ones(n_seq * S, dtype=torch.bool, device='cuda'); live[S:2 * S] = False
    R.assert_within(out[live], o_ref[live], allow_o[live], 'other sequences')
    pl = torch.ones(n_seq * heads, dtype=torch.bool, device='cuda'); pl[heads:2 * heads] = False
    R.assert_within(probs[pl][:, :S, :S], p_ref[pl], allow_p[pl], 'other probs')
    assert bool(torch.isnan(probs[~pl][:, :S, :S]).all())
    assert untouched(obuf, n_seq * S, d, 4) and bool(is_sentinel(probs[:, S:, :]).all() and is_sentinel(pbuf[n_seq * heads:]).all())


def test_small_attn_refusals(ops):
    from prcv2025reid_amd._lib import ReidHipError
    n_seq, S, heads, d = 2, 5, 1, 64
    rows = n_seq * S
    qkv = torch.zeros(rows, 3 * d, device='cuda')
    narrow = torch.as_strided(qkv, (rows, 3 * d), (3 * d - 4, 1))
    obuf, out = guarded(rows, d)
    gbuf, dqkv = guarded(rows, 3 * d)
    pbuf = sentinel_buffer(n_seq * heads + GUARD, 64, torch.float32)
    probs = pbuf[:n_seq * heads].view(-1, 8, 8)
    zp = torch.zeros(n_seq * heads, 8, 8, device='cuda')
    dout = torch.zeros(rows, d, device='cuda')
    for S_bad in (0, 9):
        with pytest.raises(ReidHipError):
            ops.small_attn_fwd(qkv, None, out, probs, n_seq, S_bad, heads)
        with pytest.raises(ReidHipError):
            ops.small_attn_bwd(qkv, zp, dout, dqkv, n_seq, S_bad, heads)
    with pytest.raises(ReidHipError):
        ops.small_attn_fwd(narrow, None, out, probs, n_seq, S, heads)                          # ld < 3 heads 64
    with pytest.raises(ReidHipError):
        ops.small_attn_fwd(qkv, None, torch.as_strided(out, (rows, d), (d - 4, 1)), probs, n_seq, S, heads)       # ldo
    with pytest.raises(ReidHipError):
        ops.small_attn_bwd(narrow, zp, dout, dqkv, n_seq, S, heads)                            # ld
    with pytest.raises(ReidHipError):
        ops.small_attn_bwd(qkv, zp, torch.as_strided(dout, (rows, d), (d - 4, 1)), dqkv, n_seq, S, heads)         # ldo
    with pytest.raises(ReidHipError):
        ops.small_attn_bwd(qkv, zp, dout, torch.as_strided(dqkv, (rows, 3 * d), (3 * d - 4, 1)), n_seq, S, heads)  # lddqkv
    torch.cuda.synchronize()
    assert bool(is_sentinel(obuf).all() and is_sentinel(gbuf).all() and is_sentinel(pbuf).all())


# ---------------------------------------------------------------------------------------------------------- reid_masked_mean
@pytest.mark.parametrize('M', [1, 3, 4, 5, 323])
def test_masked_mean_exact(ops, M):
    """Exact operands and 0/1 masks: the sums are exact, so forward = fp32(sum / cnt) and backward = fp32(dout / cnt) on kept rows,
    each within the one rounding of the division (u |value|) and EQUAL where cnt is a power of two; an all-zero mask row gives 0
    forward and backward; the backward writes all M rows, masked ones as +0."""
    for B in (1, 3):
        for D in (4, 64, 200, 512):
            gen = torch.Generator(device='cuda').manual_seed(M * 1000 + B * 10 + D)
            x64 = exact_ints((B, M, D), -8, 8, -2, gen)
            mask = (torch.rand(B, M, generator=gen, device='cuda') < 0.6).double()
            mask[0] = 1.0                                                                     # cnt = M (a power of two for M = 1, 4)
            if B == 3:
                mask[1] = 0.0                                                                 # no valid row at all
            assert_bit_budget(x64.abs().sum(1), 2.0 ** -2)
            s, cnt = R.masked_mean_ref(x64, mask)
            want = s / cnt[:, None]
            ci = cnt.long()
            pow2 = (ci & (ci - 1)) == 0
            x, mk = x64.float().contiguous(), mask.float().contiguous()
            bits = []
            for rep in range(2):
                buf, out = flat_guarded(B * D)
                ops.masked_mean(x, mk, out, B, M, D)
                torch.cuda.synchronize()
                bits.append(buf.view(torch.int32).clone())
            got = out.view(B, D).double()
            R.assert_within(got, want, U * want.abs(), f'fwd {(B, M, D)}')
            assert torch.equal(got[pow2], want[pow2]), (B, M, D)
            assert bool(is_sentinel(buf[B * D:]).all()) and torch.equal(bits[0], bits[1]), (B, M, D)
            g64 = exact_ints((B, D), -8, 8, -2, gen)
            g64 = torch.where(g64 == 0, torch.full_like(g64, -0.25), g64)                     # non-zero, both signs: 0 * negative is -0
            wantb = mask[:, :, None] * (g64 / cnt[:, None])[:, None, :]
            g = g64.float().contiguous()
            bits = []
            for rep in range(2):
                buf, dx = flat_guarded(B * M * D)
                ops.masked_mean(g, mk, dx, B, M, D, backward=True)
                torch.cuda.synchronize()
                bits.append(buf.view(torch.int32).clone())
            gotb = dx.view(B, M, D)
            R.assert_within(gotb, wantb, U * wantb.abs(), f'bwd {(B, M, D)}')
            assert torch.equal(gotb.double()[pow2], wantb[pow2]), (B, M, D)
            assert bool((gotb[mask == 0].view(torch.int32) == 0).all()), (B, M, D)            # +0 bit pattern
            if B == 3:
                assert float(got[1].abs().max()) == 0.0 and float(gotb[1].abs().max()) == 0.0
            assert bool(is_sentinel(buf[B * M * D:]).all()) and torch.equal(bits[0], bits[1]), (B, M, D)


def test_masked_mean_and_bnneck_bwd_refusals(ops):
    from prcv2025reid_amd._lib import ReidHipError
    B = 65536
    x = torch.zeros(B, 1, 4, device='cuda'); mk = torch.ones(B, 1, device='cuda')
    buf, out = flat_guarded(B * 4)
    with pytest.raises(ReidHipError):
        ops.masked_mean(x, mk, out, B, 1, 4)
    with pytest.raises(ReidHipError):
        ops.masked_mean(x, mk, out, 4, 0, 4)
    torch.cuda.synchronize()
    assert bool(is_sentinel(buf).all())
    # reid_bnneck_bwd_p1 reads dy and x sixteen bytes at a time: leading dimensions that are no multiple of 4, or below D
    rows, D = 8, 64
    z = torch.zeros(rows, D + 8, device='cuda')
    vec = torch.ones(D, device='cuda'); rn = torch.ones(rows, device='cuda')
    dz = sentinel_buffer(rows, D, torch.float32); s1 = sentinel_buffer(1, D, torch.float32)[0]; s2 = sentinel_buffer(1, D, torch.float32)[0]
    good = z[:, :D]
    for dy, xx in ((torch.as_strided(z, (rows, D), (D + 2, 1)), good), (good, torch.as_strided(z, (rows, D), (D + 2, 1))),
                   (torch.as_strided(z, (rows, D), (D - 4, 1)), good), (good, torch.as_strided(z, (rows, D), (D - 4, 1)))):
        with pytest.raises(ReidHipError):
            ops.bnneck_bwd_p1(dy, xx, vec, vec, vec, vec, rn, dz, s1, s2)
    torch.cuda.synchronize()
    assert bool(is_sentinel(dz).all() and is_sentinel(s1).all() and is_sentinel(s2).all())
