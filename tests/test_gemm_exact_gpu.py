"""GPU: the GEMM family element-wise against fp64 on EXACT operands -- reid_mer_gemm on every dispatch path x epilogue, reid_gemm_tn,
reid_lora_bwd_fused, reid_lora_da_fused and reid_merge_lora_table.

Operands are small integers times powers of two (helpers.exact_ints) with a checked bit budget (helpers.assert_bit_budget): every
product and partial sum is then exact in fp32, so the kernels' accumulators equal the fp64 reference in any summation order and the
only tolerance left is the one of the transcendental epilogues.  fp32 outputs must equal the reference; 16-bit outputs must equal its
round-to-nearest-even into the output format (helpers.round16), ties included.  Every output buffer is filled with a sentinel NaN
pattern first: padding columns, 32 guard rows and rows a call does not own must keep it bit for bit, and a second call gives the same
bits.  Scale variants (x 2^9, x 2^-20) move IEEE-half outputs across 65504 (saturation) and into half's subnormal range."""
import pytest
import torch

from gemm_cases import CASES, S, case_plan, plan_labels
from helpers import (U, assert_bit_budget, check_bounded, count_ties16, exact_ints, f_dgelu, f_dquick, f_gelu, f_quick, is_sentinel, quantum16,
                     round16, sentinel_buffer)

pytestmark = pytest.mark.gpu

GUARD = 32          # guard rows after the last row of every output buffer


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


def set_knob(name, value):
    from prcv2025reid_amd import _lib
    _lib.check(_lib.lib().reid_set_knob(name, value))


def padded16(vals, ld, fmt):
    """Exact 16-bit device operand with the values of float64 `vals` [rows, cols] in a [rows, ld] sentinel buffer; returns the view."""
    rows, cols = vals.shape
    buf = sentinel_buffer(rows, ld, T16(), fmt)
    v = vals.to(T16())
    assert torch.equal(v.double(), vals), 'operand not representable in the 16-bit format'
    buf[:, :cols] = v
    return buf[:, :cols]


def padded32(vals, ld):
    rows, cols = vals.shape
    buf = sentinel_buffer(rows, ld, torch.float32)
    v = vals.float()
    assert torch.equal(v.double(), vals)
    buf[:, :cols] = v
    return buf[:, :cols]


# The derived error budgets of the transcendental epilogues (f_gelu, f_dgelu, f_quick, f_dquick, check_bounded) live in helpers.py:
# reid_sgemm and reid_eltwise_f32 call the same gauss_cdf_pdf / quick_gelu_f and are held to the same budgets.


REQUIRED_LABELS = {'skinny64x32', 'skinny256x32', 'skinny64x64', 'skinny256x64', 'skinny128x32', 'main128_lean', 'main128_generic',
                   'pp256', 'pp224', 'pps_ragged', 'pps_multi'}

TRANSCENDENTAL = ('gelu', 'gelu_dsave', 'dgelu', 'quick_gelu', 'dquick_gelu')
# Operands: A integers in [-a, a], B integers in [-a, a] times 2^-8 (a = 64: outputs of a few hundred with 15-16 significant bits, so
# that bf16 and half both round, ties included; 32 / 16 where row_scale / aux spend part of the 24-bit budget).  Scale variants
# (exponent of A, exponent of B on top of its 2^-8): x1, x2^9 (half outputs beyond 65504: saturation), x2^-20 (half outputs in the
# subnormal range, rounded at 2^-24 from a 2^-28 grid; the operands stay normal: |A| >= 2^-14, |B| >= 2^-14).
SCALES = {'x1': (0, 0), 'up': (5, 4), 'down': (-14, -6)}

PARAMS = [pytest.param(c, s, id=f"{c['name']}-{s}") for c in CASES
          for s in (('x1',) if c.get('act') in TRANSCENDENTAL else ('x1', 'up', 'down'))]

STATS = {}          # per (flavor, case): ties, clamped, subnormal counts and worst err / bound -- printed per test


def test_dispatch_table_reaches_every_path():
    """The case table, planned by the library itself (reid_mer_gemm_plan) for THIS device's CU count, reaches every kernel / tile."""
    from prcv2025reid_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reached = set()
    for c in CASES:
        labels = plan_labels(c, case_plan(ops, c, 0))
        print(f"{c['name']:28s} -> {sorted(labels)}")
        reached |= labels
    missing = REQUIRED_LABELS - reached
    assert not missing, f'no case reaches {sorted(missing)} on {cus} CUs'
    print('reached:', sorted(reached))


def _build(c, scale, fmt, gen):
    """Operands (device), fp64 reference pieces and the call's keyword arguments for case `c`."""
    sa, sb = SCALES[scale]
    e = sa + sb
    M, N, K = c['M'], c['N'], c['K']
    act = c.get('act', 'none')
    a = 16 if act in TRANSCENDENTAL or act == 'mul_aux' else (32 if c.get('row_scale') else 64)
    A64 = exact_ints((M, K), -a, a, sa, gen)
    A = padded16(A64, c['lda'], fmt)
    if c.get('groups'):
        mus = [2, 0, 3, 1][:len(c['groups'])]
        Bst = exact_ints((4, N, K), -a, a, sb - 8, gen)
        Bbuf = sentinel_buffer(4 * N, K + 8, T16(), fmt).view(4, N, K + 8)
        Bbuf[:, :, :K] = Bst.to(T16())
        B = Bbuf[:, :, :K]
        ends = list(torch.tensor(c['groups']).cumsum(0).mul(S).tolist())
        acc = torch.empty(M, N, device='cuda', dtype=torch.float64)
        absacc = torch.empty_like(acc)
        lo = 0
        for hi, mu in zip(ends, mus):
            acc[lo:hi] = A64[lo:hi] @ Bst[mu].t()
            absacc[lo:hi] = A64[lo:hi].abs() @ Bst[mu].abs().t()
            lo = hi
        kw = dict(row_groups=(ends, mus))
    else:
        B64 = exact_ints((N, K), -a, a, sb - 8, gen)
        B = padded16(B64, K + 8, fmt)
        acc = A64 @ B64.t()
        absacc = A64.abs() @ B64.abs().t()
        kw = {}
    q = 2.0 ** (e - 8)                                    # quantum of every product and of bias / R
    if c.get('K2'):
        K2, k2n = c['K2'], c['k2_group_n']
        G = N // k2n
        T64 = exact_ints((M, G * K2), -a, a, sa, gen)
        B264 = exact_ints((N, K2), -a, a, sb - 8, gen)
        kw.update(A2=padded16(T64, G * K2 + 8, fmt), B2=padded16(B264, K2 + 8, fmt), K2=K2, k2_group_n=k2n)
        for g in range(G):
            cols = slice(g * k2n, (g + 1) * k2n)
            acc[:, cols] += T64[:, g * K2:(g + 1) * K2] @ B264[cols].t()
            absacc[:, cols] += T64[:, g * K2:(g + 1) * K2].abs() @ B264[cols].abs().t()
    if c.get('bias'):
        hi = 25600 if act in TRANSCENDENTAL else 1024     # +-100 / +-4: the activations see x down to about -100
        bias64 = exact_ints((N,), -hi, hi, e - 8, gen)
        kw['bias'] = bias64.float()
        acc += bias64
        absacc += bias64.abs()
    rows = torch.arange(M, device='cuda')
    if c.get('row_scale'):
        n_img = (M + S - 1) // S
        rs = torch.tensor([0.0, 1.25, 2.0], device='cuda', dtype=torch.float64)[torch.randint(0, 3, (n_img,), generator=gen, device='cuda')]
        kw.update(row_scale=rs.float(), rows_per_img=S)
        acc *= rs[rows // S].view(-1, 1)
        absacc *= 2.0
        q /= 4.0                                          # 1.25 = 5 / 4
    if c.get('R'):
        Rrows = S if c.get('patch') else M
        R64 = exact_ints((Rrows, N), -2 ** 14, 2 ** 14, e - 8, gen)
        if c.get('patch'):
            Rbuf = padded32(R64, c['ldr'])                 # the position table; row 0 (the CLS position) is not added here
            R = Rbuf[1:]
            kw.update(R=R, r_period=S - 1, c_group=S - 1, c_group_stride=S, c_row_off=1)
            Rm = R64[1:][rows % (S - 1)]
        else:
            R = padded32(R64, c['ldr'])
            kw['R'] = R
            Rm = R64
        acc += Rm
        absacc += Rm.abs()
    pre = acc
    aux64 = None
    if act in ('dgelu', 'dquick_gelu'):
        aux64 = round16(torch.empty(M, N, device='cuda', dtype=torch.float64).uniform_(-100.0, 100.0, generator=gen), fmt)
    elif act == 'mul_aux':
        aux64 = exact_ints((M, N), -8, 8, -1, gen)
        q /= 2.0
        absacc = absacc * 4.0
    elif act == 'drelu':
        aux64 = exact_ints((M, N), -4, 4, 0, gen)
    if aux64 is not None:
        kw.update(aux=padded16(aux64, c['ldaux'], fmt), act=act)
    elif act != 'none':
        kw['act'] = act
    if c.get('mask_r'):
        n_img = (M + S - 1) // S
        mods = torch.randint(0, 4, (n_img,), generator=gen, device='cuda').to(torch.int32)
        kw.update(img_mod=mods, mask_r=c['mask_r'], mask_period=c['mask_period'], rows_per_img=S)
        keep = ((torch.arange(N, device='cuda') % c['mask_period']) // c['mask_r']).view(1, -1) == mods.long()[rows // S].view(-1, 1)
    else:
        keep = None
    if c.get('alpha', 1.0) != 1.0:
        kw['alpha'] = c['alpha']
    assert_bit_budget(absacc, q)
    return A, B, kw, pre, aux64, keep


def _crow(c, M):
    """Output row of each GEMM row (patch rows land behind each image's CLS slot)."""
    m = torch.arange(M, device='cuda')
    if c.get('patch'):
        return (m // (S - 1)) * S + m % (S - 1) + 1, (M // (S - 1)) * S
    return m, M


@pytest.mark.parametrize('case,scale', PARAMS)
def test_mer_gemm_exact(ops, case, scale):
    c = case
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(sum(map(ord, c['name'] + scale)))
    plan = case_plan(ops, c, 0)
    labels = plan_labels(c, plan)
    A, B, kw, pre, aux64, keep = _build(c, scale, fmt, gen)
    M, N = c['M'], c['N']
    act = c.get('act', 'none')
    out = c.get('out', 't16')
    cdt = torch.float32 if out == 'f32' else (torch.float16 if out == 'f16' else T16())
    cfmt = 'f32' if out == 'f32' else ('f16' if out == 'f16' else fmt)
    crow, crows = _crow(c, M)
    # the lean GELU epilogues evaluate Phi with gelu_both_x2, the generic one and every dgelu with gauss_cdf_pdf
    x2 = act in ('gelu', 'gelu_dsave') and plan.epilogue != 0          # (0 = REID_EPI_GENERIC)

    def run():
        C = sentinel_buffer(crows + GUARD, c['ldc'], cdt, cfmt)
        C2 = sentinel_buffer(M + GUARD, c['ldc2'], T16(), fmt) if c.get('C2') else None
        if C2 is not None:
            kw['C2'] = C2[:M, :N]
        set_knob(b'GEMM_TILE', c.get('tile', 0) or -1)
        try:
            ops.gemm(A, B, C[:crows, :N], **kw)
        finally:
            set_knob(b'GEMM_TILE', -1)
        torch.cuda.synchronize()
        return C, C2

    C, C2 = run()
    # ownership: padding columns, guard rows and skipped rows keep the sentinel
    owned = torch.zeros(crows + GUARD, c['ldc'], dtype=torch.bool, device='cuda')
    owned[crow, :N] = True
    stray = ~is_sentinel(C, cfmt) & ~owned
    assert not bool(stray.any()), (f'{int(stray.sum())} stores outside the rows / columns the call owns: rows '
                                   f'{stray.any(1).nonzero().flatten()[:8].tolist()}, columns {stray.any(0).nonzero().flatten()[:8].tolist()}')
    if C2 is not None:
        owned2 = torch.zeros(M + GUARD, c['ldc2'], dtype=torch.bool, device='cuda')
        owned2[:M, :N] = True
        assert bool(is_sentinel(C2, fmt)[~owned2].all()), 'a C2 store outside [M, N]'
    got = C[crow, :N]
    st = dict(labels=sorted(labels), ties=0, clamped=0, subnormal=0, exact16=0, ratio=None)

    def exact16(o, ref, f):
        want = round16(ref, f)
        bad = o.double() != want
        assert not bool(bad.any()), (f'{int(bad.sum())} elements differ, e.g. (got, round16(ref), ref): '
                                     f'{list(zip(o.double()[bad][:4].tolist(), want[bad][:4].tolist(), ref[bad][:4].tolist()))}')
        st['exact16'] += 1
        st['ties'] += count_ties16(ref, f)
        if f == 'f16':
            st['clamped'] += int((ref.abs() >= 65520.0).sum())
            st['subnormal'] += int(((ref != 0) & (ref.abs() < 2.0 ** -14)).sum())

    # the value that reaches C
    if act in TRANSCENDENTAL:
        if act == 'gelu' or act == 'gelu_dsave':
            f, err = f_gelu(pre, x2)
        elif act == 'quick_gelu':
            f, err = f_quick(pre)
        else:
            d, derr = (f_dgelu(aux64, False) if act == 'dgelu' else f_dquick(aux64))
            f, err = pre * d, pre.abs() * derr + U * (pre * d).abs()
        st['ratio'] = check_bounded(got, f, err, cfmt)
    else:
        ref = pre
        if act == 'relu':
            ref = ref.clamp_min(0.0)
        elif act == 'drelu':
            ref = ref * (aux64 > 0)
        elif act == 'mul_aux':
            ref = ref * aux64
        if keep is not None:
            ref = ref * keep
        ref = ref * c.get('alpha', 1.0)
        if out == 'f32':
            assert torch.equal(got.double(), ref), f'max |d| = {float((got.double() - ref).abs().max()):.3g}'
        else:
            exact16(got, ref, cfmt)
        if keep is not None:
            assert bool((got[~keep].view(torch.int16) == 0).all()), 'a masked LoRA column is not +0.0'
    if C2 is not None:
        g2 = C2[:M, :N]
        if act == 'gelu_dsave':
            d, derr = f_dgelu(pre, x2)
            r2 = check_bounded(g2, d, derr, fmt)
            st['ratio_C2'] = r2
        else:
            exact16(g2, pre, fmt)                          # the pre-activation
    # the same call again: the same bits everywhere (sentinels included)
    C_again, C2_again = run()
    assert torch.equal(C.view(torch.int32 if cdt == torch.float32 else torch.int16),
                       C_again.view(torch.int32 if cdt == torch.float32 else torch.int16))
    if C2 is not None:
        assert torch.equal(C2.view(torch.int16), C2_again.view(torch.int16))
    if scale == 'x1' and st['exact16']:
        assert st['ties'] > 0, 'no exact tie among the 16-bit outputs: round-to-nearest-even untested'
    if scale == 'up' and cfmt == 'f16':
        assert st['clamped'] > 0, 'no output crossed 65504'
    if scale == 'down' and cfmt == 'f16':
        assert st['subnormal'] > 0, 'no output in the subnormal range of IEEE half'
    STATS[(fmt, c['name'], scale)] = st
    print(f"[{fmt}] {c['name']}-{scale}: {st}")


def test_mer_gemm_contract_refusals(ops):
    """K must be a multiple of 64 (a K = 96 call is refused, as include/reid_hip.h says); alpha = 0 means 1."""
    from prcv2025reid_amd import _lib
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(3)
    A64 = exact_ints((200, 96), -4, 4, 0, gen); B64 = exact_ints((256, 96), -4, 4, -4, gen)
    C = torch.empty(200, 256, device='cuda')
    with pytest.raises(_lib.ReidHipError):
        ops.gemm(A64.to(T16()), B64.to(T16()), C)
    A = padded16(exact_ints((200, 128), -4, 4, 0, gen), 136, fmt); B = padded16(exact_ints((256, 128), -4, 4, -4, gen), 136, fmt)
    ops.gemm(A, B, C, alpha=0.0)
    assert torch.equal(C.double(), A.double() @ B.double().t())


# ---- reid_gemm_tn ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,P,Q', [(1000, 8, 40), (777, 72, 200), (4099, 40, 768), (130, 200, 72), (5000, 96, 8), (63, 768, 32),
                                   (2100, 200, 384), (1000, 768, 32)])
def test_gemm_tn_exact(ops, M, P, Q):
    """C = beta C + alpha X^T Y: exact against fp64 for P, Q multiples of 8 that are not multiples of any tile, M not a multiple of
    the 64-row slab step, beta = 0 over a sentinel-filled C, beta = 1 and 0.5 accumulation; ldc > Q padding and guard rows untouched;
    a repeated call gives the same bits (fp32 atomics in any order are exact here)."""
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(M * 7 + P * 3 + Q)
    X64 = exact_ints((M, P), -4, 4, 0, gen); Y64 = exact_ints((M, Q), -4, 4, -4, gen)
    X = padded16(X64, P + 8, fmt); Y = padded16(Y64, Q + 8, fmt)
    ref = X64.t() @ Y64
    assert_bit_budget(X64.abs().t() @ Y64.abs() * 3.0, 2.0 ** -6)
    ldc = Q + 8

    def fresh():
        return sentinel_buffer(P + GUARD, ldc, torch.float32)
    owned = torch.zeros(P + GUARD, ldc, dtype=torch.bool, device='cuda'); owned[:P, :Q] = True
    C = fresh()
    ops.gemm_tn(X, Y, C[:P, :Q], alpha=0.5, beta=0.0)
    torch.cuda.synchronize()
    assert bool(is_sentinel(C)[~owned].all())
    assert torch.equal(C[:P, :Q].double(), 0.5 * ref)
    C1 = fresh()
    ops.gemm_tn(X, Y, C1[:P, :Q], alpha=0.5, beta=0.0)
    assert torch.equal(C.view(torch.int32), C1.view(torch.int32))
    ops.gemm_tn(X, Y, C[:P, :Q], alpha=2.0, beta=1.0)
    assert torch.equal(C[:P, :Q].double(), 2.5 * ref)
    ops.gemm_tn(X, Y, C[:P, :Q], alpha=0.25, beta=0.5)
    assert torch.equal(C[:P, :Q].double(), 1.5 * ref)
    assert bool(is_sentinel(C)[~owned].all())


# ---- fused LoRA kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_img,rpi,r,lddy_extra', [(24, 197, 8, 0), (7, 197, 4, 1536), (256, 1, 8, 0), (3, 50, 8, 768), (100, 197, 8, 0),
                                                    (5, 32, 2, 0), (4, 33, 8, 0)])
def test_lora_bwd_fused_exact(ops, n_img, rpi, r, lddy_extra):
    """U = round16(mask(dY B) * scale) and dB = dB0 + dY^T T exactly, both kernels behind the entry point (LORA_IMPL default with a
    masked T, 1 = the slab kernel with any T); padding and guard rows of U and dB keep their sentinels."""
    fmt = flavor()
    M, N, Rp = n_img * rpi, 768, 32
    gen = torch.Generator(device='cuda').manual_seed(M + r + lddy_extra)
    dY64 = exact_ints((M, N + lddy_extra), -4, 4, 0, gen)
    dYw = padded16(dY64, N + lddy_extra + 8, fmt)
    o = lddy_extra // 2
    dY = dYw[:, o:o + N]; dY64 = dY64[:, o:o + N]
    mods = torch.randint(0, 4, (n_img,), generator=gen, device='cuda').to(torch.int32)
    keep = (torch.arange(Rp, device='cuda').view(1, -1) // r) == mods.long().repeat_interleave(rpi).view(-1, 1)
    T_any64 = exact_ints((M, Rp), -4, 4, -2, gen)
    BT64 = exact_ints((Rp, N), -4, 4, -4, gen)
    BT = padded16(BT64, N + 8, fmt)
    scale = 32.0 / r
    dB064 = exact_ints((N, Rp), -1024, 1024, -4, gen)
    U64 = (dY64 @ BT64.t()) * scale * keep
    assert_bit_budget((dY64.abs() @ BT64.abs().t()) * scale, 2.0 ** -4)
    for impl, T64 in ((-1, T_any64 * keep), (1, T_any64), (1, T_any64 * keep)):
        Tm = padded16(T64, Rp + 8, fmt)
        dB_want = dB064 + dY64.t() @ T64
        assert_bit_budget(dB064.abs() + dY64.abs().t() @ T64.abs(), 2.0 ** -4)
        U = sentinel_buffer(M + GUARD, Rp + 8, T16(), fmt)
        dBb = sentinel_buffer(N + GUARD, Rp + 8, torch.float32)
        dBb[:N, :Rp] = dB064.float()
        set_knob(b'LORA_IMPL', impl)
        try:
            ops.lora_bwd_fused(dY, Tm, BT, U[:M, :Rp], dBb[:N, :Rp], mods, rpi, r, scale)
        finally:
            set_knob(b'LORA_IMPL', -1)
        assert torch.equal(U[:M, :Rp].double(), round16(U64, fmt)), impl
        assert bool((U[:M, :Rp][~keep].view(torch.int16) == 0).all()), impl          # other modalities' columns: +0.0
        assert torch.equal(dBb[:N, :Rp].double(), dB_want), impl
        assert bool(is_sentinel(U[:M, Rp:], fmt).all() and is_sentinel(U[M:], fmt).all()), impl
        assert bool(is_sentinel(dBb[:N, Rp:]).all() and is_sentinel(dBb[N:]).all()), impl


def test_lora_bwd_fused_column_blocks_exact(ops):
    """fc1's 3072-column cotangent as four 768-column launches through the fp32 scratch u_partial: exact U and dB, both kernels."""
    fmt = flavor()
    n_img, rpi, r, N, Rp = 5, 197, 8, 3072, 32
    M = n_img * rpi
    gen = torch.Generator(device='cuda').manual_seed(11)
    dY64 = exact_ints((M, N), -4, 4, 0, gen)
    dY = padded16(dY64, N + 8, fmt)
    mods = torch.randint(0, 4, (n_img,), generator=gen, device='cuda').to(torch.int32)
    keep = (torch.arange(Rp, device='cuda').view(1, -1) // r) == mods.long().repeat_interleave(rpi).view(-1, 1)
    T64 = exact_ints((M, Rp), -4, 4, -2, gen) * keep
    Tm = padded16(T64, Rp + 8, fmt)
    BT64 = exact_ints((Rp, N), -4, 4, -4, gen)
    BT = padded16(BT64, N + 8, fmt)
    scale = 4.0
    U64 = (dY64 @ BT64.t()) * scale * keep
    assert_bit_budget((dY64.abs() @ BT64.abs().t()) * scale, 2.0 ** -4)
    for impl in (-1, 1):
        U = sentinel_buffer(M + GUARD, Rp + 8, T16(), fmt)
        dB = sentinel_buffer(N + GUARD, Rp + 8, torch.float32)
        dB[:N, :Rp] = 0.0
        scratch = torch.full((M, Rp), float('nan'), device='cuda')
        set_knob(b'LORA_IMPL', impl)
        try:
            ops.lora_bwd_fused(dY, Tm, BT, U[:M, :Rp], dB[:N, :Rp], mods, rpi, r, scale, u_partial=scratch)
        finally:
            set_knob(b'LORA_IMPL', -1)
        assert torch.equal(U[:M, :Rp].double(), round16(U64, fmt)), impl
        assert torch.equal(dB[:N, :Rp].double(), dY64.t() @ T64), impl
        assert bool(is_sentinel(U[:M, Rp:], fmt).all() and is_sentinel(U[M:], fmt).all() and is_sentinel(dB[:N, Rp:]).all()
                    and is_sentinel(dB[N:]).all()), impl


@pytest.mark.parametrize('n_img,rpi,r,K,G', [(24, 197, 8, 768, 1), (9, 197, 8, 3072, 1), (11, 197, 8, 768, 3), (3, 50, 4, 768, 3),
                                             (100, 197, 8, 768, 1), (5, 33, 2, 1536, 1)])
def test_lora_da_fused_exact(ops, n_img, rpi, r, K, G):
    """dA = dA0 + U^T X exactly; rows of adapters whose modality no image has keep dA0's bits; padding and guard rows untouched."""
    fmt = flavor()
    M, Rp = n_img * rpi, 32
    gen = torch.Generator(device='cuda').manual_seed(M + K + G)
    X64 = exact_ints((M, K), -4, 4, -4, gen)
    X = padded16(X64, K + 8, fmt)
    mods = torch.randint(0, 4, (n_img,), generator=gen, device='cuda').to(torch.int32)
    keep = ((torch.arange(G * Rp, device='cuda').view(1, -1) % Rp) // r) == mods.long().repeat_interleave(rpi).view(-1, 1)
    U64 = exact_ints((M, G * Rp), -4, 4, 0, gen) * keep
    U = padded16(U64, G * Rp + 8, fmt)
    dA064 = exact_ints((G * Rp, K), -1024, 1024, -4, gen)
    want = dA064 + U64.t() @ X64
    assert_bit_budget(dA064.abs() + U64.abs().t() @ X64.abs(), 2.0 ** -4)
    dA = sentinel_buffer(G * Rp + GUARD, K + 8, torch.float32)
    dA[:G * Rp, :K] = dA064.float()
    assert ops.lora_da_fused_ok(K, Rp, rpi, r, G)
    ops.lora_da_fused(X, U, dA[:G * Rp, :K], mods, rpi, r, n_groups=G)
    got = dA[:G * Rp, :K]
    assert torch.equal(got.double(), want)
    unused = ~keep.any(0)                                  # adapter rows no image's modality selects
    assert torch.equal(got[unused].view(torch.int32), dA064[unused].float().view(torch.int32))
    assert bool(is_sentinel(dA[:G * Rp, K:]).all() and is_sentinel(dA[G * Rp:]).all())


@pytest.mark.parametrize('r,G,N,K', [(8, 1, 768, 768), (4, 3, 384, 128), (16, 1, 256, 3072), (32, 1, 256, 768), (24, 3, 384, 128),
                                     (64, 1, 128, 128)])
def test_merge_lora_table_exact(ops, r, G, N, K):
    """W_eff[mu] = round16(W + s B_mu A_mu) exactly (one rounding of an exact fp32 value, ties included) and W_eff^T its exact transpose;
    the weff arena around both stacks keeps its sentinels."""
    fmt = flavor()
    gen = torch.Generator(device='cuda').manual_seed(r + G + N)
    nmod = 4
    Rp = ((nmod * r + 31) // 32) * 32
    W64 = exact_ints((N, K), -2 ** 14, 2 ** 14, -19, gen)              # |W| <= 2^-5, |s B A| <= r 2^-7: 15-18 significant bits
    W = W64.float()
    A64 = exact_ints((G * Rp, K), -64, 64, -8, gen); B64 = exact_ints((N, Rp), -64, 64, -8, gen)
    offA, offB = 32, 32 + G * Rp * K
    arena = torch.zeros(G * Rp * K + N * Rp + 64, device='cuda')
    arena[offA:offA + G * Rp * K] = A64.flatten().float(); arena[offB:offB + N * Rp] = B64.flatten().float()
    s = 2.0 ** -3
    total = 2 * nmod * N * K + 128
    weff = sentinel_buffer(1, total, T16(), fmt).view(-1)
    oE, oET = 64, 64 + nmod * N * K
    table = torch.tensor([[W.data_ptr(), offA, offB, oE, oET, N, K, G]], dtype=torch.int64, device='cuda')
    ops.merge_lora_table(table, 1, (N // 64) * (K // 64), arena, weff, Rp, r, nmod, s)
    E = weff[oE:oE + nmod * N * K].view(nmod, N, K); ET = weff[oET:oET + nmod * N * K].view(nmod, K, N)
    assert torch.equal(ET.view(torch.int16), E.transpose(1, 2).view(torch.int16))
    assert bool(is_sentinel(weff[:oE], fmt).all() and is_sentinel(weff[oET + nmod * N * K:], fmt).all())
    n_g = N // G
    ties = 0
    for mu in range(nmod):
        ref = W64.clone()
        absr = W64.abs()
        for gi in range(G):
            Bg = B64[gi * n_g:(gi + 1) * n_g, mu * r:(mu + 1) * r]; Ag = A64[gi * Rp + mu * r: gi * Rp + (mu + 1) * r]
            ref[gi * n_g:(gi + 1) * n_g] += s * (Bg @ Ag)
            absr[gi * n_g:(gi + 1) * n_g] += s * (Bg.abs() @ Ag.abs())
        assert_bit_budget(absr, 2.0 ** -19)
        assert torch.equal(E[mu].double(), round16(ref, fmt)), mu
        ties += count_ties16(ref, fmt)
    assert ties > 0
    print(f'[{fmt}] merge r={r} G={G} N={N} K={K}: ties={ties}')
