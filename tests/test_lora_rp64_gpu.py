"""GPU: the one-pass adapter-gradient kernels at Rp = 64 adapter columns (rank 16 x four modalities) element-wise against fp64 on EXACT
operands -- reid_lora_bwd_fused (N = 768 and the 3072-column form through u_partial [M, 64]) and reid_lora_da_fused -- and the domain
the two entry points accept.

Method of test_gemm_exact_gpu.py: operands are small integers times powers of two with a checked bit budget, so every partial sum is
exact in fp32 and the accumulators equal the fp64 reference in any order; fp32 outputs must EQUAL it, 16-bit outputs its
round-to-nearest-even.  Outputs live in sentinel buffers: padding columns and 32 guard rows keep the sentinel, a second call gives the
same bits.  img_mod = arange(n_img) % n_mod, so every 16-column window (and every position of a modality inside its window) occurs;
a further call with every image in the LAST modality shows that the columns / rows of the other modalities keep their non-zero start
bit for bit.  The shapes are the ones at which the step ring of the image kernels takes another path: one step (no counted wait), a
second step of one row, four steps (first buffer reuse), seven steps with a ragged last one (the ring wraps twice)."""
import pytest
import torch

from helpers import assert_bit_budget, exact_ints, is_sentinel, round16, sentinel_buffer

pytestmark = pytest.mark.gpu

GUARD = 32
RP = 64


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


def padded16(vals, ld, fmt):
    """Exact 16-bit device operand with the values of float64 `vals` [rows, cols] in a [rows, ld] sentinel buffer; returns the view."""
    rows, cols = vals.shape
    buf = sentinel_buffer(rows, ld, T16(), fmt)
    v = vals.to(T16())
    assert torch.equal(v.double(), vals), 'operand not representable in the 16-bit format'
    buf[:, :cols] = v
    return buf[:, :cols]


def keep_mask(mods, rpi, r, groups=1):
    """[M, groups * RP] bool: column c of a row is kept iff (c % RP) // r is the modality of the row's image."""
    cols = torch.arange(groups * RP, device='cuda').view(1, -1) % RP
    return (cols // r) == mods.long().repeat_interleave(rpi).view(-1, 1)


def mods_of(n_img, r):
    """(every modality in turn, every image in the last modality)"""
    n_mod = RP // r
    return ((torch.arange(n_img, device='cuda') % n_mod).to(torch.int32),
            torch.full((n_img,), n_mod - 1, device='cuda', dtype=torch.int32))


def _bwd_case(ops, n_img, rpi, r, N, lddy_extra, seed):
    fmt = flavor()
    M = n_img * rpi
    gen = torch.Generator(device='cuda').manual_seed(seed)
    dY64 = exact_ints((M, N + lddy_extra), -4, 4, 0, gen)
    dYw = padded16(dY64, N + lddy_extra + 8, fmt)
    o = lddy_extra // 2
    dY = dYw[:, o:o + N]; dY64 = dY64[:, o:o + N]
    T_any64 = exact_ints((M, RP), -4, 4, -2, gen)
    BT64 = exact_ints((RP, N), -4, 4, -4, gen)
    BT = padded16(BT64, N + 8, fmt)
    scale = 32.0 / r
    dB064 = exact_ints((N, RP), -1024, 1024, -4, gen)
    dB064 = torch.where(dB064 == 0, torch.full_like(dB064, 2.0 ** -4), dB064)          # a non-zero start everywhere
    assert_bit_budget((dY64.abs() @ BT64.abs().t()) * scale, 2.0 ** -4)
    assert_bit_budget(dB064.abs() + dY64.abs().t() @ T_any64.abs(), 2.0 ** -4)
    for which, mods in enumerate(mods_of(n_img, r)):
        keep = keep_mask(mods, rpi, r)
        T64 = T_any64 * keep
        Tm = padded16(T64, RP + 8, fmt)
        U64 = (dY64 @ BT64.t()) * scale * keep
        dB_want = dB064 + dY64.t() @ T64
        bits = []
        for rep in range(2):
            U = sentinel_buffer(M + GUARD, RP + 8, T16(), fmt)
            dBb = sentinel_buffer(N + GUARD, RP + 8, torch.float32)
            dBb[:N, :RP] = dB064.float()
            scratch = torch.full((M, RP), float('nan'), device='cuda') if N > 768 else None
            ops.lora_bwd_fused(dY, Tm, BT, U[:M, :RP], dBb[:N, :RP], mods, rpi, r, scale, u_partial=scratch)
            torch.cuda.synchronize()
            bits.append((U.view(torch.int16).clone(), dBb.view(torch.int32).clone()))
        assert torch.equal(U[:M, :RP].double(), round16(U64, fmt)), which
        assert bool((U[:M, :RP][~keep].view(torch.int16) == 0).all()), which            # the 64 - r other columns of every row: +0.0
        assert int((~keep).sum()) == M * (RP - r)
        assert torch.equal(dBb[:N, :RP].double(), dB_want), which
        if which == 1:                                                                   # other modalities' columns of dB: the start, bit for bit
            other = ~keep.any(0)
            assert int(other.sum()) == RP - r
            assert torch.equal(dBb[:N, :RP][:, other].view(torch.int32), dB064.float()[:, other].view(torch.int32))
        assert bool(is_sentinel(U[:M, RP:], fmt).all() and is_sentinel(U[M:], fmt).all()), which
        assert bool(is_sentinel(dBb[:N, RP:]).all() and is_sentinel(dBb[N:]).all()), which
        assert torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1]), which


@pytest.mark.parametrize('n_img,rpi,r,lddy_extra', [(5, 197, 16, 0), (4, 33, 16, 768), (4, 32, 16, 0), (6, 100, 16, 0), (8, 64, 8, 0),
                                                    (16, 32, 4, 0)])
def test_lora_bwd_fused_rp64_exact(ops, n_img, rpi, r, lddy_extra):
    """U = round16(mask(dY B) * scale) [M, 64] and dB = dB0 + dY^T T [768, 64] exactly from the image kernel's Rp = 64 form."""
    assert ops.lora_bwd_fused_ok(768, RP, rpi, r)
    _bwd_case(ops, n_img, rpi, r, 768, lddy_extra, n_img * rpi + r + lddy_extra)


def test_lora_bwd_fused_rp64_column_blocks_exact(ops):
    """fc1's 3072-column cotangent as four 768-column launches through the fp32 scratch u_partial [M, 64] (pre-filled with NaN)."""
    assert ops.lora_bwd_fused_ok(3072, RP, 197, 16)
    _bwd_case(ops, 5, 197, 16, 3072, 0, 11)


@pytest.mark.parametrize('n_img,rpi,r,K,G', [(5, 197, 16, 768, 1), (4, 33, 16, 3072, 1), (6, 100, 16, 768, 3), (8, 64, 8, 768, 3)])
def test_lora_da_fused_rp64_exact(ops, n_img, rpi, r, K, G):
    """dA = dA0 + U^T X exactly with 64 adapter columns per group; padding and guard rows untouched; rows of other modalities' adapters
    keep dA0's bits."""
    fmt = flavor()
    M = n_img * rpi
    gen = torch.Generator(device='cuda').manual_seed(M + K + G)
    X64 = exact_ints((M, K), -4, 4, -4, gen)
    X = padded16(X64, K + 8, fmt)
    U_any64 = exact_ints((M, G * RP), -4, 4, 0, gen)
    dA064 = exact_ints((G * RP, K), -1024, 1024, -4, gen)
    dA064 = torch.where(dA064 == 0, torch.full_like(dA064, 2.0 ** -4), dA064)
    assert_bit_budget(dA064.abs() + U_any64.abs().t() @ X64.abs(), 2.0 ** -4)
    assert ops.lora_da_fused_ok(K, RP, rpi, r, G)
    for which, mods in enumerate(mods_of(n_img, r)):
        keep = keep_mask(mods, rpi, r, G)
        U64 = U_any64 * keep
        U = padded16(U64, G * RP + 8, fmt)
        want = dA064 + U64.t() @ X64
        bits = []
        for rep in range(2):
            dA = sentinel_buffer(G * RP + GUARD, K + 8, torch.float32)
            dA[:G * RP, :K] = dA064.float()
            ops.lora_da_fused(X, U, dA[:G * RP, :K], mods, rpi, r, n_groups=G)
            torch.cuda.synchronize()
            bits.append(dA.view(torch.int32).clone())
        got = dA[:G * RP, :K]
        assert torch.equal(got.double(), want), which
        if which == 1:
            unused = ~keep.any(0)                              # adapter rows of the modalities no image has
            assert int(unused.sum()) == G * (RP - r)
            assert torch.equal(got[unused].view(torch.int32), dA064[unused].float().view(torch.int32))
        assert bool(is_sentinel(dA[:G * RP, K:]).all() and is_sentinel(dA[G * RP:]).all()), which
        assert torch.equal(bits[0], bits[1]), which


def _refused(ops, Rp, rpi, r):
    """ops.lora_bwd_fused must raise an argument error before any launch: every output still holds its sentinel."""
    from prcv2025reid_amd._lib import ReidHipError
    fmt = flavor()
    n_img = 64 if rpi == 1 else 2
    M, N = n_img * rpi, 768
    dY = torch.zeros(M, N, dtype=T16(), device='cuda')
    Tm = torch.zeros(M, Rp, dtype=T16(), device='cuda')
    BT = torch.zeros(Rp, N, dtype=T16(), device='cuda')
    U = sentinel_buffer(M, Rp, T16(), fmt)
    dB = sentinel_buffer(N, Rp, torch.float32)
    mods = torch.zeros(n_img, dtype=torch.int32, device='cuda')
    with pytest.raises(ReidHipError) as ei:
        ops.lora_bwd_fused(dY, Tm, BT, U, dB, mods, rpi, r, 2.0)
    torch.cuda.synchronize()
    assert bool(is_sentinel(U, fmt).all() and is_sentinel(dB).all())
    return str(ei.value)


def test_lora_rp64_domain(ops):
    assert ops.lora_bwd_fused_ok(768, 64, 1, 16) is False
    assert ops.lora_bwd_fused_ok(768, 64, 197, 16) is True
    assert ops.lora_bwd_fused_ok(768, 32) is True
    assert ops.lora_bwd_fused_ok(768, 32, 1, 8) is True and ops.lora_bwd_fused_ok(3072, 64, 197, 16) is True
    assert not ops.lora_bwd_fused_ok(768, 64) and not ops.lora_bwd_fused_ok(768, 64, 197, 32) and not ops.lora_bwd_fused_ok(768, 96, 197, 16)
    assert not ops.lora_bwd_fused_ok(768, 128, 197, 16)
    assert ops.lora_da_fused_ok(768, 64, 197, 16, 1) and ops.lora_da_fused_ok(768, 64, 197, 16, 3)
    assert not ops.lora_da_fused_ok(768, 128, 197, 16, 1)
    msg = _refused(ops, 64, 1, 16)                              # the class-row form: no kernel for 64 adapter columns
    assert 'rows_per_img' in msg and '32' in msg
    _refused(ops, 96, 197, 16)
