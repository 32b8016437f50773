"""GPU: the one-pass attention backward (attn_bwd_fused_kernel: dS parked in LDS by the key-tile phase, dQ = dS K from that image)
at the sizes the other attention tests leave out -- the benchmark's two calls against the two-kernel form, and every tile count at
a full last tile and at one padded key row / query column -- element by element against fp64 with the bounds of
test_kernels_gpu._attn_ref64, and the same bits from a repeated call."""
import pytest
import torch

from test_kernels_gpu import ops, T16, rel_err, _attn_inputs, _attn_ref64_chunked, _check_elements, _fmt16, _rounding  # noqa: F401

pytestmark = pytest.mark.gpu


def _inputs(n_seq, S, heads, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    d = heads * 64
    q32, k32, v32, do32, _ = _attn_inputs(n_seq, S, heads, {}, g)
    qkv = torch.empty(n_seq * S, 3 * d, device='cuda', dtype=T16())
    qkv.view(n_seq, S, 3, heads, 64).copy_(torch.stack([q32, k32, v32], 2).permute(0, 3, 2, 1, 4))
    dout = torch.empty(n_seq * S, d, device='cuda', dtype=T16())
    dout.view(n_seq, S, heads, 64).copy_(do32.transpose(1, 2))
    return qkv, dout


def _backward(ops, qkv, out, dout, lse, n_seq, S, heads, q_tiles, knob):
    """dqkv (NaN-filled before the call: every element the call owns must be written) and the published delta of one call."""
    from prcv2025reid_amd import _lib
    d = heads * 64
    lib = _lib.lib()
    _lib.check(lib.reid_set_knob(b'ATTN_BWD', knob))
    try:
        dqkv = torch.full((n_seq * S, 3 * d), float('nan'), device='cuda', dtype=T16())
        delta = torch.full((n_seq, heads, S), float('nan'), device='cuda')
        ops.attn_bwd(qkv, out, dout, lse, dqkv, delta, n_seq, S, heads, q_tiles=q_tiles)
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.reid_set_knob(b'ATTN_BWD', -1))
    return dqkv, delta


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


def _forms(ops, n_seq, S, heads, q_tiles, seed):
    qkv, dout = _inputs(n_seq, S, heads, seed)
    d = heads * 64
    out = torch.empty(n_seq * S, d, device='cuda', dtype=T16())
    lse = torch.empty(n_seq, heads, S, device='cuda')
    ops.attn_fwd(qkv, out, lse, n_seq, S, heads, q_tiles=q_tiles)
    fused = _backward(ops, qkv, out, dout, lse, n_seq, S, heads, q_tiles, 2)
    again = _backward(ops, qkv, out, dout, lse, n_seq, S, heads, q_tiles, 2)
    two = _backward(ops, qkv, out, dout, lse, n_seq, S, heads, q_tiles, 1)
    assert _same_bits(fused[0], again[0]) and _same_bits(fused[1], again[1]), 'one-pass backward: a repeated call gave other bits'
    q_rows = min(S, 32 * q_tiles) if q_tiles else S
    fq = fused[0].view(n_seq, S, 3 * d)
    assert bool((fq[:, q_rows:, :d] == 0).all()), 'dQ of the rows left out by q_tiles not exactly 0'
    assert bool(torch.isfinite(fq[:, :q_rows]).all() and torch.isfinite(fq[:, :, d:]).all())
    # delta: the same products in the same order in both forms
    assert _same_bits(fused[1][:, :, :q_rows].contiguous(), two[1][:, :, :q_rows].contiguous()), 'published delta differs between the forms'
    tq = two[0].view(n_seq, S, 3 * d)
    for i, nm in enumerate(('dQ', 'dK', 'dV')):
        a, b = fq[:, :q_rows if i == 0 else S, i * d:(i + 1) * d], tq[:, :q_rows if i == 0 else S, i * d:(i + 1) * d]
        print(f'{nm}: one-pass vs two-kernel max |d| {float((a.float() - b.float()).abs().max()):.3e}')
        assert rel_err(a, b) < 2e-3, nm
    return qkv, dout, fused[0], q_rows


@pytest.mark.parametrize('q_tiles', [0, 1], ids=['vision_step', 'vision_cls'])
def test_attention_bwd_bench_calls(ops, q_tiles):
    """The benchmark's calls (256 images x 197 tokens x 12 heads; the last block's class rows only): the one-pass form against the
    two-kernel form, repeat bits, pruned rows."""
    _forms(ops, 256, 197, 12, q_tiles, 197 + q_tiles)


# every tile count with a full last tile and with one padded key row / query column of the dS image; q_tiles pruning at NT >= 2
TILE_CASES = [(nt, 32 * nt - pad, qt) for nt in range(1, 8) for pad in (0, 1) for qt in ((0, 1) if nt > 1 and pad else (0,))]


@pytest.mark.parametrize('nt,S,q_tiles', TILE_CASES, ids=[f'nt{c[0]}_S{c[1]}_qt{c[2]}' for c in TILE_CASES])
def test_attention_bwd_tiles_fp64(ops, nt, S, q_tiles):
    from prcv2025reid_amd import _lib
    n_seq, heads = 3, 2
    d = heads * 64
    qkv, dout, dqkv, q_rows = _forms(ops, n_seq, S, heads, q_tiles, 31 * S + nt)
    mant, emin = _fmt16(_lib.flavor())
    q, k, v = (qkv.double().view(n_seq, S, 3, heads, 64)[:, :, i].transpose(1, 2) for i in range(3))
    do = dout.double().view(n_seq, S, heads, 64).transpose(1, 2)
    allowed = torch.ones(1, 1, S, S, dtype=torch.bool, device='cuda')
    ref, bnd = _attn_ref64_chunked(q, k, v, do, allowed, q_rows, mant, emin)
    got3 = dqkv.view(n_seq, S, 3, heads, 64)
    ratios = {}
    for i, nm in enumerate(('dQ', 'dK', 'dV')):
        got, rr, bb = got3[:, :, i].transpose(1, 2), ref[nm], bnd[nm]
        if nm == 'dQ':
            got, rr, bb = got[:, :, :q_rows], rr[:, :, :q_rows], bb[:, :, :q_rows]
        tol = _rounding(rr.abs() + bb, mant, emin)
        _check_elements(got, rr, bb, tol, f'nt{nt} S{S} q_tiles={q_tiles} {nm}')
        ratios[nm] = float(((got.double() - rr).abs() / (bb + tol)).max())
    print(f'attention bwd [{_lib.flavor()}] nt{nt} S{S} q_tiles={q_tiles}: ' + ' '.join(f'{k_} {v_:.3f}' for k_, v_ in ratios.items()))
