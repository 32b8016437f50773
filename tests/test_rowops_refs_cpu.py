"""CPU: the fp64 references and allowances of test_head_small_exact_gpu.py / test_rowops_exact_gpu.py (rowops_refs.py) checked on their
own against torch in float64, the method of test_loss_refs_cpu.py:

  * LayerNorm, L2 normalisation, softmax attention (forward, and backward against autograd), im2col and the masked mean agree with
    F.layer_norm, F.normalize, an explicit softmax attention / the oracle's attention_core, F.unfold and a plain loop;
  * the allowances are wide enough for an honest fp32 evaluation (the two-pass LayerNorm and F.normalize in torch float32 on the CPU
    pass them on every input family) and they bite: a variance divided by cols - 1, or a one-pass variance at |mean|/std = 1000, fails them;
  * the one constant that is measured instead of derived, the exponential's share of the small-attention allowance, is measured here."""
import pytest
import torch
import torch.nn.functional as F

import rowops_refs as R
from oracle import reid_oracle as O

COLS = (4, 8, 64, 260, 512, 768, 772, 1024)


@pytest.mark.parametrize('cols', COLS)
def test_layernorm_reference_and_allowance(cols):
    g = torch.Generator().manual_seed(cols)
    eps = R.f32(1e-5)
    gamma = torch.randn(cols, generator=g, dtype=torch.float32); beta = torch.randn(cols, generator=g, dtype=torch.float32)
    for fam in R.LN_FAMILIES:
        x = R.ln_family(fam, 5, cols, g)
        x64 = x.double()
        mu, dm, rstd, dr = R.ln_stats_ref(x64, eps)
        y64, _ = R.ln_y_ref(x64, mu, rstd, gamma.double(), beta.double())
        want = F.layer_norm(x64, (cols,), gamma.double(), beta.double(), eps)
        assert float((y64 - want).abs().max()) <= 1e-12 * float(want.abs().max())
        # a two-pass fp32 evaluation (the kernel's order of operations, torch float32 on the CPU): inside the allowance of the
        # statistics, and of y given ITS statistics
        m32 = x.sum(1) / cols
        d32 = x - m32[:, None]
        r32 = 1.0 / torch.sqrt((d32 * d32).sum(1) / cols + torch.tensor(eps, dtype=torch.float32))
        y32 = d32 * r32[:, None] * gamma + beta
        assert y32.dtype == torch.float32
        R.assert_within(m32.flatten(), mu, dm, f'{fam} mean')
        R.assert_within(r32.flatten(), rstd, dr, f'{fam} rstd')
        yk, ak = R.ln_y_ref(x64, m32.flatten().double(), r32.flatten().double(), gamma.double(), beta.double())
        R.assert_within(y32, yk, ak, f'{fam} y')
        # the gate bites: an unbiased variance, and (from mean/std = 1000 on) the one-pass variance
        var_unb = x64.var(1, unbiased=True) if cols > 1 else None
        with pytest.raises(AssertionError):
            R.assert_within((var_unb + eps) ** -0.5, rstd, dr, 'unbiased')
        if fam == 'mean1000' and cols >= 64:
            xs = x.float()
            one_pass = ((xs * xs).mean(1) - xs.mean(1) ** 2).clamp_min(0).double()
            with pytest.raises(AssertionError):
                R.assert_within((one_pass + eps) ** -0.5, rstd, dr, 'one-pass')
    c = torch.full((2, cols), 3.0, dtype=torch.float64)         # a constant row: y = beta, rstd = 1 / sqrt(eps)
    mu, dm, rstd, dr = R.ln_stats_ref(c, eps)
    assert torch.equal(mu, torch.full((2,), 3.0, dtype=torch.float64)) and float((rstd - eps ** -0.5).abs().max()) < 1e-9


@pytest.mark.parametrize('D', [4, 512, 1024])
def test_l2norm_reference_and_allowance(D):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(5, D, generator=g, dtype=torch.float32)
    x[1] = 0.0
    x[2] *= 2.0 ** -50                                            # norm below eps: y = x scale / eps
    eps = R.f32(1e-12)
    for scale in (1.0, 8.0):
        y, allow = R.l2norm_ref(x.double(), eps, scale)
        want = F.normalize(x.double(), dim=1, eps=eps) * scale
        assert float((y - want).abs().max()) <= 1e-14 * scale
        assert float(y[1].abs().max()) == 0.0
        assert float((y[2] - x[2].double() * scale / eps).abs().max()) <= 1e-15 * float(y[2].abs().max())
        R.assert_within(F.normalize(x, dim=1, eps=1e-12) * scale, y, allow, 'fp32 normalize')
        with pytest.raises(AssertionError):
            R.assert_within(y * (1 + 1e-5), y, allow, 'scaled')


def _torch_attention(qkv, km, drop, dout, n_seq, S, heads):
    """Softmax attention written out with autograd, float64."""
    d = heads * 64
    x = qkv.clone().requires_grad_(True)
    q, k, v = (x[:, i * d:(i + 1) * d].reshape(n_seq, S, heads, 64).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / 8.0
    if km is not None:
        s = s + torch.where(km, 0.0, float('-inf')).double()[:, None, None, :]
    p = torch.softmax(s, -1)
    pm = p if drop is None else p * drop.reshape(n_seq, heads, S, S)
    out = (pm @ v).transpose(1, 2).reshape(n_seq * S, d)
    out.backward(dout)
    return out.detach(), p.detach().reshape(n_seq * heads, S, S), x.grad


def test_attention_reference_and_measured_exponential_share():
    worst = 0.0
    for n_seq, S, heads in R.ATTN_SHAPES:
        qkv, dout, km = R.attn_inputs(n_seq, S, heads, R.attn_seed(n_seq, S, heads))
        g = torch.Generator().manual_seed(S)
        drop = (torch.rand(n_seq * heads, S, S, generator=g) < 0.7).double() * 2.0
        for mask, dr in ((None, None), (km, None), (km, drop)):
            out, p, t = R.attn_fwd_ref(qkv, mask, dr, n_seq, S, heads)
            o2, p2, g2 = _torch_attention(qkv, mask, dr, dout, n_seq, S, heads)
            assert float((out - o2).abs().max()) < 1e-12 and float((p - p2).abs().max()) < 1e-14
            dqkv, allow = R.attn_bwd_ref(qkv, p, dr, dout, n_seq, S, heads)
            assert float((dqkv - g2).abs().max()) <= 1e-12 * max(1.0, float(g2.abs().max()))
            assert bool((allow >= 0).all())
            if dr is not None:
                continue
            # the oracle's attention in float32 against float64, normalised by the condition term of the exponential's share
            d = heads * 64
            add = None if mask is None else torch.where(mask, 0.0, float('-inf'))[:, None, None, :]
            parts = [qkv[:, i * d:(i + 1) * d].reshape(n_seq, S, d) for i in range(3)]
            o64 = O.attention_core(*parts, heads, None if add is None else add.double()).reshape(n_seq * S, d)
            assert float((o64 - out).abs().max()) < 1e-12
            o32 = O.attention_core(*(x.float() for x in parts), heads, None if add is None else add.float()).reshape(n_seq * S, d)
            _, _, cond_o = R.attn_fwd_allow(t, 1.0)
            ok = cond_o > 0
            worst = max(worst, float(((o32.double() - o64).abs()[ok] / cond_o[ok]).max()))
    print(f'\n  fp32 oracle attention against fp64, worst |d out| / condition term over {len(R.ATTN_SHAPES)} shapes: {worst:.3e} '
          f'= {worst / R.U32:.2f} u;  rowops_refs.ATTN_ORACLE_WORST = {R.ATTN_ORACLE_WORST:.3e}')
    assert 0.8 * R.ATTN_ORACLE_WORST <= worst <= R.ATTN_ORACLE_WORST, 'rowops_refs.ATTN_ORACLE_WORST is not the measured value'
    assert R.ATTN_EXPF_REL == 4.0 * R.ATTN_ORACLE_WORST


def test_fully_masked_sequence_is_nan_in_the_reference():
    qkv, dout, km = R.attn_inputs(3, 5, 8, 7)
    km[1] = False
    out, p, _ = R.attn_fwd_ref(qkv, km, None, 3, 5, 8)
    o2, _, _ = _torch_attention(qkv, km, None, dout, 3, 5, 8)
    nan = torch.isnan(out)
    assert torch.equal(nan, torch.isnan(o2)) and bool(nan[5:10].all()) and not bool(nan[:5].any() or nan[10:].any())


@pytest.mark.parametrize('n,H,W,P', [(2, 32, 64, 16), (1, 16, 16, 8)])
def test_im2col_reference_is_unfold(n, H, W, P):
    g = torch.Generator().manual_seed(H + W)
    img = torch.randn(n, 3, H, W, generator=g, dtype=torch.float64)
    for cin in (3, 1):
        src = img if cin == 3 else img.mean(1, keepdim=True)
        want = F.unfold(src, P, stride=P).transpose(1, 2).reshape(n * (H // P) * (W // P), cin * P * P)
        assert float((R.im2col_ref(img, P, cin) - want).abs().max()) < 1e-15


def test_masked_mean_reference():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 8, generator=g, dtype=torch.float64)
    mask = (torch.rand(3, 5, generator=g) < 0.5).double(); mask[1] = 0.0
    s, cnt = R.masked_mean_ref(x, mask)
    for b in range(3):
        rows = [x[b, m] for m in range(5) if mask[b, m] > 0]
        want = torch.stack(rows).sum(0) / len(rows) if rows else torch.zeros(8, dtype=torch.float64)
        assert float((s[b] / cnt[b] - want).abs().max()) < 1e-15
