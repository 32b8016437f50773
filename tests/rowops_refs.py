"""fp64 references, input families and per-element allowances of test_head_small_exact_gpu.py / test_rowops_exact_gpu.py (checked on
their own, against torch in float64 on the CPU, by test_rowops_refs_cpu.py).  Everything here is device-agnostic torch.

Allowances are first-order rounding counts of the kernels' own operation order, u = 2^-24 per fp32 operation:
  * a row sum of `cols` terms is a lane's chain (cols / 64 terms, at least 4) followed by six shuffle levels: every term passes through
    at most k = cols / 64 + 10 roundings, so |d sum| <= k u sum|term|;
  * sqrt and division are correctly rounded (u), rsqrtf is good to 2 ulp (4u), a 64-term dot through wave_sum costs 8u sum|term| (one
    product, six levels, one spare), an 8-term chain 8u."""
import torch

U32 = 2.0 ** -24


def f32(v):
    """The value a C `float` argument takes (eps = 1e-5 is not an fp32 number)."""
    return float(torch.tensor(v, dtype=torch.float32))


def assert_within(got, ref, allow, what, half_quantum=None):
    """|got - ref| <= allow (+ half a spacing of the 16-bit output format) for EVERY element; NaN in `got` fails."""
    got = got.double()
    lim = allow if half_quantum is None else allow + half_quantum
    bad = ~((got - ref).abs() <= lim)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, first at {i}: got {float(got[i])!r} '
                             f'ref {float(ref[i])!r} |d| {abs(float(got[i]) - float(ref[i])):.3e} bound {float(lim[i]):.3e}')
    return float(((got - ref).abs() / lim.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_FAMILIES = ('randn', 'mean10', 'mean1000', 'outlier')


def ln_family(name, rows, cols, gen):
    """fp32 rows of the family: unit normal; mean / std = 10 and 1000 (where a one-pass variance loses everything); one outlier channel
    100 x the rest (CLIP's residual stream)."""
    x = torch.randn(rows, cols, generator=gen, dtype=torch.float32, device=gen.device)
    if name == 'mean10':
        x = x + 10.0
    elif name == 'mean1000':
        x = x + 1000.0
    elif name == 'outlier':
        x[:, cols // 3] *= 100.0
    return x


def ln_chain(cols):
    return cols / 64 + 10


def ln_stats_ref(x, eps):
    """fp64 mean and rstd of the rows of `x` with the allowance of an fp32 two-pass evaluation:
    |d mean| <= (k + 2) u mean|x| =: dm (sum, division);  the centred second pass sees mean + delta, so it sums var + delta^2, each
    square off by 3u and the chain by k u, division and + eps 2u:  relative r = (dm^2 + (k + 6) u (var + dm^2)) / (var + eps) on the
    radicand, half of it (to second order) on rstd, plus 4u rsqrtf and one spare."""
    cols = x.shape[1]
    k = ln_chain(cols)
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    dm = (k + 2) * U32 * x.abs().mean(1)
    w = var + eps
    rstd = w ** -0.5
    r = (dm * dm + (k + 6) * U32 * (var + dm * dm)) / w
    return mu, dm, rstd, rstd * (0.5 * r * (1 + r) + 5 * U32)


def ln_y_ref(x, mean, rstd, gamma, beta):
    """fp64 y = (x - mean) rstd gamma + beta from GIVEN statistics (the kernel's own) and what fp32 may add: the subtraction and two
    products on t = (x - mean) rstd gamma (3u, one spare), the final add (u |y|)."""
    t = (x - mean[:, None]) * rstd[:, None] * gamma
    y = t + beta
    return y, 4 * U32 * t.abs() + U32 * y.abs()


# ---------------------------------------------------------------------------------------------------------------- L2 norm
def l2norm_ref(x, eps, scale):
    """fp64 y = x scale / max(||x||, eps); fp32: the sum of squares (k + 1) u (halved by the root), sqrt, division, product 3u, one spare."""
    k = ln_chain(x.shape[1])
    n = (x * x).sum(1).sqrt().clamp_min(eps)
    y = x * (scale / n)[:, None]
    return y, y.abs() * ((k + 1) / 2 + 4) * U32


# ---------------------------------------------------------------------------------------------------------------- im2col / masked mean
def im2col_ref(images, patch, cin):
    """[n, 3, H, W] -> [n (H/P)(W/P), cin P P] with column = c P P + py P + px; cin == 1 averages the three channels first."""
    n, _, H, W = images.shape
    img = images if cin == 3 else images.sum(1, keepdim=True) / 3.0
    gh, gw = H // patch, W // patch
    return img.reshape(n, cin, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * gh * gw, cin * patch * patch)


def masked_mean_ref(x, mask):
    """(sum_m mask x, max(count, 1)) of x [B, M, D], mask [B, M]."""
    return (x * mask[:, :, None]).sum(1), mask.sum(1).clamp_min(1.0)


# ---------------------------------------------------------------------------------------------------------------- small attention
def _heads(t, n_seq, S, heads):
    return t.reshape(n_seq, S, heads, 64).permute(0, 2, 1, 3)


def _rows(t, n_seq, S, heads):
    return t.permute(0, 2, 1, 3).reshape(n_seq * S, heads * 64)


def attn_inputs(n_seq, S, heads, seed, spread=3.5):
    """(qkv, dout, key_mask) on the CPU, fp32-representable float64.  q and k have standard deviation `spread`, so the scaled scores
    q.k / 8 have standard deviation spread^2 ~ 12: they reach +-30.  The random key mask keeps at least one key per sequence and, from
    two keys on, masks key 0 of sequence 0 and leaves only the LAST key of the last sequence."""
    g = torch.Generator().manual_seed(seed)
    d = heads * 64
    qkv = torch.randn(n_seq * S, 3 * d, generator=g, dtype=torch.float32)
    qkv[:, :2 * d] *= spread
    dout = torch.randn(n_seq * S, d, generator=g, dtype=torch.float32)
    km = torch.rand(n_seq, S, generator=g) < 0.6
    km[torch.arange(n_seq), torch.randint(0, S, (n_seq,), generator=g)] = True
    if S > 1:
        km[0, 0] = False; km[0, 1] = True
        km[-1] = False; km[-1, S - 1] = True
    return qkv.double(), dout.double(), km


def attn_fwd_ref(qkv, key_mask, drop, n_seq, S, heads):
    """fp64 softmax(q k^T / 8 + mask) (dropout multipliers `drop` [n_seq heads, S, S] applied after the softmax) v.
    Returns out [n_seq S, d], probs [n_seq heads, S, S], and the terms of the allowance (attn_fwd_allow)."""
    d = heads * 64
    q, k, v = (_heads(qkv[:, i * d:(i + 1) * d], n_seq, S, heads) for i in range(3))
    s = q @ k.transpose(-1, -2) / 8.0
    sabs = q.abs() @ k.abs().transpose(-1, -2) / 8.0
    if key_mask is not None:
        s = s.masked_fill(~key_mask.bool()[:, None, None, :], float('-inf'))
    p = torch.softmax(s, -1)
    m = torch.ones_like(p) if drop is None else drop.reshape(n_seq, heads, S, S)
    out = (p * m) @ v
    a = (s - s.max(-1, keepdim=True).values)
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).abs()
    return _rows(out, n_seq, S, heads), p.reshape(n_seq * heads, S, S), dict(p=p, a=a, sabs=sabs, mv=(m[..., None] * v[:, :, None]).abs())


def attn_fwd_allow(t, expf_rel):
    """(allow_out [n_seq S, d], allow_probs [items, S, S]).  Exponent argument a_j = s_j - max: off by the score's dot (8u sum|q k| / 8) and
    the subtraction (u |a_j|) -- the error of the maximum shifts every key alike and cancels; e_j = exp(a_j) by that much relatively, plus
    the exponential's own error, which is NOT derived: `expf_rel` (g_j + sum_l p_l g_l) with g = 1 + |a| (the fast exponential scales its
    argument by log2 e first, an error proportional to |a|); the denominator is an 8-term chain and one division (9u):
        |d p_j| <= p_j (d_j + sum_l p_l d_l + 9u) (1 % for the second order),   out = sum_j p_j m_j v_j: two products and an 8-term chain (10u) on top."""
    p, a, sabs, mv = t['p'], t['a'], t['sabs'], t['mv']
    dj = 8 * U32 * sabs + U32 * a
    eta = dj + (p * dj).sum(-1, keepdim=True) + 9 * U32
    g = 1.0 + a
    cond = p * (g + (p * g).sum(-1, keepdim=True))
    allow_p = 1.01 * p * eta + expf_rel * cond + 2.0 ** -120        # (a result below fp32's normal range may be flushed to 0)
    n_seq, heads, S, _ = p.shape
    allow_o = ((allow_p + 10 * U32 * p)[..., None] * mv).sum(3)
    cond_o = (cond[..., None] * mv).sum(3)
    return _rows(allow_o, n_seq, S, heads), allow_p.reshape(n_seq * heads, S, S), _rows(cond_o, n_seq, S, heads)


def attn_bwd_ref(qkv, probs, drop, dout, n_seq, S, heads):
    """fp64 backward of attn_fwd_ref from GIVEN probabilities (the kernel's own saved ones: the backward calls no exponential), and the
    allowance of its fp32 evaluation.  dp_j = (go . v_j) m_j: 9u sum|go v| m;  dot = sum_j p_j dp_j: the dp errors and a 10u chain;
    ds_j = p_j (dp_j - dot) / 8: those, and 3u |ds_j|;  dq = ds k, dk = ds^T q, dv = (p m)^T go: 8-term chains of products (10u)."""
    d = heads * 64
    q, k, v = (_heads(qkv[:, i * d:(i + 1) * d], n_seq, S, heads) for i in range(3))
    go = _heads(dout, n_seq, S, heads)
    p = probs.reshape(n_seq, heads, S, S)
    m = torch.ones_like(p) if drop is None else drop.reshape(n_seq, heads, S, S)
    dp = (go @ v.transpose(-1, -2)) * m
    e_dp = 9 * U32 * (go.abs() @ v.abs().transpose(-1, -2)) * m.abs()
    dot = (p * dp).sum(-1, keepdim=True)
    e_dot = (p * e_dp).sum(-1, keepdim=True) + 10 * U32 * (p * dp.abs()).sum(-1, keepdim=True)
    ds = p * (dp - dot) / 8.0
    e_ds = p / 8.0 * (e_dp + e_dot) + 3 * U32 * ds.abs()
    dq, e_dq = ds @ k, e_ds @ k.abs() + 10 * U32 * (ds.abs() @ k.abs())
    dk, e_dk = ds.transpose(-1, -2) @ q, e_ds.transpose(-1, -2) @ q.abs() + 10 * U32 * (ds.abs().transpose(-1, -2) @ q.abs())
    pm = p * m
    dv, e_dv = pm.transpose(-1, -2) @ go, 10 * U32 * (pm.abs().transpose(-1, -2) @ go.abs())
    cat = lambda a, b, c: torch.cat([_rows(a, n_seq, S, heads), _rows(b, n_seq, S, heads), _rows(c, n_seq, S, heads)], 1)
    return cat(dq, dk, dv), cat(e_dq, e_dk, e_dv)


# The exponential's share (attn_fwd_allow): measured, not derived.  test_rowops_refs_cpu.py evaluates oracle.reid_oracle.attention_core in
# float32 (libm's exponential, 1 ulp) against float64 on attn_inputs of every shape of the GPU test and takes the worst
# |o32 - o64| / cond_out; the kernel's fast __expf (a few ulp) gets four times that.
ATTN_SHAPES = [(n_seq, S, heads) for S in (1, 2, 5, 8) for heads in (1, 8) for n_seq in (1, 3, 9)]
ATTN_ORACLE_WORST = 2.5e-6  # measured 2.464e-6 (41 u), rounded up
ATTN_EXPF_REL = 4.0 * ATTN_ORACLE_WORST


def attn_seed(n_seq, S, heads):
    return 1000 * S + 10 * heads + n_seq
