"""GPU: the kernels behind the backbone -- BN-neck, label-smoothed CE, SDM loss, AP/CMC -- element by element.

Floating-point kernels (csrc/head.hip, csrc/sdm.hip) are called through prcv2025reid_amd.ops on fp32 inputs and compared with the
same operation written plainly in fp64 on the exact upcast of those inputs (loss_refs.py).  Next to it runs the *fp32 floor*: the
plain PyTorch fp32 implementation on the CPU on the same inputs (F.batch_norm + F.normalize, F.cross_entropy, the oracle's SDM in
float32, autograd for the gradients).  Errors are normalised so that a large element cannot hide a small one:
  * by the row's own max|ref| for row-normalised outputs (y, dz, dx, dlogits, dq / dg row by row),
  * by the element's own |ref| for per-column statistics (mean, invstd, rnorm, running statistics),
  * by the sum of the absolute values of the summed terms (fp64) for reductions that may cancel (sum_dz, sum_dz_xhat, losses).
GATE: worst normalised kernel error <= 4 x max(worst normalised floor error on the same inputs, 2^-24).  4 = 2 x 2: the kernels use
the hardware rsqrt / exp / log (up to ~2 ulp where libm gives 1) and sum in another order (wave butterflies, LDS partials, atomics);
each can at most about double the constant of a u * sum|terms| bound.  Every test prints its kernel and floor figures (-s).

Output buffers are filled with a sentinel NaN pattern first: padding columns and 32 guard rows must keep it bit for bit.

reid_rank_metrics (csrc/metrics.hip) is exact: rank1 and npos must equal a numpy walk of the stable descending argsort, and
|ap - ref| <= 1e-12 (at most 8192 terms <= 1 summed in double in another order differ by <= 8192 x 2^-53 ~ 9e-13 before the
division by the number of positives).

The externally reduced form of reid_bnneck_fwd (count != rows: sums all-reduced by the caller) keeps the one-pass variance
sqsum / count - mu^2 and gets its own DERIVED bound, not the gate (test_bnneck_external_statistics): with d = the number of fp32
roundings a term of the sums passes through, |d mean| <= (d + 1) u E|x| and |d var| <= (3 d + 6) u E[x^2], i.e. a relative error of
the variance that grows as 1 + (mean / std)^2 -- the statement of include/reid_hip.h.

Measured on an MI355X, identical in both flavors (the kernels are fp32).  Worst kernel error with the floor of the same case, and
the largest share of its own gate any case used:

    output         kernel    floor     share of gate
    mean           5.9e-08   5.9e-08   0.25
    invstd         1.0e-07   6.6e-08   0.39      (before the fix: 7.3e-04 at |mean|/std = 30, 4.3e-01 at 1000, 8 rows)
    running_var    1.0e-07   1.1e-07   0.28
    rnorm          3.6e-06   7.1e-06   0.38
    y              1.1e-04   1.0e-04   0.39      (|mean|/std = 1000 columns: the fp32 rounding of the mean itself)
    dz             7.8e-06   9.4e-06   0.31
    dx             1.8e-04   1.8e-04   0.37
    sum_dz         2.2e-05   2.1e-05   0.39
    sum_dz_xhat    3.0e-04   3.0e-04   0.38
    ce row_loss    1.7e-07   1.6e-07   0.53
    ce loss_sum    1.3e-07   7.8e-09   0.55      (before the fix: 3.1e-07 at 1030 rows, over the gate of 2.4e-07)
    ce dlogits     *         *         0.50      (* rows whose only non-zero gradient is below fp32's 1 - p: kernel and floor both 1.0)
    sdm loss       1.2e-07   8.6e-08   0.47
    sdm dq         5.1e-07   5.2e-07   0.41
    sdm dg         5.3e-07   3.4e-07   0.39
    AP             |ap - ref| <= 5.6e-17 (8192 positives); rank1 and npos equal everywhere
    external BN    share of the derived bound: mean 0.15, invstd 0.09, running_var 0.25, y 0.06

With the one-pass variance the library had before, 42 of the 46 BN-neck cases fail this gate.
"""
import numpy as np
import pytest
import torch

import loss_refs as R
from helpers import exact_ints, is_sentinel, round16, sentinel_buffer

pytestmark = pytest.mark.gpu

GUARD = 32
F32 = lambda v: float(np.float32(v))            # the value a float parameter of the C ABI really carries
EPS, MOM = F32(1e-5), F32(0.1)
WORST = {}                                      # name -> (kernel, floor) worst over the module, printed per test


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


def padded_in(vals, ld):
    """fp32 device operand [rows, cols] inside a [rows + GUARD, ld] sentinel buffer: what lies beyond a row must never be read."""
    rows, cols = vals.shape
    buf = sentinel_buffer(rows + GUARD, ld, torch.float32)
    buf[:rows, :cols] = vals.cuda()
    return buf[:rows, :cols]


def out_buf(rows, cols, ld, dtype=torch.float32):
    buf = sentinel_buffer(rows + GUARD, ld, dtype, flavor())
    return buf, buf[:rows, :cols]


def assert_untouched(buf, rows, cols):
    f = flavor()
    assert bool(is_sentinel(buf[rows:], f).all()), 'guard rows were written'
    assert bool(is_sentinel(buf[:rows, cols:], f).all()), 'padding columns were written'
    assert not bool(is_sentinel(buf[:rows, :cols], f).any()), 'an output element was not written'


def report(tag, kernel, floor, factor=R.GATE_FACTOR):
    """Print every figure, then assert the gate on each."""
    bad = []
    for k in kernel:
        fl = floor[k]
        lim = R.gate_limit(fl, factor)
        w = WORST.get(k, (0.0, 0.0))
        WORST[k] = (max(w[0], kernel[k]), max(w[1], fl))
        if not kernel[k] <= lim:
            bad.append(k)
    print(f'\n  {tag} [{flavor()}]: ' + '  '.join(f'{k} {kernel[k]:.2e}/{floor[k]:.2e}' for k in kernel) + '   (kernel/floor)')
    assert not bad, f'{tag}: over the gate: ' + ', '.join(f'{k}: kernel {kernel[k]:.3e} > {R.GATE_FACTOR:g} x max(floor {floor[k]:.3e}, 2^-24)'
                                                         for k in bad)


# ---- BN-neck -----------------------------------------------------------------------------------------------------------------
MIXED = [0, 1, 3, 6, 10, 30, 100, 1000]         # ratios side by side, the way the fused feature has them (median 3-6, max 65)


def run_bnneck(ops, x, gamma, beta, rm, rv, dy, training, pad):
    """The four entry points on device copies of the CPU inputs; returns the outputs on the CPU plus the layout checks done."""
    rows, D = x.shape
    ld = D + pad
    xv = padded_in(x, ld); dyv = padded_in(dy, ld + 4 if pad else D)
    g_, b_ = gamma.cuda(), beta.cuda()
    rm2, rv2 = rm.cuda().clone(), rv.cuda().clone()
    ybuf, yv = out_buf(rows, D, ld + 8 if pad else D)
    ybbuf, ybv = out_buf(rows, D, ld + 8 if pad else D, T16())
    dxbuf, dxv = out_buf(rows, D, ld + 12 if pad else D)
    dzbuf, dzv = out_buf(rows, D, D)
    vec = lambda n: sentinel_buffer(1, n + GUARD, torch.float32).view(-1)
    s1, s2, mean, invstd, a, b = (vec(D) for _ in range(6))
    rn = vec(rows)
    if training:
        ops.bnneck_stats(xv, s1[:D], s2[:D])
    ops.bnneck_fwd(xv, g_, b_, rm2, rv2, s1 if training else None, s2 if training else None, float(rows), training, yv, ybv,
                   mean, invstd, rn, eps=EPS, momentum=MOM, scale=8.0)
    ops.bnneck_bwd_p1(dyv, xv, g_, b_, mean, invstd, rn, dzv, a, b, scale=8.0)
    ops.bnneck_bwd_p2(dzv, xv, g_, mean, invstd, a, b, float(rows), training, dxv)
    torch.cuda.synchronize()
    for buf in (ybuf, ybbuf, dxbuf, dzbuf):
        assert_untouched(buf, rows, D)
    for v, n in ((mean, D), (invstd, D), (a, D), (b, D), (rn, rows)) + (((s1, D), (s2, D)) if training else ()):
        assert bool(is_sentinel(v[n:]).all()) and not bool(is_sentinel(v[:n]).any())
    # the 16-bit copy is the round-to-nearest-even of the fp32 output the kernel itself wrote
    assert torch.equal(ybv.double(), round16(yv.double(), flavor())), '16-bit copy != round16(y)'
    if not training:
        assert torch.equal(rm2.cpu(), rm) and torch.equal(rv2.cpu(), rv), 'eval mode changed the running statistics'
    return dict(mean=mean[:D], invstd=invstd[:D], y=yv, rnorm=rn[:rows], running_mean=rm2, running_var=rv2, dz=dzv, sum_dz=a[:D],
                sum_dz_xhat=b[:D], dx=dxv)


def check_bnneck(ops, tag, inputs, training, pad):
    x, gamma, beta, rm, rv, dy = inputs
    got = run_bnneck(ops, x, gamma, beta, rm, rv, dy, training, pad)
    ref = R.bn_neck_plain(*(t.double() for t in inputs), training, eps=EPS, momentum=MOM)
    floor = R.bn_errors(R.bn_neck_floor(x, gamma, beta, rm, rv, dy, training, eps=EPS, momentum=MOM), ref)
    report(tag, R.bn_errors(got, ref), floor)


@pytest.mark.parametrize('rows', [8, 64])
@pytest.mark.parametrize('ratio', [0, 1, 10, 30, 100, 1000])
def test_bnneck_ratio_sweep(ops, rows, ratio):
    """x = m_c + s_c n with |m_c| / s_c = ratio in every column: the batch variance must not lose (ratio)^2 of fp32's precision."""
    check_bnneck(ops, f'bnneck rows {rows} ratio {ratio}', R.bn_inputs(rows, 512, [ratio], seed=rows + ratio), True, 0)


@pytest.mark.parametrize('rows,D,ratios,negative,pad,training', [
    (64, 512, MIXED, False, 8, True),            # ratios mixed across the columns, padded leading dimensions
    (64, 512, [30], True, 4, True),              # negative means
    (2, 64, [10], False, 0, True),
    (37, 100, [1, 30], True, 4, True),           # D a multiple of 4, not of 64
    (1024, 1024, [100], False, 0, True),
    (4100, 512, [30, 1000], False, 8, True),     # beyond the 64 x 64 row split of reid_bnneck_stats
    (64, 512, [10], False, 0, False),            # running statistics
    (37, 1024, MIXED, True, 8, False),
    (8, 64, MIXED, True, 4, True),
])
def test_bnneck_shapes(ops, rows, D, ratios, negative, pad, training):
    check_bnneck(ops, f'bnneck {rows}x{D} ratios {ratios} {"train" if training else "eval"} pad {pad}',
                 R.bn_inputs(rows, D, ratios, seed=rows + D, negative=negative), training, pad)


def test_bnneck_constant_column(ops):
    """Columns whose true variance is 0 (a constant far from 0, and all zeros): finite outputs, equal to the reference in the gate."""
    inputs = list(R.bn_inputs(64, 512, [10], seed=77))
    inputs[0][:, 5] = 3.7; inputs[0][:, 64] = 0.0; inputs[0][:, 300] = -1234.5678
    check_bnneck(ops, 'bnneck constant columns', tuple(inputs), True, 0)


def test_bnneck_external_statistics(ops):
    """sum / sqsum / count supplied by the caller as the sum over the two halves of a batch (count = 64, rows = 32: the
    data-parallel form), against the fp64 BN over the whole batch, at |mean|/std <= 1.

    This form cannot re-read the other half, so it keeps var = sqsum / count - mu^2.  Its bound is derived, not measured.  A term
    of a column sum passes through d roundings: its lane's serial chain (rows_half / 4 - 1 adds; + 1 for the product in sqsum),
    3 adds combining the four lanes, the atomic onto a zeroed word (exact), 1 add of the two halves: d = rows_half / 4 + 3.
      mean:  |d mu|  <= (d + 1) u E|x|                                  (+ 1: the division)
      var:   |d var| <= (d + 2) u E[x^2]  +  (2 (d + 1) + 1) u E[x^2]  +  u var  <=  (3 d + 6) u E[x^2]
             (sqsum / count;  mu * mu with |mu| <= E|x| and (E|x|)^2 <= E[x^2];  the subtraction)
      invstd = rsqrt(var + eps): relative error <= |d var| / (2 (var + eps)) + 3 u  (rsqrt 2 ulp, the sum)
    y then moves by the first-order image of those two: dz_c = |d mu_c| invstd |gamma| + |z_c - beta_c| e_c, and after the projection
    of the normalisation |d y_c| <= 8 rnorm (dz_c + |u_c| sum_k |u_k| dz_k); on top of that comes the ordinary gate of y."""
    rows, D, half = 64, 512, 32
    x, gamma, beta, rm, rv, dy = R.bn_inputs(rows, D, [0, 0.3, 1], seed=9)
    xd = x.cuda()
    s = [torch.empty(D, device='cuda') for _ in range(4)]
    ops.bnneck_stats(xd[:half], s[0], s[1]); ops.bnneck_stats(xd[half:], s[2], s[3])
    s1, s2 = s[0] + s[2], s[1] + s[3]
    y = torch.empty(half, D, device='cuda'); mean = torch.empty(D, device='cuda'); invstd = torch.empty(D, device='cuda')
    rn = torch.empty(half, device='cuda'); rm2, rv2 = rm.cuda().clone(), rv.cuda().clone()
    ops.bnneck_fwd(xd[:half], gamma.cuda(), beta.cuda(), rm2, rv2, s1, s2, float(rows), True, y, None, mean, invstd, rn, eps=EPS,
                   momentum=MOM, scale=8.0)
    ins = tuple(t.double() for t in (x, gamma, beta, rm, rv, dy))
    ref = R.bn_neck_plain(*ins, True, eps=EPS, momentum=MOM)
    X = ins[0]
    d = half // 4 + 3
    ex2 = (X * X).mean(0); var = ((X - X.mean(0)) ** 2).mean(0)
    b_mu = (d + 1) * R.U24 * X.abs().mean(0)
    b_var = (3 * d + 6) * R.U24 * ex2
    b_inv = b_var / (2 * (var + EPS)) + 3 * R.U24                                       # relative
    e_mu = ((mean.cpu().double() - ref['mean']).abs() / b_mu).max()
    e_inv = ((invstd.cpu().double() - ref['invstd']).abs() / ref['invstd'] / b_inv).max()
    rv_ref = ref['running_var']
    e_rv = ((rv2.cpu().double() - rv_ref).abs() / (MOM * b_var * rows / (rows - 1) + 4 * R.U24 * rv_ref)).max()
    z = ((X - ref['mean']) * ref['invstd'] * ins[1] + ins[2])[:half]
    dz = b_mu * ref['invstd'] * ins[1].abs() + (z - ins[2]).abs() * b_inv
    u = z * ref['rnorm'][:half, None]
    b_y = 8.0 * ref['rnorm'][:half, None] * (dz + u.abs() * (u.abs() * dz).sum(1, keepdim=True))
    fl = R.bn_neck_floor(x, gamma, beta, rm, rv, dy, True, eps=EPS, momentum=MOM)
    floor_y = R.err_rows(fl['y'][:half], ref['y'][:half])
    rowmax = ref['y'][:half].abs().amax(1, keepdim=True)
    e_y = ((y.cpu().double() - ref['y'][:half]).abs() / (b_y + R.gate_limit(floor_y) * rowmax)).max()
    print(f'\n  bnneck external statistics [{flavor()}]: share of the derived bound used: mean {float(e_mu):.3f}  invstd {float(e_inv):.3f}  '
          f'running_var {float(e_rv):.3f}  y {float(e_y):.3f}   (worst invstd bound {float(b_inv.max()):.2e} relative)')
    assert float(e_mu) <= 1.0 and float(e_inv) <= 1.0 and float(e_rv) <= 1.0 and float(e_y) <= 1.0


def test_bnneck_wrapper(ops):
    """head.BNNeckFn (the only caller of the kernels in the model) on one high-ratio case: forward, running statistics, gradients."""
    from prcv2025reid_amd.head import BNNeckFn
    inputs = R.bn_inputs(64, 512, MIXED, seed=4, negative=True)
    x, gamma, beta, rm, rv, dy = inputs
    xr, gr, br = (t.cuda().requires_grad_(True) for t in (x, gamma, beta))
    rm2, rv2 = rm.cuda().clone(), rv.cuda().clone()
    y = BNNeckFn.apply(xr, gr, br, rm2, rv2, True, MOM, EPS)
    y.backward(dy.cuda())
    ref = R.bn_neck_plain(*(t.double() for t in inputs), True, eps=EPS, momentum=MOM)
    got = dict(y=y.detach(), running_mean=rm2, running_var=rv2, dx=xr.grad, sum_dz=br.grad, sum_dz_xhat=gr.grad)
    floor = R.bn_errors(R.bn_neck_floor(x, gamma, beta, rm, rv, dy, True, eps=EPS, momentum=MOM), ref)
    report('BNNeckFn', R.bn_errors(got, ref), floor)


# ---- label-smoothed cross entropy ------------------------------------------------------------------------------------------------
def check_ce(ops, rows, C, scale, smoothing, mode, pad, seed):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(rows, C, generator=g) * scale).float()
    lab = torch.randint(0, C, (rows,), generator=g)
    lab[0] = 0 if seed % 2 else C - 1
    if rows >= 5:
        lab[0] = 0; lab[1] = C - 1; lab[2] = -1; lab[3] = C
    valid = None
    if mode == 'mixed':
        valid = (torch.rand(rows, generator=g) > 0.3).to(torch.uint8); valid[0] = 1
    elif mode == 'zero':
        valid = torch.zeros(rows, dtype=torch.uint8)
    sm = F32(smoothing)
    init = torch.tensor([0.0, 0.0]) if mode == 'zero' else torch.tensor([2.5, 3.0])
    zv = padded_in(z, C + pad)
    rl = sentinel_buffer(1, rows + GUARD, torch.float32).view(-1)
    acc = init.cuda().clone()
    vd = None if valid is None else valid.cuda()
    ops.ce_ls_fwd(zv, lab.cuda(), vd, rl, acc, sm)
    loss, lscale, _, ok = R.ce_plain(z.double(), lab, valid, sm, 1.0)
    cnt = int(ok.sum())
    gs = torch.tensor([0.7 / max(cnt, 1)], dtype=torch.float32)
    dlbuf, dlv = out_buf(rows, C, C + (pad + 4 if pad else 0))
    ops.ce_ls_bwd(zv, lab.cuda(), vd, gs.cuda(), dlv, sm)
    torch.cuda.synchronize()
    assert_untouched(dlbuf, rows, C)
    assert bool(is_sentinel(rl[rows:]).all())
    _, _, d, _ = R.ce_plain(z.double(), lab, valid, sm, float(gs[0]))
    fl_loss, fl_d = R.ce_floor(z, lab, valid, sm, float(gs[0]))
    acc = acc.cpu()
    assert float(acc[1]) == float(init[1]) + cnt, (float(acc[1]), cnt)                 # the count is exact
    if mode == 'zero':
        assert float(acc[0]) == 0.0 and float(dlv.abs().max()) == 0.0 and float(rl[:rows].abs().max()) == 0.0
    total = float(init[0]) + float(loss.sum()); total_scale = float(init[0]) + float(lscale.sum())
    fl_total = float((init[0] + fl_loss.sum()).float())
    kernel = dict(row_loss=R.err_sums(rl[:rows], loss, lscale), loss_sum=R.err_sums([float(acc[0])], [total], [total_scale]),
                  dlogits=R.err_rows(dlv, d))
    floor = dict(row_loss=R.err_sums(fl_loss, loss, lscale), loss_sum=R.err_sums([fl_total], [total], [total_scale]),
                 dlogits=R.err_rows(fl_d, d))
    return kernel, floor


@pytest.mark.parametrize('scale', [1, 30, 1e4])
@pytest.mark.parametrize('C', [1, 7, 64, 400, 1000, 4099])
def test_ce_label_smoothing_elementwise(ops, C, scale):
    """rows x smoothing x valid mask x padding for one (C, logit scale); labels 0, C-1, -1 and C in every case with >= 5 rows.
    The loss scale 1e4 is what nan_to_num (reid_eltwise_f32 op 6) can feed the classifier."""
    modes = ['none', 'mixed', 'zero']
    worst_k, worst_f = {}, {}
    i = 0
    for rows in (1, 5, 67, 1030):
        for smoothing in (0.0, 0.1):
            mode = modes[i % 3]; pad = 0 if i % 2 == 0 else 12
            k, f = check_ce(ops, rows, C, scale, smoothing, mode, pad, seed=1000 * i + C)
            print(f'\n    ce rows {rows} C {C} scale {scale:g} smoothing {smoothing} valid {mode} pad {pad}: '
                  + '  '.join(f'{n} {k[n]:.2e}/{f[n]:.2e}' for n in k), end='')
            for n in k:
                if n not in worst_k or k[n] / R.gate_limit(f[n]) > worst_k[n] / R.gate_limit(worst_f[n]):
                    worst_k[n], worst_f[n] = k[n], f[n]                                # the sub-case closest to its own gate
            i += 1
    report(f'ce C {C} scale {scale:g}', {'ce_' + n: v for n, v in worst_k.items()}, {'ce_' + n: v for n, v in worst_f.items()})


def test_ce_wrapper(ops):
    from prcv2025reid_amd.losses import CrossEntropyLSFn
    g = torch.Generator().manual_seed(8)
    rows, C = 67, 400
    z = (torch.randn(rows, C, generator=g) * 30).float(); lab = torch.randint(0, C, (rows,), generator=g); lab[2] = -1; lab[3] = C
    valid = (torch.rand(rows, generator=g) > 0.3).to(torch.uint8)
    zr = z.cuda().requires_grad_(True)
    loss, cnt = CrossEntropyLSFn.apply(zr, lab.cuda(), valid.cuda(), F32(0.1))
    (loss * 0.7).backward()
    l64, s64, _, ok = R.ce_plain(z.double(), lab, valid, F32(0.1), 1.0)
    n = int(ok.sum())
    assert float(cnt) == n
    gs = float(np.float32(0.7) / np.float32(n))
    d64 = R.ce_plain(z.double(), lab, valid, F32(0.1), gs)[2]
    fl, fd = R.ce_floor(z, lab, valid, F32(0.1), gs)
    kernel = dict(ce_mean=R.err_sums([float(loss)], [float(l64.sum()) / n], [float(s64.sum()) / n]), ce_dlogits=R.err_rows(zr.grad, d64))
    floor = dict(ce_mean=R.err_sums([float(fl.sum() / n)], [float(l64.sum()) / n], [float(s64.sum()) / n]), ce_dlogits=R.err_rows(fd, d64))
    report('CrossEntropyLSFn', kernel, floor)


# ---- SDM ---------------------------------------------------------------------------------------------------------------------
# The +-20 clamp of the scores cannot be reached: the rows are unit vectors and tau is clamped to >= 0.15, so |S| <= 1 / 0.15 = 6.67.
def sdm_reference(q, gal, ql, gl, qv, gv, P, N, tau_c, gs, dtype, plain=True):
    """Per-pair losses (+ scales) and both gradients of sum_p gs[p] loss_p on the valid rows, in `dtype`, on the CPU."""
    from oracle import reid_oracle as O
    qc = q.to(dtype).requires_grad_(True); gc = gal.to(dtype).requires_grad_(True)
    gi = gv.bool()
    losses, scales, flags = [], [], []
    tot = 0.0
    for p in range(P):
        qi = qv[p * N:(p + 1) * N].bool()
        y = (ql[qi].view(-1, 1) == gl[gi].view(1, -1)).to(dtype)
        qq = qc[p * N:(p + 1) * N][qi]
        if plain:
            L, sc = R.sdm_plain(qq, gc[gi], y, tau_c)
        else:
            L, sc = O.sdm_loss(qq, gc[gi], y.float(), tau=tau_c), torch.zeros(())
            if not L.requires_grad:
                L = L + 0.0 * (qq.sum() + gc.sum())
        losses.append(float(L)); scales.append(float(sc)); flags.append(1.0 if float(y.sum()) > 0 else 0.0)
        tot = tot + L * float(gs[p])
    tot.backward()
    return losses, scales, flags, qc.grad, gc.grad


@pytest.mark.parametrize('P,N,Mg,D,tau,pad,zero_rows', [
    (1, 16, 48, 32, 0.05, 8, False),             # D = 32: one K step; tau below the clamp
    (2, 64, 64, 64, 0.15, 0, True),
    (1, 130, 70, 1024, 0.2, 8, True),
    (2, 40, 33, 64, 0.5, 4, False),
    (1, 64, 64, 32, 0.9, 0, False),              # tau above the clamp
    (1, 1, 48, 64, 0.2, 4, False),               # N = 1
    (1, 16, 1, 64, 0.2, 0, False),               # Mg = 1
    (3, 64, 64, 64, 0.2, 8, False),              # pair 1 has no valid row
    (1, 600, 520, 512, 0.2, 0, False),           # 128-wide tiles, several tiles per side (atomics in the backward)
])
def test_sdm_elementwise(ops, P, N, Mg, D, tau, pad, zero_rows):
    """test_sdm's construction (random labels 0..9, ~20 % of the rows masked out) with the temperature clamp, the extreme widths,
    padded leading dimensions, exactly-zero rows (the eps = 1e-8 branch of the normalisation), pre-filled gradient buffers and
    gradients judged row by row."""
    g = torch.Generator().manual_seed(N + 7 * P + D)
    q = torch.randn(P * N, D, generator=g); gal = torch.randn(Mg, D, generator=g)
    ql = torch.randint(0, 10, (N,), generator=g); gl = torch.randint(0, 10, (Mg,), generator=g)
    qv = (torch.rand(P * N, generator=g) > 0.2).to(torch.uint8); gv = (torch.rand(Mg, generator=g) > 0.2).to(torch.uint8)
    qv[0] = 1; gv[0] = 1; ql[0] = gl[0]                                   # at least one positive pair
    if P >= 3:
        qv[N:2 * N] = 0
    if zero_rows:
        q[2] = 0.0; gal[3] = 0.0; qv[2] = 1; gv[3] = 1; ql[2] = gl[0]; gl[3] = ql[0]    # valid rows with positives, norm exactly 0
    tau_c = min(max(tau, 0.15), 0.5)
    gs = torch.linspace(0.7, 1.3, P)
    qd = padded_in(q, D + pad); gd = padded_in(gal, D + (2 * pad))
    dev = lambda t: t.cuda()
    ws = torch.empty(ops.sdm_ws_floats(P, N, Mg, D), device='cuda')
    res = torch.zeros(2 * P, device='cuda'); res2 = torch.zeros(2 * P, device='cuda')
    ops.sdm_fwd(qd, gd, dev(ql), dev(gl), dev(qv), dev(gv), tau, ws, res2, P=P)
    ops.sdm_fwd(qd, gd, dev(ql), dev(gl), dev(qv), dev(gv), tau, ws, res, P=P)
    assert torch.equal(res.view(torch.int32), res2.view(torch.int32)), 'two forward calls on the same inputs differ in bits'
    ref_l, ref_s, ref_f, ref_dq, ref_dg = sdm_reference(q, gal, ql, gl, qv, gv, P, N, tau_c, gs, torch.float64)
    fl_l, _, _, fl_dq, fl_dg = sdm_reference(q, gal, ql, gl, qv, gv, P, N, tau_c, gs, torch.float32, plain=False)
    res = res.cpu()
    assert res[1::2].tolist() == ref_f
    for p in range(P):
        if ref_f[p] == 0.0:
            assert float(res[2 * p]) == 0.0
    # gradients: zero-initialised buffers for the row-wise gate ...
    dqbuf, dq = out_buf(P * N, D, D + pad); dgbuf, dg = out_buf(Mg, D, D + pad)
    dq.zero_(); dg.zero_()
    ops.sdm_bwd(qd, gd, dev(ql), dev(gl), dev(qv), dev(gv), tau, ws, gs.cuda(), dq, dg, P=P)
    torch.cuda.synchronize()
    assert_untouched(dqbuf, P * N, D); assert_untouched(dgbuf, Mg, D)
    kernel = dict(sdm_loss=R.err_sums(res[0::2], ref_l, ref_s), sdm_dq=R.err_rows(dq, ref_dq), sdm_dg=R.err_rows(dg, ref_dg))
    floor = dict(sdm_loss=R.err_sums(fl_l, ref_l, ref_s), sdm_dq=R.err_rows(fl_dq, ref_dq), sdm_dg=R.err_rows(fl_dg, ref_dg))
    assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dg).all())
    # ... and pre-filled ones: dq / dg are `+=`.  The sum is rounded once more (u |pre + gradient|), nothing else may change.
    pre_q = exact_ints((P * N, D), -8, 8, -13, torch.Generator(device='cuda').manual_seed(1)).float()
    pre_g = exact_ints((Mg, D), -8, 8, -13, torch.Generator(device='cuda').manual_seed(2)).float()
    ws2 = torch.empty_like(ws); res3 = torch.zeros(2 * P, device='cuda')
    ops.sdm_fwd(qd, gd, dev(ql), dev(gl), dev(qv), dev(gv), tau, ws2, res3, P=P)
    aq, ag = pre_q.clone(), pre_g.clone()
    ops.sdm_bwd(qd, gd, dev(ql), dev(gl), dev(qv), dev(gv), tau, ws2, gs.cuda(), aq, ag, P=P)
    for name, acc, pre, ref, fl in (('dq', aq, pre_q, ref_dq, floor['sdm_dq']), ('dg', ag, pre_g, ref_dg, floor['sdm_dg'])):
        acc, pre = acc.cpu().double(), pre.cpu().double()
        zero = ref.abs().amax(1) == 0
        assert torch.equal(acc[zero], pre[zero]), f'{name}: a row without gradient changed'
        tol = R.gate_limit(fl) * ref.abs().amax(1, keepdim=True) + 2 * R.U24 * (pre + ref).abs()
        assert bool(((acc - pre - ref).abs() <= tol).all()), f'{name} is not pre-fill + gradient'
    report(f'sdm P{P} N{N} Mg{Mg} D{D} tau {tau}', kernel, floor)


def test_sdm_wrapper(ops):
    from prcv2025reid_amd.losses import SDMFn
    g = torch.Generator().manual_seed(21)
    P, N, Mg, D = 2, 48, 40, 512
    q = torch.randn(P * N, D, generator=g); gal = torch.randn(Mg, D, generator=g)
    ql = torch.randint(0, 6, (N,), generator=g); gl = torch.randint(0, 6, (Mg,), generator=g)
    qv = (torch.rand(P * N, generator=g) > 0.2).to(torch.uint8); gv = (torch.rand(Mg, generator=g) > 0.2).to(torch.uint8)
    gs = torch.tensor([0.6, 1.1])
    qr = q.view(P, N, D).cuda().requires_grad_(True); gr = gal.cuda().requires_grad_(True)
    loss, flag = SDMFn.apply(qr, gr, ql.cuda(), gl.cuda(), qv.view(P, N).cuda(), gv.cuda(), 0.9)
    (loss * gs.cuda()).sum().backward()
    ref_l, ref_s, ref_f, ref_dq, ref_dg = sdm_reference(q, gal, ql, gl, qv, gv, P, N, 0.5, gs, torch.float64)
    fl_l, _, _, fl_dq, fl_dg = sdm_reference(q, gal, ql, gl, qv, gv, P, N, 0.5, gs, torch.float32, plain=False)
    assert flag.tolist() == ref_f
    kernel = dict(sdm_loss=R.err_sums(loss.detach(), ref_l, ref_s), sdm_dq=R.err_rows(qr.grad.view(P * N, D), ref_dq),
                  sdm_dg=R.err_rows(gr.grad, ref_dg))
    floor = dict(sdm_loss=R.err_sums(fl_l, ref_l, ref_s), sdm_dq=R.err_rows(fl_dq, ref_dq), sdm_dg=R.err_rows(fl_dg, ref_dg))
    report('SDMFn', kernel, floor)


# ---- AP / CMC ----------------------------------------------------------------------------------------------------------------
NAN32 = 0x7FBADBAD


def run_rank(ops, scores, g_pid, q_pid, g_img=None, excl=None, max_pos=None, pad=8, absent=()):
    """reid_rank_metrics on score rows built directly (no GEMM) against loss_refs.rank_metrics_ref query by query.
    scores [nq, Ng] float32 numpy; excl: list of up to four image ids per query (or None); absent: queries given slot -1."""
    nq, Ng = scores.shape
    ld = (Ng + 3) // 4 * 4 + pad
    S = sentinel_buffer(nq + 1, ld, torch.float32)                     # NaN beyond Ng: must not be read
    S[:nq, :Ng] = torch.from_numpy(scores).cuda()
    gp = torch.from_numpy(np.asarray(g_pid, dtype=np.int32))
    uniq, inv = torch.unique(gp.long(), return_inverse=True)
    order = torch.argsort(inv, stable=True)
    counts = torch.bincount(inv, minlength=uniq.numel())
    csr_off = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(torch.int32)
    qp = torch.as_tensor(np.asarray(q_pid), dtype=torch.long)
    pos = torch.searchsorted(uniq, qp).clamp(max=uniq.numel() - 1)
    slot = torch.where(uniq[pos] == qp, pos, torch.full_like(pos, -1)).to(torch.int32)
    for i in absent:
        slot[i] = -1
    ex = None
    if excl is not None:
        ex = torch.tensor([list(e) + [-1] * (4 - len(e)) for e in excl], dtype=torch.int32).cuda()
    gi = None if g_img is None else torch.from_numpy(np.asarray(g_img, dtype=np.int32)).cuda()
    ap = torch.full((nq + 1,), -7.0, dtype=torch.float64, device='cuda')
    r1 = torch.full((nq + 1,), -7, dtype=torch.int32, device='cuda'); npos = r1.clone()
    mp = int(counts.max()) if max_pos is None else max_pos
    ops.rank_metrics(S[:nq], gp.cuda(), gi, qp.to(torch.int32).cuda(), slot.cuda(), ex, csr_off.cuda(), order.to(torch.int32).cuda(),
                     Ng, mp, ap[:nq], r1[:nq], npos[:nq])
    torch.cuda.synchronize()
    assert float(ap[nq]) == -7.0 and int(r1[nq]) == -7 and int(npos[nq]) == -7
    assert bool(is_sentinel(S[:, Ng:]).all()) and bool(is_sentinel(S[nq:]).all())
    ap, r1, npos = ap.cpu().numpy(), r1.cpu().numpy(), npos.cpu().numpy()
    worst = 0.0
    out = []
    for i in range(nq):
        want = R.rank_metrics_ref(scores[i], g_pid, int(q_pid[i]), g_img, None if excl is None else excl[i], has_slot=i not in absent)
        got = (float(ap[i]), int(r1[i]), int(npos[i]))
        assert got[1:] == want[1:], (i, got, want)
        assert abs(got[0] - want[0]) <= 1e-12, (i, got, want)
        worst = max(worst, abs(got[0] - want[0]))
        out.append(got)
    return out, worst


@pytest.mark.parametrize('Ng', [1, 3, 4, 5, 4099, 200003])
@pytest.mark.parametrize('grid', [True, False])
def test_rank_metrics_sizes(ops, Ng, grid):
    """Scores on the grid k/8 (most entries tie; the index must decide) or continuous; every exclusion count 0..4, a pid that is
    absent from the gallery (slot -1), the vector body and the scalar tail of the row scan, NaN padding behind every row."""
    rng = np.random.default_rng(Ng)
    nq = 7
    npid = max(2, Ng // 50)
    g_pid = rng.integers(0, npid, Ng)
    g_img = rng.integers(-1, max(2, Ng // 3), Ng)                      # image ids repeat; -1 = none
    scores = (rng.integers(-8, 9, (nq, Ng)) / 8.0).astype(np.float32) if grid else rng.standard_normal((nq, Ng)).astype(np.float32)
    q_pid = [int(g_pid[rng.integers(0, Ng)]) for _ in range(nq - 1)] + [npid + 5]
    excl = []
    for i in range(nq):
        ids = [int(g_img[j]) for j in rng.integers(0, Ng, i % 5)]
        pos = np.nonzero(g_pid == q_pid[i])[0]
        if len(pos) and i % 2 and ids:
            ids[0] = int(g_img[pos[0]])                                # a positive that is itself excluded
        excl.append(ids)
    out, worst = run_rank(ops, scores, g_pid, q_pid, g_img, excl, absent=(2,) if Ng > 5 else ())
    print(f'\n  rank_metrics Ng {Ng} {"grid" if grid else "continuous"} [{flavor()}]: worst |ap - ref| {worst:.1e}; npos {[o[2] for o in out]}')


@pytest.mark.parametrize('np_,max_pos', [(1, None), (63, None), (64, None), (65, 100), (8192, None), (8193, None), (300, 777)])
def test_rank_metrics_positive_counts(ops, np_, max_pos):
    """The LDS list of positives at its capacities: 64 (the smallest), a max_pos that is not a power of two, 8192 (the largest), and
    one more, which is not evaluated (npos -1, ap 0, rank1 0)."""
    rng = np.random.default_rng(np_)
    Ng = 20000
    g_pid = np.arange(2, Ng + 2); g_pid[rng.permutation(Ng)[:np_]] = 1       # every negative has a pid of its own: the longest CSR row is np_
    scores = np.stack([(rng.integers(0, 5, Ng) / 8.0), rng.standard_normal(Ng), np.where(g_pid == 1, 0.5, rng.standard_normal(Ng))]).astype(np.float32)
    out, worst = run_rank(ops, scores, g_pid, [1, 1, 1], max_pos=max_pos)
    assert all(o[2] == (np_ if np_ <= 8192 else -1) for o in out)
    print(f'\n  rank_metrics {np_} positives max_pos {max_pos} [{flavor()}]: worst |ap - ref| {worst:.1e}')


def test_rank_metrics_tie_rules(ops):
    """Hand-built rows of 12 entries, pid 1 = positive.  Expected ranks are written out, and checked against the reference too."""
    P = [1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]                                       # positives at 0, 3, 7 and Ng - 1
    rows = [
        [0.5] * 12,                                                                 # all scores equal: rank = index + 1
        [0.5, 0.9, 0.1, 0.5, 0.7, 0.3, 0.6, 0.5, 0.2, 0.8, 0.4, 0.5],               # all positives share one score (s_first == s_last)
        [0.9, 0.5, 0.1, 0.7, 0.2, 0.5, 0.1, 0.5, 0.5, 0.1, 0.5, 0.6],               # negatives tie the weakest positive (index 7) on both sides
        [0.1, 0.9, 0.9, 0.1, 0.9, 0.9, 0.9, 0.1, 0.9, 0.9, 0.9, 0.1],               # every positive behind every negative
    ]
    scores = np.array(rows, np.float32)
    out, _ = run_rank(ops, scores, P, [1, 1, 1, 1])
    assert [o[1] for o in out] == [1, 5, 1, 9]                                        # row 1: four negatives above 0.5
    assert abs(out[0][0] - (1 / 1 + 2 / 4 + 3 / 8 + 4 / 12) / 4) < 1e-15
    # row 2: order 0(.9) 3(.7) 11(.6) then the 0.5 group by index: 1, 5, 7(+), 8, 10 -> the positive at 7 has rank 6
    assert abs(out[2][0] - (1 / 1 + 2 / 2 + 3 / 3 + 4 / 6) / 4) < 1e-15
    # exclusions on the tied row: image ids = index; drop the positive 3 and the negatives 1 and 5 that precede positive 7
    g_img = list(range(12))
    out, _ = run_rank(ops, scores[2:3].repeat(5, 0), P, [1] * 5, g_img,
                      [[], [3], [3, 1], [3, 1, 5], [0, 3, 7, 11]])
    assert [o[2] for o in out] == [4, 3, 3, 3, 0] and [o[1] for o in out] == [1, 1, 1, 1, 0]
    assert abs(out[3][0] - (1 / 1 + 2 / 2 + 3 / 3) / 3) < 1e-15                     # 0, 11, then 7 right behind them
    assert out[4] == (0.0, 0, 0)                                                    # every positive excluded
    # g_img NULL together with q_excl non-NULL: nothing is excluded
    out, _ = run_rank(ops, scores[2:3], P, [1], None, [[0, 3, 7, 11]])
    assert out[0][2] == 4

