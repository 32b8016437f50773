"""CPU: tests/optim_ref.py, the fp64 reference the GPU test of csrc/optim.hip holds the kernels to -- pinned against the library calls
it restates (torch.optim.AdamW in float64, clip_grad_norm_ on float32 tensors, the step oracle's percentile rule), and shown to
discriminate: on the GPU test's own inputs a float32 evaluation of the update passes the per-element allowances whether or not it
fuses its multiply-adds, and each of ten wrong updates, rounded the same way, fails them."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R
from oracle import step_oracle as so

COMBOS = ((R.BETAS[0], None), (R.BETAS[1], 1.0), (R.BETAS[0], 0.25), (R.BETAS[1], 0.0))      # those of test_optim_exact_gpu.py
LR = [e[1] for e in R.ENTRIES]
WD = [e[2] for e in R.ENTRIES]
GRAD_ENTRIES = [i for i, e in enumerate(R.ENTRIES) if e[3]]


# ------------------------------------------------------------------------------------------------------------ the reference
def test_inputs_hold_what_the_gpu_test_relies_on():
    assert R.SIZES == (1, 2, 3, 4, 5, 1023, 1024, 1025, 131072, 131079, 262151)
    null = [i for i, e in enumerate(R.ENTRIES) if not e[3]]
    assert null == [8] and 0 < null[0] < len(R.ENTRIES) - 1
    for t in R.STEPS:
        x = R.inputs(t)
        g = R.flat(x['g'])
        mag = np.abs(g[np.abs(g) >= 1e-12].astype(np.float64))
        assert mag.min() < 1e-11 and mag.max() > 1e3 and (g > 0).any() and (g < 0).any()
        assert (g == 0).sum() >= 12 and np.signbit(g[g == 0]).any() and not np.signbit(g[g == 0]).all()
        assert ((g != 0) & (np.abs(g) < 2.0 ** -126)).any() and (np.abs(g) == np.float32(1e-25)).any()
        big = x['g'][-1]                                                    # zeros and denormals in the second and third pass too
        assert big[R.PASS + 1] == 0 or abs(big[R.PASS + 1]) < 1e-20
        assert all(np.isfinite(a).all() for k in 'pgmv' for a in x[k])
        assert all((v >= 0).all() for v in x['v'])
        if t > 1:                                                           # zero gradient AND zero first moment, in the 5e-5 / 1e-4 entries
            for i in (5, 10):
                assert R.ENTRIES[i][1:3] == (5e-5, 1e-4) and ((x['g'][i] == 0) & (x['m'][i] == 0)).sum() >= 3
    for lr, wd in zip(LR, WD):                                              # 1 - lr wd: exact and material for the power-of-two pairs
        w = np.float32(1.0) - np.float32(lr) * np.float32(wd)
        if math.frexp(lr)[0] == 0.5 and wd:
            assert float(w) == 1.0 - lr * wd and float(w) <= 1.0 - 2.0 ** -14
    assert np.float32(1.0) - np.float32(5e-5) * np.float32(1e-4) == np.float32(1.0)
    assert any(a[2] == 0.0 and b[2] != 0.0 for a, b in zip(R.ENTRIES[1:], R.ENTRIES))


def test_adamw_matches_torch_adamw_in_float64():
    rng = np.random.default_rng(1)
    for (b1, b2), lr, wd in ((R.BETAS[0], 3e-3, 1e-4), (R.BETAS[1], 2.0 ** -6, 2.0 ** -3), (R.BETAS[0], 5e-5, 0.0)):
        f = lambda x: float(np.float32(x))
        p = rng.standard_normal(257).astype(np.float32).astype(np.float64)
        tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = torch.optim.AdamW([tp], lr=f(lr), weight_decay=f(wd), betas=(f(b1), f(b2)), eps=f(R.EPS), foreach=False)
        m, v = np.zeros_like(p), np.zeros_like(p)
        for t in range(1, 6):
            g = (10.0 ** rng.uniform(-12, 4, p.size) * rng.choice([-1.0, 1.0], p.size)).astype(np.float32).astype(np.float64)
            g[::9] = 0.0
            tp.grad = torch.from_numpy(g.copy())
            opt.step()
            (p, m, v), _ = R.adamw(p, g, m, v, None, lr, wd, b1, b2, R.EPS, t, round_bc=False)
            st = opt.state[tp]
            for got, ref in ((p, tp.detach().numpy()), (m, st['exp_avg'].numpy()), (v, st['exp_avg_sq'].numpy())):
                assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), t
    # the coefficient multiplies the gradient, nothing else
    (p2, m2, v2), _ = R.adamw(p, g, m, v, 0.25, lr, wd, b1, b2, R.EPS, 6)
    (p3, m3, v3), _ = R.adamw(p, g * 0.25, m, v, None, lr, wd, b1, b2, R.EPS, 6)
    assert np.array_equal(p2, p3) and np.array_equal(m2, m3) and np.array_equal(v2, v3)


@pytest.mark.parametrize('case', ['plain', 'clipped', 'nonfinite', '1e20', '1e-25', 'zero'])
def test_sanitize_and_clip_match_clip_grad_norm(case):
    rng = np.random.default_rng(5)
    gs = [rng.standard_normal(n).astype(np.float32) * np.float32(0.01 if case == 'plain' else 1.0) for n in (40, 7, 1)]
    if case == 'nonfinite':
        gs[0][3] = np.float32('nan'); gs[1][6] = np.float32('inf'); gs[2][0] = np.float32('-inf')
    elif case == '1e20':
        gs[1][2] = np.float32(1e20)
    elif case == '1e-25':
        gs = [np.full(n, 1e-25, dtype=np.float32) for n in (40, 7, 1)]
    elif case == 'zero':
        gs = [np.zeros(n, dtype=np.float32) for n in (40, 7, 1)]
    clean, sums, allow = zip(*[R.sanitize_sumsq(g) for g in gs])
    for g, c in zip(gs, clean):                                             # finite entries keep their bits, the others become +0.0
        fin = np.isfinite(g)
        assert np.array_equal(c.view(np.int32)[fin], g.view(np.int32)[fin]) and not c.view(np.int32)[~fin].any()
    assert sum(b for _, b in sums) == (3 if case == 'nonfinite' else 0)
    s = sum(x for x, _ in sums)
    st = R.clip(np.zeros(R.ST_FLOATS, np.float32), math.sqrt(s), 0, 0, 0.5)
    tg = [torch.nn.Parameter(torch.zeros(c.size)) for c in clean]
    for t, c in zip(tg, clean):
        t.grad = torch.from_numpy(c.copy())
    tn = float(torch.nn.utils.clip_grad_norm_(tg, max_norm=0.5))
    coef = float(st[R.ST_COEF])
    if case == '1e20':
        assert math.isinf(tn) and math.isinf(float(st[R.ST_NORM])) and coef == 0.0
        assert all(float(t.grad.abs().max()) == 0.0 for t in tg)
        return
    if case in ('1e-25', 'zero'):                                           # the squares underflow: norm 0, nothing is scaled
        assert tn == 0.0 and float(st[R.ST_NORM]) == 0.0 and coef == 1.0 and sum(allow) <= 48 * R.TINY
        assert all(np.array_equal(t.grad.numpy().view(np.int32), c.view(np.int32)) for t, c in zip(tg, clean))
        return
    # torch sums 48 squares in fp32 in its own order (<= 48 u relative on the sum, half of it on the norm), adds 1e-6 and forms
    # max_norm * (1 / x) instead of one quotient: two more roundings than the reference's float32 formula
    assert abs(tn - float(st[R.ST_NORM])) <= 25 * R.U * tn
    assert (coef == 1.0) == (case == 'plain')
    for t, c in zip(tg, clean):
        want = c.astype(np.float64) * coef
        assert np.all(np.abs(t.grad.numpy() - want) <= (25 + 4) * R.U * np.abs(want))


def test_clip_history_matches_the_step_oracle():
    cases = {
        'ten': [1.0] * 10,                                                  # needs MORE than ten
        'three': [0.25, 4.0, 2.0],
        'eleven': [float(i) for i in range(1, 12)],                         # last ten 2 .. 11: p70 = 8.3, clamps to 3
        'tenths': [0.1 * i for i in range(1, 12)],                          # 0.83 * 1.15: unclamped
        'ties': [2.0] + [0.75] * 6 + [1.5] * 4 + [0.75],
        'low': [0.01] * 11,                                                 # clamps to 0.5
        'wrap': [0.3 * (i % 7) + 0.2 for i in range(27)],                   # the ring wraps twice
    }
    for name, norms in cases.items():
        st, hist = np.zeros(R.ST_FLOATS, np.float32), []
        for i, n in enumerate(norms):
            before = st.copy()
            st = R.clip(st, n, 1, 1, 0.5)
            hist.append(float(np.float32(n)))                                # (the device keeps float32 norms)
            want = so.adaptive_max_norm(hist)
            assert abs(float(st[R.ST_MAXNORM]) - want) <= 2 * R.U * want, (name, i)
            assert int(st[R.ST_HCOUNT]) == i + 1 and st[R.ST_HIST + i % 10] == np.float32(n)
            keep = [k for k in range(10) if k != i % 10]
            assert np.array_equal(st[R.ST_HIST:][keep], before[R.ST_HIST:][keep])
            assert float(st[R.ST_COEF]) == float(R.clip_coef(np.float32(n), st[R.ST_MAXNORM]))
            quiet = R.clip(st, 7.0, 1, 0, 0.5)                               # not recorded: history untouched, the same max_norm
            assert np.array_equal(quiet[R.ST_HCOUNT:], st[R.ST_HCOUNT:]) and quiet[R.ST_MAXNORM] == st[R.ST_MAXNORM]
            fixed = R.clip(st, 7.0, 0, 1, 0.25)                              # not adaptive: the fixed value, history untouched
            assert np.array_equal(fixed[R.ST_HCOUNT:], st[R.ST_HCOUNT:]) and float(fixed[R.ST_MAXNORM]) == 0.25
    assert float(R.clip(np.zeros(20, np.float32), 5.0, 0, 0, 0.5)[R.ST_COEF]) == float(np.float32(0.5) / (np.float32(5.0) + np.float32(1e-6)))
    # the device period: recorded when the batch counter read is a multiple of the period
    a = b = np.zeros(R.ST_FLOATS, np.float32)
    for i in range(25):
        a = R.clip(a, 0.5 + 0.125 * i, 1, -3, 0.5)
        b = R.clip(b, 0.5 + 0.125 * i, 1, int(i % 3 == 0), 0.5)
        assert np.array_equal(a[:R.ST_BATCH], b[:R.ST_BATCH]) and int(a[R.ST_BATCH]) == i + 1 and int(b[R.ST_BATCH]) == 0
    assert int(a[R.ST_HCOUNT]) == 9


def test_bias_corrections():
    for b1, b2 in R.BETAS:
        for t in (1, 2, 10, 1000, 100000, 100002):
            c1, c2 = R.bias_corrections(b1, b2, t)
            assert c1.dtype == np.float32 and 0 < c1 <= 1 and 0 < c2 <= 1
    assert R.bias_corrections(0.9, 0.999, 1)[0] == np.float32(1.0) - np.float32(0.9)
    assert R.bias_corrections(0.5, 0.75, 2) == (np.float32(0.75), np.float32(math.sqrt(1 - 0.75 ** 2)))
    assert R.bias_corrections(0.9, 0.999, 100000) == (np.float32(1.0), np.float32(1.0))


# ------------------------------------------------------------------------------------------ restatements pass, mutants fail
def _run(t, betas, coef, fused, variant=None, lr=None, wd=None, t_used=None, betas_used=None):
    x = R.inputs(t)
    b = betas_used or betas
    return R.adamw_f32(R.flat(x['p']), R.flat(x['g']), R.flat(x['m']), R.flat(x['v']), coef, R.per_element(lr or LR),
                       R.per_element(wd or WD), b[0], b[1], R.EPS, t_used or t, fused=fused, variant=variant)


def _worst(got, t, betas, coef):
    (P, M, V), (eP, eM, eV) = R.expected(t, betas, coef)
    return tuple(R.ratio(g, r, e) for g, r, e in zip(got, (P, M, V), (eP, eM, eV)))


@pytest.mark.parametrize('fused', [False, True])
def test_straight_restatements_pass_every_element(fused):
    worst = (0.0, 0.0, 0.0)
    for t in R.STEPS:
        for betas, coef in COMBOS:
            r = _worst(_run(t, betas, coef, fused), t, betas, coef)
            assert max(r) <= 1.0, (t, betas, coef, r)
            worst = tuple(max(a, b) for a, b in zip(worst, r))
    print(f'float32 restatement (fused={fused}): worst error / allowance p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}')
    assert min(worst) > 0.01                                                 # the allowances are of the size of real rounding


def _swapped(vals, i, j):
    vals = list(vals); vals[i], vals[j] = vals[j], vals[i]
    return vals


MUTANTS = {
    'weight decay dropped': dict(wd=[0.0] * len(WD)),
    'wd = 0 entry decayed with its neighbour\'s wd': dict(wd=[max(WD[i - 1], WD[i + 1]) if w == 0.0 else w for i, w in enumerate(WD)]),
    'two entries\' lr exchanged': dict(lr=_swapped(LR, 6, 7)),
    'eps dropped': dict(variant='no_eps'),
    'eps inside the square root': dict(variant='eps_in_sqrt'),
    'bc1 and bc2 exchanged': dict(variant='bc_swapped'),
    'step off by one': 'step',
    'beta1 and beta2 exchanged': 'betas',
    'coef ignored': dict(variant='coef_ignored'),
    'coef applied for m but not for v': dict(variant='coef_m_only'),
}


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('name', list(MUTANTS))
def test_mutants_fail(name, fused):
    """Each wrong update must leave at least one element of p, m or v outside its allowance in at least one of the GPU test's
    configurations -- and by a wide margin, or the allowance would be doing the work of a tolerance."""
    worst, where = 0.0, None
    for t in R.STEPS:
        for betas, coef in COMBOS:
            kw = MUTANTS[name]
            if kw == 'step':
                kw = dict(t_used=t + 1)
            elif kw == 'betas':
                kw = dict(betas_used=betas[::-1])
            r = max(_worst(_run(t, betas, coef, fused, **kw), t, betas, coef))
            if r > worst:
                worst, where = r, (t, betas, coef)
            if worst > 100.0:
                break
        if worst > 100.0:
            break
    print(f'{name} (fused={fused}): worst error / allowance {worst:.3g} at t, betas, coef = {where}')
    assert worst > 100.0, name


def test_mutants_touch_the_entries_they_claim():
    """The per-entry mutants are caught IN the entry they change: the wd = 0 entries for the neighbour's decay, the two exchanged
    entries for lr, every decaying power-of-two entry for the dropped decay."""
    t, betas, coef = 10, R.BETAS[0], None
    (P, M, V), (eP, eM, eV) = R.expected(t, betas, coef)

    def per_entry(kw):
        got = _run(t, betas, coef, False, **kw)[0]
        return [R.ratio(g, r, e) for g, r, e in zip(R.split(got), R.split(P), R.split(eP))]

    ok = per_entry({})
    assert max(ok) <= 1.0
    r = per_entry(MUTANTS['wd = 0 entry decayed with its neighbour\'s wd'])
    assert r[1] > 100 and r[7] > 100 and max(x for k, x in enumerate(r) if k not in (1, 7)) <= 1.0
    r = per_entry(MUTANTS['two entries\' lr exchanged'])
    assert r[6] > 100 and r[7] > 100 and max(x for k, x in enumerate(r) if k not in (6, 7)) <= 1.0
    r = per_entry(MUTANTS['weight decay dropped'])
    for k, i in enumerate(GRAD_ENTRIES):
        if WD[i] and math.frexp(LR[i])[0] == 0.5:
            assert r[k] > 100, R.ENTRIES[i]
