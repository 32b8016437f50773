"""GPU: the fused optimizer's entry points (csrc/optim.hip) one by one through the C ABI against the fp64 reference of
tests/optim_ref.py -- reid_opt_adamw (host step and device counter), reid_opt_sumsq (read through reid_opt_clip's state),
reid_opt_clip on hand-written partials, and the arguments they refuse.

Every p / g / m / v is a 16-byte-aligned slice of one larger buffer with at least 16 sentinel floats on both sides; the table has one
entry per size of optim_ref.SIZES (the scalar tail alone, fewer vectors than threads, exact multiples, a second and a third
grid-stride pass with tails of 7) and one entry without a gradient in its middle.  p, m and v are held PER ELEMENT to the reference
plus its derived allowance (optim_ref.adamw), never to a global maximum; test_optim_ref_cpu.py shows that ten wrong updates fail
those allowances on these very inputs.  Each test prints its worst error / allowance ratio and runs under both build flavors."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import optim_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 16
ENT = R.ENTRIES
N_ENT = len(ENT)
GRAD = [i for i, e in enumerate(ENT) if e[3]]
NULL = [i for i, e in enumerate(ENT) if not e[3]][0]
COMBOS = ((R.BETAS[0], None, 0), (R.BETAS[1], 1.0, 1), (R.BETAS[0], 0.25, 1), (R.BETAS[1], 0.0, 0))      # betas, coef, zero_grad


@pytest.fixture(params=['bf16', 'f16'])
def L(request):
    """Every test runs once per build flavor: both libraries ship this code."""
    from prcv2025reid_amd import _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield _lib
    _lib.set_flavor('bf16')


def _layout(sizes):
    offs, off = [], GUARD
    for n in sizes:
        offs.append(off)
        off = (off + n + GUARD + 3) // 4 * 4
    return offs, off


OFFS, TOTAL = _layout([e[0] for e in ENT])


def _to_dev(words):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.int32)).cuda()


def _words(t):
    return t.view(torch.int32).cpu().numpy()


class Arena:
    """The four guarded device buffers of one table, and the table."""

    def __init__(self, arrs, lr=None, wd=None):
        from prcv2025reid_amd.trainer import _Entry
        self.dev, self.host0 = {}, {}
        for k in 'pgmv':
            w = np.full(TOTAL, SENTINEL32, dtype=np.int32)
            for a, o in zip(arrs[k], OFFS):
                w[o:o + a.size] = np.asarray(a, dtype=np.float32).view(np.int32)
            self.host0[k] = w
            self.dev[k] = _to_dev(w)
            assert self.dev[k].data_ptr() % 16 == 0
        ents = (_Entry * N_ENT)()
        for i, (e, o) in enumerate(zip(ENT, OFFS)):
            ptrs = [self.dev[k].data_ptr() + 4 * o for k in 'pgmv']
            assert all(p % 16 == 0 for p in ptrs)
            if not e[3]:
                ptrs[1] = None
            ents[i] = _Entry(ptrs[0], ptrs[1], ptrs[2], ptrs[3], e[0], float(lr[i] if lr else e[1]), float(wd[i] if wd else e[2]))
        assert C.sizeof(_Entry) == 48
        self.table = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8).cuda()

    def words(self, k):
        return _words(self.dev[k])

    def entry(self, w, i):
        return w[OFFS[i]:OFFS[i] + ENT[i][0]].view(np.float32)

    def flat(self, w):
        return np.concatenate([self.entry(w, i) for i in GRAD])

    def guards_intact(self, w):
        own = np.zeros(TOTAL, dtype=bool)
        for e, o in zip(ENT, OFFS):
            own[o:o + e[0]] = True
        assert (~own).sum() >= GUARD * (N_ENT + 1)
        return bool((w[~own] == SENTINEL32).all())


def _guarded_floats(n, fill_words=SENTINEL32):
    """(buffer, view): a device float buffer of n elements with GUARD sentinels on both sides."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL32, dtype=torch.int32, device='cuda')
    buf[GUARD:GUARD + n] = fill_words
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _ends_intact(buf, n):
    w = buf.cpu().numpy()
    return bool((w[:GUARD] == SENTINEL32).all() and (w[GUARD + n:] == SENTINEL32).all())


def _state(L, **preset):
    assert L.lib().reid_opt_state_floats() == R.ST_FLOATS
    buf, st = _guarded_floats(R.ST_FLOATS, 0)
    for k, x in preset.items():
        st[int(k[1:])] = float(x)
    return buf, st


def _coef_tensor(coef):
    return None if coef is None else torch.tensor([coef, 123.0], device='cuda')


def _adamw(L, arena, coef_ptr, betas, step, zero_grad, state=None, eps=R.EPS, n=N_ENT):
    L.check(L.lib().reid_opt_adamw(L.ptr(arena.table), n, coef_ptr, betas[0], betas[1], eps, step, zero_grad, L.ptr(state), L.stream_ptr()))
    torch.cuda.synchronize()


def _check_adamw(arena, before, ref, zero_grad, what):
    """p / m / v of the gradient-carrying entries per element; g; the entry without a gradient; the guards.  Returns the ratios."""
    (P, M, V), (eP, eM, eV) = ref
    out = {k: arena.words(k) for k in 'pgmv'}
    r = tuple(R.ratio(arena.flat(out[k]), x, e) for k, x, e in (('p', P, eP), ('m', M, eM), ('v', V, eV)))
    assert max(r) <= 1.0, f'{what}: worst error / allowance p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}'
    for i in GRAD:
        g = arena.entry(out['g'], i).view(np.int32)
        if zero_grad:
            assert not g.any(), (what, i, 'g is +0.0 everywhere')
        else:
            assert np.array_equal(g, arena.entry(before['g'], i).view(np.int32)), (what, i, 'g is only read')
    for k in 'pgmv':
        assert np.array_equal(arena.entry(out[k], NULL).view(np.int32), arena.entry(before[k], NULL).view(np.int32)), (what, k, 'the entry without a gradient')
        assert arena.guards_intact(out[k]), (what, k)
    return r, out


# ---------------------------------------------------------------------------------------------------------- reid_opt_adamw
@pytest.mark.parametrize('t', R.STEPS)
def test_adamw_per_element(L, t):
    x = R.inputs(t)
    worst = (0.0, 0.0, 0.0)
    for betas, coef, zg in COMBOS:
        ref = R.expected(t, betas, coef)
        what = f't={t} betas={betas} coef={coef} zero_grad={zg}'
        runs = []
        for rep in range(2):
            a = Arena(x)
            ct = _coef_tensor(coef)
            _adamw(L, a, L.ptr(ct), betas, t, zg)
            r, out = _check_adamw(a, a.host0, ref, zg, what)
            runs.append(out)
            if ct is not None:
                assert ct.tolist() == [coef, 123.0]
        assert all(np.array_equal(runs[0][k], runs[1][k]) for k in 'pgmv'), (what, 'a second run gives the same bits')
        worst = tuple(max(p, q) for p, q in zip(worst, r))
        # 5e-5 / 1e-4: 1 - lr wd rounds to 1.0f, so an element with a zero gradient and a zero first moment keeps its bits
        for i in (5, 10):
            assert ENT[i][1:3] == (5e-5, 1e-4)
            still = (x['g'][i] == 0) & (x['m'][i] == 0)
            assert still.sum() >= 3
            assert np.array_equal(a.entry(out['p'], i).view(np.int32)[still], x['p'][i].view(np.int32)[still]), what
            if coef == 0.0:                                          # a zero coefficient: every gradient is zero
                z = x['m'][i] == 0
                assert np.array_equal(a.entry(out['p'], i).view(np.int32)[z], x['p'][i].view(np.int32)[z]), what
    print(f'reid_opt_adamw t={t}: worst error / allowance p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}')


@pytest.mark.parametrize('start', [0, 9, 99999])
def test_adamw_device_counter(L, start):
    """step = 0: opt_tick_kernel advances state[16] and leaves the corrections in state[17..18]; the update reads them there."""
    betas = R.BETAS[0]
    x = R.inputs(10)
    dev = Arena(x)
    sbuf, st = _state(L, s16=start, s19=5.0, s2=0.125)
    cur = {k: [dev.entry(dev.host0[k], i).copy() for i in range(N_ENT)] for k in 'pgmv'}
    worst, equal_bc = (0.0, 0.0, 0.0), 0
    lr, wd = R.per_element([e[1] for e in ENT]), R.per_element([e[2] for e in ENT])
    for tick in range(3):
        t = start + tick + 1
        host = Arena(cur)
        before = {k: dev.words(k) for k in 'pgmv'}
        assert all(np.array_equal(before[k], host.host0[k]) for k in 'pgmv')
        _adamw(L, dev, None, betas, 0, 0, state=st)
        _adamw(L, host, None, betas, t, 0)
        s = st.cpu().numpy()
        assert float(s[R.ST_STEP]) == float(t)
        c1, c2 = R.bias_corrections(betas[0], betas[1], t)
        assert abs(float(s[R.ST_BC1]) - float(c1)) <= float(np.spacing(c1)) and abs(float(s[R.ST_BC2S]) - float(c2)) <= float(np.spacing(c2))
        assert float(s[2]) == 0.125 and float(s[R.ST_BATCH]) == 5.0 and not s[[0, 1, 3, 4]].any() and not s[5:16].any()      # the rest is not written
        ref = R.adamw(R.flat(cur['p']), R.flat(cur['g']), R.flat(cur['m']), R.flat(cur['v']), None, lr, wd, betas[0], betas[1], R.EPS, t)
        what = f'device counter t={t}'
        r, out = _check_adamw(dev, before, ref, 0, what)
        _check_adamw(host, before, ref, 0, what + ' (host step)')
        if s[R.ST_BC1] == c1 and s[R.ST_BC2S] == c2:                 # the same corrections: the same bits
            equal_bc += 1
            assert all(np.array_equal(out[k], host.words(k)) for k in 'pmv'), what
        worst = tuple(max(p, q) for p, q in zip(worst, r))
        cur = {k: [dev.entry(out[k], i).copy() for i in range(N_ENT)] for k in 'pgmv'}
    assert _ends_intact(sbuf, R.ST_FLOATS)
    print(f'reid_opt_adamw device counter from {start}: worst error / allowance p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}; '
          f'corrections bit-equal to the host\'s in {equal_bc} of 3 ticks')


# ---------------------------------------------------------------------------------------------------------- reid_opt_sumsq
NAN_PAYLOAD = 0x7FC12345
PINF, NINF = 0x7F800000, -0x00800000           # int32 words of +inf and -inf


def _sumsq_clip(L, arena, fixed=0.5):
    """ws pre-filled with garbage; sumsq, then clip (not adaptive, nothing recorded) -> (state, ws words)."""
    n_ws = L.lib().reid_opt_ws_floats(N_ENT)
    assert n_ws == 2 * 128 * N_ENT
    wbuf, ws = _guarded_floats(n_ws, NAN_PAYLOAD)
    ws[1::2] = 1e30
    sbuf, st = _state(L)
    L.check(L.lib().reid_opt_sumsq(L.ptr(arena.table), N_ENT, L.ptr(ws), L.stream_ptr()))
    L.check(L.lib().reid_opt_clip(L.ptr(ws), N_ENT, L.ptr(st), 0, fixed, 0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert _ends_intact(wbuf, n_ws) and _ends_intact(sbuf, R.ST_FLOATS)
    return st.cpu().numpy(), ws.cpu().numpy(), st


def _check_sumsq(arena, before_g, s, ws, what):
    """g, count, sum and norm against sanitize_sumsq per entry; the partials of the entry without a gradient are zeros."""
    got_g = arena.words('g')
    tot, bad, allow = 0.0, 0, 0.0
    for i in GRAD:
        clean, (ss, nb), al = R.sanitize_sumsq(arena.entry(before_g, i))
        assert np.array_equal(arena.entry(got_g, i).view(np.int32), clean.view(np.int32)), (what, i)
        tot, bad, allow = tot + ss, bad + nb, allow + al
    assert np.array_equal(arena.entry(got_g, NULL).view(np.int32), arena.entry(before_g, NULL).view(np.int32)), (what, 'the entry without a gradient')
    assert arena.guards_intact(got_g), what
    for k in 'pmv':
        assert np.array_equal(arena.words(k), arena.host0[k]), (what, k, 'only g is written')
    part, badp = ws[:128 * N_ENT].reshape(N_ENT, 128), ws[128 * N_ENT:].reshape(N_ENT, 128)
    assert not part[NULL].view(np.int32).any() and not badp[NULL].view(np.int32).any(), what
    assert float(s[R.ST_BAD]) == float(bad) == float(badp.astype(np.float64).sum()), what
    if math.isinf(tot):
        assert math.isinf(float(s[R.ST_SUMSQ])) and math.isinf(float(s[R.ST_NORM])) and s[R.ST_SUMSQ] > 0 and s[R.ST_NORM] > 0, what
        return 0.0
    assert np.isfinite(ws).all(), what
    r_sum = abs(float(s[R.ST_SUMSQ]) - tot) / (allow + R.U * (tot + allow) + 2.0 ** -149)            # state[0] is rounded to fp32
    r_norm = abs(float(s[R.ST_NORM]) - math.sqrt(tot)) / R.norm_allowance(tot, allow)
    assert r_sum <= 1.0 and r_norm <= 1.0, f'{what}: error / allowance sum {r_sum:.3f} norm {r_norm:.3f}'
    return max(r_sum, r_norm)


def _planted(x):
    g = [a.view(np.int32).copy() for a in x['g']]
    idx = {e[0]: i for i, e in enumerate(ENT)}
    plan = {5: [(4, PINF)], 1025: [(7, NAN_PAYLOAD), (1024, NINF)], 517: [(3, NAN_PAYLOAD)],
            131079: [(100, PINF), (R.PASS + 1, NAN_PAYLOAD), (131078, NINF)],
            262151: [(2 * R.PASS + 1, NAN_PAYLOAD | (1 << 31) - 2 ** 32), (R.PASS + 6, NINF), (262150, PINF)]}
    for n, spots in plan.items():
        for k, w in spots:
            g[idx[n]][k] = w
    return dict(x, g=[a.view(np.float32) for a in g]), sum(len(s) for n, s in plan.items() if n != 517)


def test_sumsq_sanitises_counts_and_sums(L):
    x = R.inputs(2)
    worst = 0.0
    for name in ('as drawn', 'non-finite planted'):
        arrs, n_bad = (x, 0) if name == 'as drawn' else _planted(x)
        runs = []
        for rep in range(2):
            a = Arena(arrs)
            s, ws, _ = _sumsq_clip(L, a)
            worst = max(worst, _check_sumsq(a, a.host0['g'], s, ws, name))
            assert float(s[R.ST_BAD]) == n_bad
            want = R.clip(np.zeros(R.ST_FLOATS, np.float32), float(s[R.ST_NORM]), 0, 0, 0.5)
            assert abs(float(s[R.ST_COEF]) - float(want[R.ST_COEF])) <= 2 * R.U * float(want[R.ST_COEF]) and s[R.ST_MAXNORM] == np.float32(0.5)
            runs.append((s, ws, a.words('g')))
        assert all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(*runs)), (name, 'a second run gives the same bits')
    print(f'reid_opt_sumsq: worst error / allowance of the sum and the norm {worst:.3f}')


def test_sumsq_zero_gradient_and_overflow(L):
    x = R.inputs(2)
    zero = dict(x, g=[np.zeros_like(a) for a in x['g']])
    zero['g'][3][1] = -0.0
    a = Arena(zero)
    s, ws, _ = _sumsq_clip(L, a)
    _check_sumsq(a, a.host0['g'], s, ws, 'zero gradient')
    assert float(s[R.ST_SUMSQ]) == 0.0 and float(s[R.ST_NORM]) == 0.0 and float(s[R.ST_COEF]) == 1.0 and float(s[R.ST_BAD]) == 0.0

    # one 1e20: its square overflows fp32, the norm is inf and the coefficient exactly 0 (what clip_grad_norm_ does on fp32 tensors);
    # the AdamW call that follows reads that coefficient: p moves only by the decayed first moment
    big = dict(x, g=[a.copy() for a in x['g']])
    big['g'][6][1000] = 1e20
    a = Arena(big)
    s, ws, st = _sumsq_clip(L, a)
    _check_sumsq(a, a.host0['g'], s, ws, '1e20')
    assert math.isinf(float(s[R.ST_NORM])) and float(s[R.ST_COEF]) == 0.0 and float(s[R.ST_BAD]) == 0.0
    betas, t = R.BETAS[0], 2
    lr, wd = R.per_element([e[1] for e in ENT]), R.per_element([e[2] for e in ENT])
    ref = R.adamw(R.flat(big['p']), R.flat(big['g']), R.flat(big['m']), R.flat(big['v']), 0.0, lr, wd, betas[0], betas[1], R.EPS, t)
    m64, v64 = R.flat(big['m']).astype(np.float64), R.flat(big['v']).astype(np.float64)
    assert np.allclose(ref[0][1], m64 * float(np.float32(0.9)), rtol=1e-7, atol=0) and np.allclose(ref[0][2], v64 * float(np.float32(0.999)), rtol=1e-7, atol=0)
    before = {k: a.words(k) for k in 'pgmv'}
    _adamw(L, a, st.data_ptr() + 4 * R.ST_COEF, betas, t, 0)
    r, _ = _check_adamw(a, before, ref, 0, '1e20, coef 0')
    print(f'reid_opt_adamw after an infinite norm: worst error / allowance p {r[0]:.3f}, m {r[1]:.3f}, v {r[2]:.3f}')


# ----------------------------------------------------------------------------------------------------------- reid_opt_clip
def _clip_call(L, ws, st, k8, adaptive, fixed, record, n_bad=(2, 3)):
    """Partials whose sum is (k8 / 8)^2 exactly, spread over both entries; bad counts likewise."""
    ws.zero_()
    sq = k8 * k8
    a = sq // 3
    ws[3] = a / 64.0; ws[200] = (sq - a) / 64.0
    ws[256 + 5] = float(n_bad[0]); ws[256 + 255] = float(n_bad[1])
    L.check(L.lib().reid_opt_clip(L.ptr(ws), 2, L.ptr(st), adaptive, fixed, record, L.stream_ptr()))
    torch.cuda.synchronize()
    return st.cpu().numpy()


def _check_clip(s, want, k8, what):
    assert float(s[R.ST_SUMSQ]) == k8 * k8 / 64.0 and float(s[R.ST_NORM]) == k8 / 8.0 and float(s[R.ST_BAD]) == 5.0, what
    assert np.array_equal(s[R.ST_HCOUNT:].view(np.int32), want[R.ST_HCOUNT:].view(np.int32)), (what, 'ring, count and counters')
    mx = float(want[R.ST_MAXNORM])
    assert abs(float(s[R.ST_MAXNORM]) - mx) <= float(np.spacing(np.float32(mx))), what
    c = float(s[R.ST_MAXNORM]) / (k8 / 8.0 + float(np.float32(1e-6)))              # the formula on the device's own max_norm, in double
    if c > 1.0 + 4 * R.U:
        assert float(s[R.ST_COEF]) == 1.0, what
        return 0.0
    assert float(s[R.ST_COEF]) <= 1.0
    r = abs(float(s[R.ST_COEF]) - min(c, 1.0)) / (2 * R.U * min(c, 1.0))            # one addition, one division
    assert r <= 1.0, f'{what}: coef error / allowance {r:.3f}'
    return r


NORMS8 = [8, 16, 12, 6, 10, 24, 4, 8, 20, 14, 9] + [1] * 10 + [64] * 4          # norms in eighths: 25 of them


def test_clip_history_ring_and_clamps(L):
    """25 recorded norms: an unclamped percentile after the 11th, a tied window under the 0.5 clamp, then the clamp at 3; steps that do
    not record and steps that are not adaptive in between leave the history alone."""
    assert len(NORMS8) == 25
    wbuf, ws = _guarded_floats(L.lib().reid_opt_ws_floats(2), 0)
    sbuf, st = _state(L)
    want = np.zeros(R.ST_FLOATS, np.float32)
    seen, worst = set(), 0.0
    for i, k8 in enumerate(NORMS8):
        want = R.clip(want, k8 / 8.0, 1, 1, 0.5)
        s = _clip_call(L, ws, st, k8, 1, 0.5, 1)
        worst = max(worst, _check_clip(s, want, k8, f'recorded norm {i}'))
        assert int(s[R.ST_HCOUNT]) == i + 1 and float(s[R.ST_HIST + i % 10]) == k8 / 8.0
        mx = float(s[R.ST_MAXNORM])
        seen.add('warm' if i < 10 else 'low' if mx == 0.5 else 'high' if mx == 3.0 else 'free')
        assert (mx == 1.0) == (i < 10)
        if i in (5, 12, 20, 24):
            want = R.clip(want, 40 / 8.0, 1, 0, 0.5)                      # adaptive, not recorded
            s2 = _clip_call(L, ws, st, 40, 1, 0.5, 0)
            worst = max(worst, _check_clip(s2, want, 40, f'unrecorded step after {i}'))
            assert np.array_equal(s2[R.ST_HCOUNT:], s[R.ST_HCOUNT:]) and s2[R.ST_MAXNORM] == s[R.ST_MAXNORM]
            want = R.clip(want, 3 / 8.0, 0, 1, 0.25)                      # not adaptive: fixed_max_norm, whatever `record` says
            s3 = _clip_call(L, ws, st, 3, 0, 0.25, 1)
            worst = max(worst, _check_clip(s3, want, 3, f'fixed step after {i}'))
            assert np.array_equal(s3[R.ST_HCOUNT:], s[R.ST_HCOUNT:]) and float(s3[R.ST_MAXNORM]) == 0.25
            assert float(s3[R.ST_COEF]) < 1.0
    assert seen == {'warm', 'free', 'low', 'high'}
    assert len(set(want[R.ST_HIST:R.ST_HIST + 10].tolist())) == 2          # the last window is tied
    assert _ends_intact(wbuf, 512) and _ends_intact(sbuf, R.ST_FLOATS)
    print(f'reid_opt_clip: worst coef error / allowance {worst:.3f}')


def test_clip_device_period(L):
    """record = -3: the device's batch counter decides; the history equals that of a run the host decided for."""
    wbuf, ws = _guarded_floats(L.lib().reid_opt_ws_floats(2), 0)
    _, st_dev = _state(L)
    _, st_host = _state(L)
    want = np.zeros(R.ST_FLOATS, np.float32)
    for i, k8 in enumerate(NORMS8):
        want = R.clip(want, k8 / 8.0, 1, -3, 0.5)
        a = _clip_call(L, ws, st_dev, k8, 1, 0.5, -3)
        b = _clip_call(L, ws, st_host, k8, 1, 0.5, int(i % 3 == 0))
        _check_clip(a, want, k8, f'device period, step {i}')
        assert np.array_equal(a[:R.ST_BATCH].view(np.int32), b[:R.ST_BATCH].view(np.int32)), i
        assert float(a[R.ST_BATCH]) == i + 1 and float(b[R.ST_BATCH]) == 0.0
    assert float(a[R.ST_BATCH]) == 25.0 and float(a[R.ST_HCOUNT]) == 9.0


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_everything_untouched(L):
    lib, sp = L.lib(), L.stream_ptr()
    a = Arena(R.inputs(2))
    n_ws = lib.reid_opt_ws_floats(N_ENT)
    wbuf, ws = _guarded_floats(n_ws)
    sbuf, st = _guarded_floats(R.ST_FLOATS)
    tab, w, s, b, e = L.ptr(a.table), L.ptr(ws), L.ptr(st), R.BETAS[0], R.EPS
    nan = float('nan')
    calls = {
        'sumsq: null table': lambda: lib.reid_opt_sumsq(None, N_ENT, w, sp),
        'sumsq: null ws': lambda: lib.reid_opt_sumsq(tab, N_ENT, None, sp),
        'sumsq: n_entries 0': lambda: lib.reid_opt_sumsq(tab, 0, w, sp),
        'sumsq: n_entries -1': lambda: lib.reid_opt_sumsq(tab, -1, w, sp),
        'sumsq: n_entries 65536': lambda: lib.reid_opt_sumsq(tab, 65536, w, sp),
        'clip: null ws': lambda: lib.reid_opt_clip(None, N_ENT, s, 1, 0.5, 1, sp),
        'clip: null state': lambda: lib.reid_opt_clip(w, N_ENT, None, 1, 0.5, 1, sp),
        'clip: n_entries 0': lambda: lib.reid_opt_clip(w, 0, s, 1, 0.5, 1, sp),
        'clip: n_entries 65536': lambda: lib.reid_opt_clip(w, 65536, s, 1, 0.5, 1, sp),
        'clip: max_norm 0': lambda: lib.reid_opt_clip(w, N_ENT, s, 0, 0.0, 1, sp),
        'clip: max_norm -1': lambda: lib.reid_opt_clip(w, N_ENT, s, 1, -1.0, 1, sp),
        'clip: max_norm NaN': lambda: lib.reid_opt_clip(w, N_ENT, s, 0, nan, 1, sp),
        'adamw: null table': lambda: lib.reid_opt_adamw(None, N_ENT, None, b[0], b[1], e, 1, 1, s, sp),
        'adamw: n_entries 0': lambda: lib.reid_opt_adamw(tab, 0, None, b[0], b[1], e, 1, 1, s, sp),
        'adamw: n_entries 65536': lambda: lib.reid_opt_adamw(tab, 65536, None, b[0], b[1], e, 1, 1, s, sp),
        'adamw: beta1 1': lambda: lib.reid_opt_adamw(tab, N_ENT, None, 1.0, b[1], e, 1, 1, s, sp),
        'adamw: beta1 < 0': lambda: lib.reid_opt_adamw(tab, N_ENT, None, -0.1, b[1], e, 1, 1, s, sp),
        'adamw: beta2 1': lambda: lib.reid_opt_adamw(tab, N_ENT, None, b[0], 1.0, e, 1, 1, s, sp),
        'adamw: beta2 NaN': lambda: lib.reid_opt_adamw(tab, N_ENT, None, b[0], nan, e, 1, 1, s, sp),
        'adamw: eps 0': lambda: lib.reid_opt_adamw(tab, N_ENT, None, b[0], b[1], 0.0, 1, 1, s, sp),
        'adamw: eps < 0': lambda: lib.reid_opt_adamw(tab, N_ENT, None, b[0], b[1], -1e-8, 1, 1, s, sp),
        'adamw: step -1': lambda: lib.reid_opt_adamw(tab, N_ENT, None, b[0], b[1], e, -1, 1, s, sp),
        'adamw: step 0 without state': lambda: lib.reid_opt_adamw(tab, N_ENT, None, b[0], b[1], e, 0, 1, None, sp),
    }
    for name, call in calls.items():
        with pytest.raises(L.ReidHipError):
            L.check(call())
        torch.cuda.synchronize()
        assert L.lib().reid_last_error(), name
        for k in 'pgmv':
            assert np.array_equal(a.words(k), a.host0[k]), (name, k)
        assert bool((wbuf == SENTINEL32).all()) and bool((sbuf == SENTINEL32).all()), name
