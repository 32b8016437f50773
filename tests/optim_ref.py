"""Plain fp64 reference of the fused optimizer (csrc/optim.hip: reid_opt_sumsq, reid_opt_clip, reid_opt_adamw) with an allowance per
output element, the seeded inputs of tests/test_optim_exact_gpu.py, and float32 restatements (straight and mutated) that
tests/test_optim_ref_cpu.py uses to show that the allowances accept a correct kernel and reject a wrong one.

Conventions: u = 2^-24 is the fp32 unit roundoff, TINY = 2^-126 the smallest normal.  Every fp32 operation returns its exact result
times (1 + d), |d| <= u, or -- where the result is subnormal, or a build flushes subnormals to zero -- within TINY of it.  An
operation therefore adds u * |result| + TINY to the error its operands carry; the operands' errors are carried through the operation
exactly (product rule with the cross term, quotient with the perturbed denominator, |sqrt a - sqrt b| <= min(|a - b| / sqrt a,
sqrt |a - b|)).  A compiler that contracts a product and a sum into one fused multiply-add only removes a rounding, so the bounds hold
for contracted and uncontracted code alike.  Nothing here is fitted to what a GPU returned, and nothing reads a compiled reference.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
PASS = 128 * 256 * 4            # elements one grid-stride pass covers: 128 workgroups x 256 threads x 4 floats
EPS = 1e-8
F = np.float32


def _f(x):
    """The double that equals float32(x): what a kernel receives for a float argument."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------ sumsq
def sanitize_sumsq(g32):
    """-> (g', (sumsq, n_bad), allowance).

    g' is a float32 copy of g with every non-finite entry (NaN of any payload, +inf, -inf) set to +0.0 and every other entry
    bit-identical: -0.0 and denormals are finite.  sumsq is the float64 sum of the squares ROUNDED TO FLOAT32, the semantics of the
    kernel and of torch.nn.utils.clip_grad_norm_ on fp32 tensors: a square that overflows fp32 (|g| > 1.84e19) is +inf and makes the
    sum +inf, a square that underflows contributes what fp32 gives (a denormal, or 0 below 2^-150).  n_bad counts the replaced entries.

    The allowance covers the kernel's fp32 accumulation: a term travels through at most the chain of one thread, four fused
    multiply-adds per grid-stride pass, ceil(n / 131072) passes, then six shuffle levels and two additions across the four waves --
    ceil(n / 131072) * 4 + 8 roundings, each of at most u times a partial sum of non-negative terms, which the total bounds.  The sum of
    the workgroups' partials is formed in double and adds nothing.  n * TINY more covers squares in the subnormal range (a fused
    multiply-add does not round the square on its own, a build that flushes them drops them).  An infinite sum has an infinite
    allowance: compare it with `==`."""
    g = np.array(g32, dtype=np.float32, copy=True)
    bad = ~np.isfinite(g)
    g[bad] = F(0.0)
    with np.errstate(over='ignore', under='ignore'):
        sq = np.multiply(g, g, dtype=np.float32)
    s = float(sq.astype(np.float64).sum())
    chain = math.ceil(g.size / PASS) * 4 + 8
    allow = chain * U * s + g.size * TINY if math.isfinite(s) else math.inf
    return g, (s, int(bad.sum())), allow


def norm_allowance(sumsq, allow):
    """Allowance of float32(sqrt(sumsq')) for |sumsq' - sumsq| <= allow: the square root's own bound plus the one rounding to fp32 (the
    double sqrt is exact to 2^-53)."""
    if not math.isfinite(sumsq):
        return math.inf
    n = math.sqrt(sumsq)
    d = min(allow / n, math.sqrt(allow)) if n > 0 else math.sqrt(allow)
    return d + U * (n + d) + 2.0 ** -149


# ------------------------------------------------------------------------------------------------------------------- clip
ST_SUMSQ, ST_NORM, ST_COEF, ST_MAXNORM, ST_BAD, ST_HCOUNT, ST_HIST = 0, 1, 2, 3, 4, 5, 6        # the device state (csrc/optim.hip)
ST_STEP, ST_BC1, ST_BC2S, ST_BATCH, ST_FLOATS = 16, 17, 18, 19, 20


def clip_coef(norm32, max_norm32):
    """min(1, max_norm / (norm + 1e-6)) with the sum and the quotient each rounded to float32 (torch.nn.utils.clip_grad_norm_)."""
    with np.errstate(over='ignore', under='ignore', divide='ignore'):
        c = F(max_norm32) / (F(norm32) + F(1e-6))
    return F(1.0) if c > F(1.0) else F(c)


def clip(state, norm, adaptive, record, fixed):
    """The 20-float device state after reid_opt_clip saw the gradient norm `norm` (a double; the state stores float32(norm)).

    record < 0 is the device period: the batch counter state[19] is read, incremented, and the norm is recorded when the value read is
    a multiple of -record.  With `adaptive`, a recorded norm goes to slot count % 10 of the history ring state[6..15] and the count
    state[5] grows by one; once MORE THAN ten norms were recorded max_norm = clamp(np.percentile(last ten, 70) * 1.15, 0.5, 3), before
    that 1.0.  Without `adaptive` max_norm = fixed and the history is left alone.  state[1] = norm, state[3] = max_norm, state[2] =
    clip_coef.  state[0] and state[4] (the sum of squares and the non-finite count) are the caller's."""
    st = np.array(state, dtype=np.float32, copy=True)
    assert st.size == ST_FLOATS
    with np.errstate(over='ignore'):
        nf = F(norm)
    mx = F(fixed)
    if record < 0:
        bi = int(st[ST_BATCH])
        st[ST_BATCH] = F(bi + 1)
        record = int(bi % (-record) == 0)
    if adaptive:
        cnt = int(st[ST_HCOUNT])
        if record:
            st[ST_HIST + cnt % 10] = nf
            cnt += 1
            st[ST_HCOUNT] = F(cnt)
        if cnt > 10:
            p70 = float(np.percentile(st[ST_HIST:ST_HIST + 10].astype(np.float64), 70))
            mx = F(min(3.0, max(0.5, p70 * 1.15)))
        else:
            mx = F(1.0)
    st[ST_NORM], st[ST_MAXNORM], st[ST_COEF] = nf, mx, clip_coef(nf, mx)
    return st


# ------------------------------------------------------------------------------------------------------------------ adamw
class _E:
    """A float64 value array with a bound on the error of its fp32 evaluation."""
    __slots__ = ('x', 'e')

    def __init__(self, x, e=0.0):
        self.x = np.asarray(x, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.x.shape)


def _rounded(x, e):
    return _E(x, e + U * (np.abs(x) + e) + TINY)


def _mul(a, b):
    return _rounded(a.x * b.x, np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e)


def _add(a, b, sign=1.0):
    return _rounded(a.x + sign * b.x, a.e + b.e)


def _div(a, b):
    q = a.x / b.x
    room = np.abs(b.x) - b.e
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.where(room > 0, (a.e + np.abs(q) * b.e) / np.where(room > 0, room, 1.0), np.inf)
    return _rounded(q, e)


def _sqrt(a):
    r = np.sqrt(a.x)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.minimum(np.where(r > 0, a.e / np.where(r > 0, r, 1.0), np.inf), np.sqrt(a.e))
    return _rounded(r, e)


def bias_corrections(beta1, beta2, t):
    """(float32(1 - beta1^t), float32(sqrt(1 - beta2^t))) from float64 arithmetic on the float32 betas."""
    return F(1.0 - _f(beta1) ** t), F(math.sqrt(1.0 - _f(beta2) ** t))


def adamw(p, g, m, v, coef, lr, wd, beta1, beta2, eps, t, round_bc=True):
    """-> ((p', m', v'), (ep, em, ev)): one AdamW step in float64 from fp32 inputs, in the order of adamw_one (csrc/optim.hip), which is
    torch's single-tensor AdamW, and for each output element a bound on what an fp32 evaluation of the same expressions may differ by.

        G  = g * coef                                      1 operation
        p1 = p * (1 - lr * wd)                             3
        m' = m + (G - m) * (1 - beta1)                     4
        v' = v * beta2 + ((1 - beta2) * G) * G             5
        d  = sqrt(v') / bc2 + eps                          3
        p' = p1 - (lr / bc1) * (m' / d)                    4

    Derivation.  Each operation adds u |result| + TINY (module docstring) to the error carried by its operands, so a plain sum of k
    rounded terms carries at most k u sum|terms| and the errors of G, m' and v' reach p' through (lr / bc1) m' / d with their first
    derivatives: |d m'| (lr / bc1) / d for the first moment, |step| |d d| / d for the denominator, where |d sqrt(v')| <= |d v'| / sqrt(v')
    and never more than sqrt|d v'| (so a v' that underflowed cannot blow the bound up).  The code below carries these terms operation by
    operation instead of in closed form, including the second-order cross terms, so it is a bound and not an estimate.  lr, wd, the
    betas and eps are the float32 values the kernel receives; lr and wd may be arrays (one value per element).  The bias corrections
    are float32(1 - beta1^t) and float32(sqrt(1 - beta2^t)) evaluated in float64; the device evaluates pow itself, so one fp32 ulp is
    allowed on each (`round_bc=False` keeps them in float64 with no allowance: the form torch.optim.AdamW computes on the host).
    coef None means the kernel's "no coefficient": G = g exactly."""
    p, g, m, v = (_E(np.asarray(a, dtype=np.float64)) for a in (p, g, m, v))
    lr_, wd_ = _E(np.asarray(lr, dtype=np.float32)), _E(np.asarray(wd, dtype=np.float32))
    b1, b2, one = _E(_f(beta1)), _E(_f(beta2)), _E(1.0)
    G = g if coef is None else _mul(g, _E(_f(coef)))
    p1 = _mul(p, _add(one, _mul(lr_, wd_), -1.0))
    M = _add(m, _mul(_add(G, m, -1.0), _add(one, b1, -1.0)))
    V = _add(_mul(v, b2), _mul(_mul(_add(one, b2, -1.0), G), G))
    if round_bc:
        c1, c2 = bias_corrections(beta1, beta2, t)
        bc1, bc2 = _E(float(c1), float(np.spacing(c1))), _E(float(c2), float(np.spacing(c2)))
    else:
        bc1, bc2 = _E(1.0 - _f(beta1) ** t), _E(math.sqrt(1.0 - _f(beta2) ** t))
    d = _add(_div(_sqrt(V), bc2), _E(_f(eps)))
    P = _add(p1, _mul(_div(lr_, bc1), _div(M, d)), -1.0)
    return (P.x, M.x, V.x), (P.e, M.e, V.e)


def ratio(got, ref, allow):
    """Worst |got - ref| / allow over the elements; a NaN or an infinity in `got` counts as infinitely wrong."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.abs(got - ref) / allow
    r = np.where(np.isfinite(got), r, np.inf)
    return float(np.max(r))


# ------------------------------------------------------------------------------------- float32 restatements and their mutants
VARIANTS = ('coef_ignored', 'coef_m_only', 'no_eps', 'eps_in_sqrt', 'bc_swapped')


def adamw_f32(p, g, m, v, coef, lr, wd, beta1, beta2, eps, t, fused=False, variant=None):
    """The same step with every operation rounded to float32 (numpy never fuses), or with `fused` the lerp, the addcmul and the final
    update as fused multiply-adds (float64 product and sum, rounded once).  `variant` (VARIANTS) breaks the formula on purpose."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    lr, wd = np.asarray(lr, dtype=np.float32), np.asarray(wd, dtype=np.float32)
    one, b1, b2, eps = F(1.0), F(beta1), F(beta2), F(eps)
    d64 = lambda a: np.asarray(a, dtype=np.float64)
    with np.errstate(all='ignore'):
        G = g if coef is None else g * F(coef)
        gm = g if variant == 'coef_ignored' else G
        gv = g if variant in ('coef_ignored', 'coef_m_only') else G
        c1, c2 = one - b1, one - b2
        bc1, bc2 = bias_corrections(beta1, beta2, t)
        if variant == 'bc_swapped':
            bc1, bc2 = bc2, bc1
        if fused:
            w = (1.0 - d64(lr) * d64(wd)).astype(np.float32)
            p1 = p * w
            M = (d64(m) + d64(gm - m) * float(c1)).astype(np.float32)
            V = (d64(v) * float(b2) + d64(c2 * gv) * d64(gv)).astype(np.float32)
        else:
            p1 = p * (one - lr * wd)
            M = m + (gm - m) * c1
            V = v * b2 + (c2 * gv) * gv
        if variant == 'no_eps':
            den = np.sqrt(V) / bc2
        elif variant == 'eps_in_sqrt':
            den = np.sqrt(V + eps) / bc2
        else:
            den = np.sqrt(V) / bc2 + eps
        a, b = lr / bc1, M / den
        P = (d64(p1) - d64(a) * d64(b)).astype(np.float32) if fused else p1 - a * b
    return P, M, V


# --------------------------------------------------------------------------------------------------------------------- inputs
# (n, lr, weight_decay, has a gradient).  Powers of two make 1 - lr * wd exact and far from 1; a wd = 0 entry sits next to entries
# that decay; every lr is distinct among the power-of-two entries; 5e-5 / 1e-4 and 3e-3 / 1e-4 are the project's own pairs (for the first
# 1 - lr * wd rounds to 1.0f).  The entry without a gradient sits in the middle of the table.
ENTRIES = (
    (1, 2.0 ** -6, 2.0 ** -3, True), (2, 2.0 ** -7, 0.0, True), (3, 2.0 ** -5, 2.0 ** -3, True), (4, 2.0 ** -8, 2.0 ** -2, True),
    (5, 2.0 ** -4, 2.0 ** -3, True), (1023, 5e-5, 1e-4, True), (1024, 3e-3, 1e-4, True), (1025, 2.0 ** -9, 0.0, True),
    (517, 2.0 ** -3, 2.0 ** -1, False),
    (131072, 2.0 ** -11, 2.0 ** -1, True), (131079, 5e-5, 1e-4, True), (262151, 2.0 ** -10, 2.0 ** -3, True),
)
SIZES = tuple(e[0] for e in ENTRIES if e[3])
STEPS = (1, 2, 10, 1000, 100000)          # t = 1 starts from zero moments, the others from a mid-training state
BETAS = ((0.9, 0.999), (0.5, 0.75))
SPECIALS = np.array([0.0, -0.0, 1e-40, 1e-25, -1e-25, -3e-42, 0.0], dtype=np.float32)      # zeros, denormals, squares that underflow


def _loguniform(rng, n):
    return (10.0 ** rng.uniform(-12.0, 4.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _gradient(rng, n):
    g = _loguniform(rng, n)
    if n >= 64:
        pos = list(np.linspace(0, n - 1, 28).astype(np.int64))            # first vector, body, the last element (the scalar tail)
        pos += [k * PASS + j for k in range(1, n // PASS + 1) for j in (1, 2) if k * PASS + j < n]      # later grid-stride passes
        pos = np.unique(pos)
    else:
        pos = np.arange(1, n, 2)
    g[pos] = SPECIALS[np.arange(pos.size) % SPECIALS.size]
    return g


@functools.lru_cache(maxsize=None)
def inputs(t):
    """Per table entry: p standard normal; g of magnitude log-uniform over 1e-12 .. 1e4 and both signs with SPECIALS planted;
    t == 1: zero moments, else m like g and v log-uniform over the same range, and m = 0 at every second zero gradient."""
    rng = np.random.default_rng(7700 + t)
    out = dict(p=[], g=[], m=[], v=[])
    for n, lr, wd, has_g in ENTRIES:
        p = rng.standard_normal(n).astype(np.float32)
        g = _gradient(rng, n)
        if t == 1:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            m, v = _loguniform(rng, n), np.abs(_loguniform(rng, n))
            m[np.flatnonzero(g == 0)[::2]] = 0.0
        for k, a in zip('pgmv', (p, g, m, v)):
            a.setflags(write=False)
            out[k].append(a)
    return out


def per_element(values):
    """One float32 value per element of the concatenated gradient-carrying entries."""
    return np.concatenate([np.full(e[0], x, dtype=np.float32) for e, x in zip(ENTRIES, values) if e[3]])


def flat(arrs):
    """The gradient-carrying entries of a per-entry list, concatenated."""
    return np.concatenate([a for e, a in zip(ENTRIES, arrs) if e[3]])


def split(a):
    """Inverse of flat: per gradient-carrying entry."""
    out, o = [], 0
    for n in SIZES:
        out.append(a[o:o + n]); o += n
    return out


@functools.lru_cache(maxsize=8)
def expected(t, betas, coef):
    """adamw() on inputs(t), all gradient-carrying entries concatenated: ((P, M, V), (eP, eM, eV))."""
    x = inputs(t)
    lr, wd = per_element([e[1] for e in ENTRIES]), per_element([e[2] for e in ENTRIES])
    return adamw(flat(x['p']), flat(x['g']), flat(x['m']), flat(x['v']), coef, lr, wd, betas[0], betas[1], EPS, t)
