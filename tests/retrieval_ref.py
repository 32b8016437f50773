"""fp64 restatement of the cosine top-k contract (include/reid_hip.h, csrc/retrieval.hip) and the fixtures of
test_retrieval_exact_gpu.py.  Everything here runs on the CPU in float64; test_retrieval_ref_cpu.py checks that the fixtures hold the
ties, clusters and gaps they claim.

The contract: sim = Q . G^T; entries with exq[q] >= 0 and exq[q] == exg[g] are set to exactly -1e9 (the reference's
masked_fill(-1e9)); the list of a query is the first k of the order (score descending, index ascending) -- a stable descending
argsort.  Excluded rows stay in the ranking, last, with score float32(-1e9), in index order.

Exact fixtures: operands are integers in [-4, 4] times 2^e, e = -round(log2(sqrt(20/3 D))) (row norms 0.7 .. 1.3), representable in
bf16 and f16.  Every product is a multiple of 2^2e and the absolute sum of a row's products is at most 16 D quanta < 2^24, so every
16-bit score, fp32 score and partial sum is exact in any order: the expected indices AND the expected score bits are unique.

Rounded fixture: unit fp32 rows; the fp32 score of csrc/retrieval.hip's row_dot passes a term through n = 4 ceil(D / 256) + 6 roundings
(3 fma/add steps of dot4_acc + 1 accumulate per 256 columns, 6 butterfly levels) plus the final add, so
|score - fp64| <= b = (n + 1) 2^-24 sum_i |Q[q, i] G[g, i]|.  Seeds are chosen (ROUNDED_SEEDS, searched on the CPU with
find_rounded_seed) so that in every query's fp64 top k + 1 each adjacent gap is 0 between bit-identical rows or > 2 b: the list is then
unique under that bound."""
import functools
import math

import numpy as np

# ---- constants and dispatch of csrc/retrieval.hip, restated ------------------------------------------------------------------------
SAMPLE = 8192                      # rows of the threshold sample (tiled path)
SELECT_SV = 512                    # survivors select_fast_kernel can hold; more: the query is flagged
SELECT_FAST_K_MAX = 32             # select_fast_kernel up to here (unless knob TOPK_TILE = 9), select_kernel beyond
SCAN_NQ_MAX, SCAN_KG, SCAN_CNT_STRIDE = 128, 16, 32
SCAN_WS = (SCAN_NQ_MAX * SCAN_CNT_STRIDE + 4 * SCAN_KG * 32) * 4      # counters + group maxima, carved out of the sample area of ws
STREAM_SQ, STREAM_K_MAX, STREAM_LIST_BUDGET = 4, 32, 16384
EXCLUDED = float(np.float32(-1e9))                                     # (exactly representable: 1e9 = 2^9 * 1953125)
EPS16 = {'bf16': 2.0 ** -8 * 1.01, 'f16': 2.0 ** -10 * 1.01}            # EPS_BF16 = REID_T16_EPS * 1.01f; the filter margin is 2 EPS


def cap_for(Ng, k):
    """Candidate-list capacity per query: 6 k ceil(Ng / SAMPLE) + 64, clamped to [256, 8192]."""
    return int(min(max(6 * k * ((Ng + SAMPLE - 1) // SAMPLE) + 64, 256), 8192))


def topk_ws_bytes(Nq, Ng, k):
    """thr[Nq] | cnt[Nq] | cand_idx[Nq cap] | cand_score[Nq cap] | dense[Nq min(Ng, SAMPLE)] | 256."""
    return Nq * 8 + Nq * cap_for(Ng, k) * 8 + Nq * min(Ng, SAMPLE) * 4 + 256


def scan_ok(Nq, Ng, D, k, cus):
    """reid_topk_scan_ok with the knob at its default; cus = compute units of the device."""
    if not (1 <= Nq <= SCAN_NQ_MAX and 1 <= k <= SCAN_KG and k <= Ng and D in (256, 512)):
        return False
    cus = max(cus & ~7, 8)
    grid = min((Ng + 63) // 64, cus)
    return grid >= 4 * k and Nq * min(Ng, SAMPLE) * 4 >= SCAN_WS


def stream_ok(Nq, Ng, D, k):
    return 1 <= Nq <= STREAM_SQ and 1 <= k <= STREAM_K_MAX and k <= Ng and D % 256 == 0 and 256 <= D <= 1024


def filter_tile(Nq, Ng):
    """Tile of the tiled filter pass (reid_cosine_topk, phase B)."""
    if Nq <= 64 and Ng >= 1024:
        return '64x256'
    return '128x128' if Nq < 256 or Ng < 1024 else '128x256'


def kth_form(k):
    return 'kth_fast<2>' if k <= 32 else 'kth_fast<4>' if k <= 128 else 'kth_kernel'


def stream_merge_in_lds(Nq, Ng, k):
    groups = min(STREAM_LIST_BUDGET // k, 1024)
    if Nq == 1:
        groups = min(groups, 512)
    groups = min(groups, (Ng + 15) // 16)
    n = groups * k
    return ((n + 3) & ~3) * 8 + min(16 * k * k + 64, n) * 8 <= 160 * 1024 - 64


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def similarity(Q64, G64, exq=None, exg=None):
    sim = np.asarray(Q64, np.float64) @ np.asarray(G64, np.float64).T
    if exq is not None and exg is not None:
        eq, eg = np.asarray(exq).reshape(-1, 1), np.asarray(exg).reshape(1, -1)
        sim[(eq >= 0) & (eq == eg)] = EXCLUDED
    return sim


def ranking(Q64, G64, exq, exg, k):
    """(idx int32 [Nq, k], score float64 [Nq, k]): the first k of (score descending, index ascending)."""
    sim = similarity(Q64, G64, exq, exg)
    Nq, Ng = sim.shape
    assert 1 <= k <= Ng
    idx = np.empty((Nq, k), np.int32)
    score = np.empty((Nq, k), np.float64)
    for q in range(Nq):
        row = sim[q]
        kth = np.partition(row, Ng - k)[Ng - k]                        # the k-th largest value
        cand = np.flatnonzero(row >= kth)                              # ascending indices
        order = cand[np.lexsort((cand, -row[cand]))][:k]
        idx[q], score[q] = order, row[order] + 0.0                     # (+ 0.0: a zero score is +0, as s = 0.f + ... in the kernels)
    return idx, score


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def score_bound(Q64, G64, idx, D):
    """b[q, r] = (n + 1) 2^-24 sum_i |Q[q, i] G[idx[q, r], i]| with n = 4 ceil(D / 256) + 6 (module docstring)."""
    n = 4 * ((D + 255) // 256) + 6
    Q, G = np.abs(np.asarray(Q64, np.float64)), np.abs(np.asarray(G64, np.float64))
    return (n + 1) * 2.0 ** -24 * np.einsum('qd,qrd->qr', Q, G[np.asarray(idx, np.int64)])


# ---- exact fixtures ----------------------------------------------------------------------------------------------------------------
def lattice_exp(D):
    return -int(round(math.log2(math.sqrt(20.0 / 3.0 * D))))


TIE_KINDS = ('tie2', 'tieK5', 'tie65', 'tie513', 'tieCap')
MUST_POSITIONS = (3, 37, 70, SAMPLE - 1, SAMPLE, SAMPLE + 299)       # tile 0 / tile 1 / chunk 1 / both sides of the sample's end


def tie_size(kind, Ng, k):
    return {'tie2': 2, 'tieK5': k + 5, 'tie65': 65, 'tie513': SELECT_SV + 1, 'tieCap': cap_for(Ng, k) + 1}[kind]


class Fixture:
    """Q, G float64 [.., D]; exq / exg int32 or None; idx / score: the expected lists; kind[q]: what was planted for query q."""

    def quantum(self):
        return 2.0 ** (2 * self.exp)

    def must_flag(self, fast):
        """Queries every batched raw path must flag: a tie group beyond the candidate capacity, the all-zero query when the gallery
        exceeds it; with select_fast_kernel also the group beyond its SELECT_SV survivors."""
        cap = cap_for(self.Ng, self.k)
        out = [q for q, kd in enumerate(self.kind) if kd == 'tieCap' or (kd == 'zero' and self.Ng > cap) or (fast and kd == 'tie513')]
        return np.array(out, np.int64)

    def tied_with_kth(self, q):
        """Indices of ALL gallery rows whose score equals the k-th score of query q (empty unless the (k+1)-th ties too)."""
        row = similarity(self.Q[q:q + 1], self.G, None if self.exq is None else self.exq[q:q + 1], self.exg)[0]
        tied = np.flatnonzero(row == self.score[q, self.k - 1])
        above = int((row > self.score[q, self.k - 1]).sum())
        return tied if above + len(tied) > self.k else tied[:0]


@functools.lru_cache(maxsize=None)
def exact_fixture(Nq, Ng, D, k, seed=0, excl='main', neg=False, first=0):
    """See the module docstring.  excl: None | 'main' (sparse ids: one query loses its best three rows, one loses a random 5 %, one has
    an id nobody shares, -1 on both sides everywhere else) | 'dense' (all but min(k - 1, 5) rows share id 9: the query with id 9 has fewer
    than k usable rows) | 'all' (every gallery row has id 4, so has one query).  neg: gallery entries >= 0 and one query <= 0.
    first: index of the first planted query (the planted queries are first .. first + n - 1)."""
    rng = np.random.default_rng([seed, Nq, Ng, D, k])
    e = lattice_exp(D)
    G = rng.integers(0 if neg else -4, 5, (Ng, D)).astype(np.float64) * 2.0 ** e
    Q = rng.integers(-4, 5, (Nq, D)).astype(np.float64) * 2.0 ** e
    cap = cap_for(Ng, k)
    ties = [t for t in TIE_KINDS if tie_size(t, Ng, k) + 16 <= Ng]     # (none in a gallery of a few rows)
    ties = ties[seed % max(len(ties), 1):] + ties[:seed % max(len(ties), 1)]
    room, fit = Ng - 64 - k, []                                        # all groups together leave rows of the lattice
    for t in ties:
        if tie_size(t, Ng, k) <= room:
            fit.append(t); room -= tie_size(t, Ng, k)
    ties = fit
    others = ['zero'] + (['neg'] if neg else []) + ([] if neg or Ng < SAMPLE + 2 * k + 16 else ['far', 'near'])
    others += {'main': ['ex3', 'exPart', 'exAlone'], 'dense': ['exFew', 'ex7'], 'all': ['exAll'], None: []}[excl]
    rot = seed % len(others)
    plan = ties[:1] + others[rot:] + others[:rot] + ties[1:]
    kind = ['plain'] * Nq
    for j, kd in enumerate(plan[:max(0, Nq - first)]):
        kind[first + j] = kd
    used = set()
    free_order = rng.permutation(Ng)

    def take(n, lo=0, hi=Ng, prefer=()):
        out = [p for p in dict.fromkeys(prefer) if lo <= p < hi and p not in used][:n]
        used.update(out)
        for p in free_order:
            if len(out) >= n:
                break
            if lo <= p < hi and p not in used:
                out.append(int(p)); used.add(int(p))
        assert len(out) == n
        return out

    for q, kd in enumerate(kind):
        if kd == 'zero':
            Q[q] = 0.0
        elif kd == 'neg':
            Q[q] = -rng.integers(1, 5, D).astype(np.float64) * 2.0 ** e
    # (the largest groups first: a group of m <= k rows must find the ranks above it settled)
    for q, kd in sorted(enumerate(kind), key=lambda t: -tie_size(t[1], Ng, k) if t[1] in TIE_KINDS else -Ng):
        if kd in TIE_KINDS:                                           # copies of the row at rank max(1, k - m + 2): ranks k and k + 1 tie
            m = tie_size(kd, Ng, k)
            j = max(1, k - m + 2)
            src = int(ranking(Q[q:q + 1], G, None, None, j)[0][0, j - 1])
            used.add(src)
            G[take(m - 1, prefer=(Ng - 1,) + MUST_POSITIONS)] = G[src]
        elif kd in ('far', 'near'):                                   # the whole top k beyond / inside the sample: q with j entries cleared
            lo, hi = (SAMPLE, Ng) if kd == 'far' else (0, SAMPLE)
            for j, p in enumerate(take(k, lo, hi)):
                G[p] = Q[q]
                G[p, :j] = 0.0
    exq = exg = None
    if excl == 'main':
        exq, exg = np.full(Nq, -1, np.int32), np.full(Ng, -1, np.int32)
        exg[rng.random(Ng) < 0.05] = 11
        for q, kd in enumerate(kind):
            if kd == 'ex3':
                exq[q] = 7
            elif kd == 'exPart':
                exq[q] = 11
            elif kd == 'exAlone':
                exq[q] = 5
        for q in np.flatnonzero(exq == 7):
            exg[ranking(Q[q:q + 1], G, None, None, min(3, Ng))[0][0]] = 7
    elif excl == 'dense':
        exq, exg = np.full(Nq, -1, np.int32), np.full(Ng, 9, np.int32)
        free = take(min(k - 1, 5))
        exg[free] = [(-1, 7)[i & 1] for i in range(len(free))]
        for q, kd in enumerate(kind):
            exq[q] = {'exFew': 9, 'ex7': 7}.get(kd, -1)
    elif excl == 'all':
        exq, exg = np.full(Nq, -1, np.int32), np.full(Ng, 4, np.int32)
        for q, kd in enumerate(kind):
            if kd == 'exAll':
                exq[q] = 4
    fx = Fixture()
    fx.Nq, fx.Ng, fx.D, fx.k, fx.exp, fx.excl, fx.neg, fx.exact = Nq, Ng, D, k, e, excl, neg, True
    fx.Q, fx.G, fx.exq, fx.exg, fx.kind = Q, G, exq, exg, kind
    fx.idx, fx.score = ranking(Q, G, exq, exg, k)
    for a in (fx.Q, fx.G, fx.idx, fx.score):
        a.setflags(write=False)
    return fx


# ---- rounded fixture -----------------------------------------------------------------------------------------------------------------
CLUSTERS = (3000, 150)          # near-duplicates around queries 0 and 1: beyond every candidate capacity used / inside the smallest (256)
ROUNDED_SEEDS = {(8, 9001, 512, 10): 3, (8, 9001, 256, 10): 2}      # (Nq, Ng, D, k) -> seed; see find_rounded_seed


def _unit32(x):
    x = x.astype(np.float32)
    return (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


def gaps_ok(Q, G, k):
    """The uniqueness condition of the module docstring on the fp64 top k + 1 of every query."""
    idx, sc = ranking(Q, G, None, None, min(k + 1, G.shape[0]))
    b = score_bound(Q, G, idx, Q.shape[1])
    gap = sc[:, :-1] - sc[:, 1:]
    same = (G[idx[:, :-1]] == G[idx[:, 1:]]).all(-1)
    return bool(np.all(np.where(same, gap == 0, gap > 2 * np.maximum(b[:, :-1], b[:, 1:]))))


def _rounded_arrays(Nq, Ng, D, k, seed):
    rng = np.random.default_rng([seed, Nq, Ng, D, k, 77])
    Q = _unit32(rng.standard_normal((Nq, D)))
    G = _unit32(rng.standard_normal((Ng, D)))
    sigma = 0.1 / math.sqrt(D)                                        # |delta|^2 ~ 0.01: scores 0.995 +- 3e-4 (D = 512) .. 4e-4 (D = 256)
    where = rng.permutation(Ng - 1)
    at = 0
    for q, n in enumerate(CLUSTERS):
        rows = where[at:at + n]; at += n
        G[rows] = _unit32(Q[q].astype(np.float64) + sigma * rng.standard_normal((n, D)))
    Q, G = Q.astype(np.float64), G.astype(np.float64)
    G[Ng - 1] = G[ranking(Q[2:3], G, None, None, 1)[0][0, 0]]          # one bit-identical pair: query 2's best row again, in the ragged tail
    return Q, G


@functools.lru_cache(maxsize=None)
def rounded_fixture(Nq, Ng, D, k):
    Q, G = _rounded_arrays(Nq, Ng, D, k, ROUNDED_SEEDS[(Nq, Ng, D, k)])
    fx = Fixture()
    fx.Nq, fx.Ng, fx.D, fx.k, fx.excl, fx.neg, fx.exact = Nq, Ng, D, k, None, False, False
    fx.Q, fx.G, fx.exq, fx.exg = Q, G, None, None
    fx.kind = ['cluster', 'cluster', 'twin'] + ['plain'] * (Nq - 3)
    fx.idx, fx.score = ranking(Q, G, None, None, k)
    fx.bound = score_bound(Q, G, fx.idx, D)
    for a in (fx.Q, fx.G, fx.idx, fx.score, fx.bound):
        a.setflags(write=False)
    return fx


def find_rounded_seed(Nq, Ng, D, k, tries=64):
    """The first seed whose arrays meet gaps_ok (how ROUNDED_SEEDS was filled)."""
    for seed in range(tries):
        if gaps_ok(*_rounded_arrays(Nq, Ng, D, k, seed), k):
            return seed
    raise AssertionError('no seed found')


# ---- what the tiled path keeps (exact fixtures only: their 16-bit scores ARE the scores) ----------------------------------------------------
def tiled_candidates(fx, q, flavor):
    """Number of candidates the sample / threshold / filter launches keep for query q: the threshold kernels restated (kth_fast_kernel<T>
    keeps the T largest of lane l's elements {i : (i / 4) % 64 == l}, or {i % 64 == l} when the sample's length is no multiple of 4, and
    pops the k largest of the 64 T; kth_kernel takes the k-th largest), thr = that - 2 EPS, candidates = rows scoring >= thr."""
    row = similarity(fx.Q[q:q + 1], fx.G, None if fx.exq is None else fx.exq[q:q + 1], fx.exg)[0]
    ns, k = min(fx.Ng, SAMPLE), fx.k
    sample = row[:ns]
    if k > 128:
        kth = np.sort(sample)[ns - k]
    else:
        T = 2 if k <= 32 else 4
        lane = (np.arange(ns) // 4) % 64 if ns % 4 == 0 else np.arange(ns) % 64
        pool = np.concatenate([np.sort(sample[lane == l])[-T:] for l in range(64)])
        kth = np.sort(pool)[len(pool) - k] if len(pool) >= k else -np.inf
    return int((row >= kth - 2 * EPS16[flavor]).sum())


# ---- the cases of test_retrieval_exact_gpu.py ---------------------------------------------------------------------------------------------------
class Case:
    """One call of a raw entry point on an exact fixture.  path: 'scan' (reid_topk_scan_ok must hold), 'tiled' (it must not, under the
    case's knobs) or 'stream'; knobs: ((name, value), ...) set around the call; complete: planted kinds that must come back unflagged."""

    def __init__(self, path, Nq, Ng, D, k, seed=0, excl='main', neg=False, knobs=(), complete=(), why=''):
        self.path, self.Nq, self.Ng, self.D, self.k, self.seed, self.excl, self.neg = path, Nq, Ng, D, k, seed, excl, neg
        self.knobs, self.complete, self.why = tuple(knobs), tuple(complete), why

    @property
    def id(self):
        knobs = ''.join(f'-{n}{v}' for n, v in self.knobs)
        return f'{self.path}-{self.Nq}x{self.Ng}x{self.D}-k{self.k}-{self.excl}{"-neg" if self.neg else ""}{knobs}'

    def fixture(self):
        return exact_fixture(self.Nq, self.Ng, self.D, self.k, self.seed, self.excl, self.neg)

    @property
    def fast_select(self):
        return self.path != 'stream' and self.k <= SELECT_FAST_K_MAX and ('TOPK_TILE', 9) not in self.knobs


def scan_cases(cus):
    """Scan: Nq <= 128, k <= 16, D in {256, 512}, ceil(Ng / 64) >= 4 k (and cus >= 4 k), Nq min(Ng, 8192) >= 6144.  cus: the device's
    compute units rounded down to a multiple of 8, as the code does."""
    cus = max(cus & ~7, 8)
    S = lambda *a, **kw: Case('scan', *a, **kw)
    T = lambda *a, **kw: Case('tiled', *a, **kw)
    return [
        # the workspace edge Nq * Ng = 6144 (one step per workgroup, chunks = 4 k exactly in the second and third) ...
        S(1, 6144, 512, 1, 0, 'main'), S(3, 2048, 512, 8, 1, None), S(6, 1024, 512, 4, 2, 'main'),
        # ... and just below it: the tiled path
        T(1, 6143, 512, 1, 0, 'main'), T(2, 2048, 512, 8, 1, None), T(5, 1024, 512, 4, 2, 'main'),
        S(33, 4033, 512, 16, 1, 'dense', why='k = KG, two query groups, ragged last tile'),
        S(128, 2561, 512, 10, 0, 'main', why='all four query groups, 41 chunks = 4 k + 1'),
        S(5, 4097, 256, 10, 3, 'main', why='odd Ng, D = 256, exclusion (ADVICE.md)'),
        S(40, 64 * cus + 64 * 3 + 5, 256, 10, 4, 'all', why='some workgroups take two chunks'),
        S(16, 3 * 64 * cus + 37, 256, 10, 2, 'main', why='four steps for some workgroups: ring slots reused'),
        S(16, 3 * 64 * cus + 37, 256, 10, 2, None, neg=True, why='the same without exclusion, scores of one sign'),
        S(8, 2561, 512, 10, 5, None, neg=True, why='D = 512 without exclusion, all-negative rows'),
    ]


NO_SCAN = (('TOPK_SCAN', 0),)


def tiled_cases():
    """Tiled (knob TOPK_SCAN = 0 throughout): filter tile 64x256 for Nq <= 64 and Ng >= 1024, 128x256 for Nq >= 256 and Ng >= 1024, else
    128x128; threshold kth_fast<2> for k <= 32, kth_fast<4> up to 128, kth_kernel beyond; select_fast_kernel for k <= 32 unless
    TOPK_TILE = 9, else select_kernel."""
    T = lambda *a, **kw: Case('tiled', *a, knobs=NO_SCAN + tuple(kw.pop('knobs', ())), **kw)
    tile9 = (('TOPK_TILE', 9),)
    cases = [
        T(3, 1500, 512, 10, 0, 'main'), T(70, 900, 512, 10, 1, 'main'), T(257, 1100, 256, 10, 2, 'dense'),          # the three filter tiles
        T(70, 900, 256, 40, 3, None), T(70, 900, 256, 129, 4, 'main'), T(70, 900, 256, 33, 0, 'all'),               # kth_fast<4>, kth_kernel, select_kernel
        T(3, 1500, 512, 10, 0, 'main', knobs=tile9), T(70, 900, 512, 10, 1, None, neg=True, knobs=tile9),
        # select_kernel has no survivor limit: the 513-row group (seed 3: query 0) fits cap_for = 544 and must come back complete
        T(5, 57400, 256, 10, 3, 'main', knobs=tile9, complete=('tie513',)), T(5, SAMPLE + 300, 256, 40, 3, None, complete=('tie513',)),
        T(3, 1024, 256, 1024, 0, None), T(3, 1500, 256, 1024, 1, 'main'), T(3, 13, 256, 13, 0, 'main'),              # k = 1024, k == Ng
        T(5, SAMPLE, 512, 10, 1, 'main'), T(5, SAMPLE + 1, 512, 10, 2, 'dense'), T(5, SAMPLE + 300, 512, 10, 4, 'main'),
        T(70, 900, 512, 10, 2, None, neg=True),
    ]
    cases += [T(3, 1500, D, 10, i, 'main') for i, D in enumerate((64, 192, 320, 768, 1024))]        # select_fast_kernel's own dot loop
    return cases + [T(3, 1500, D, 10, i, 'main', knobs=tile9) for i, D in ((1, 192), (2, 320))]   # row_dot's ragged tail in select_kernel


def stream_cases():
    """Streaming: Nq <= 4 (NQP = 1, 2, 4, 4), D = 256 DJ with DJ = 1 .. 4 (four rows in flight for DJ <= 2, two beyond), k <= 32; the merge
    runs in LDS or from global memory (stream_merge_in_lds)."""
    S = lambda *a, **kw: Case('stream', *a, **kw)
    excl = ('main', None, 'dense', 'all')
    cases = [S(Nq, 777, D, 10, Nq + j, excl[(Nq + j) % 4]) for Nq in (1, 2, 3, 4) for j, D in enumerate((256, 512, 768, 1024))]
    cases += [S(3, 13, 512, 1, 0, 'main'), S(2, 13, 256, 10, 1, 'dense'), S(4, 777, 256, 32, 2, 'main'), S(1, 777, 1024, 1, 3, None),
              S(2, 8200, 256, 32, 1, 'main', why='merge from global memory'), S(3, 16400, 512, 16, 2, 'main', why='just past the merge switch'),
              S(4, 777, 512, 10, 0, None, neg=True)]
    return cases


def all_cases(cus=256):
    return scan_cases(cus) + tiled_cases() + stream_cases()
