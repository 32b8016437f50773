"""GPU: every path of the cosine top-k (csrc/retrieval.hip, retrieval.py) per element against the fp64 ranking of retrieval_ref.py.

Exact fixtures (integers times a power of two, bit budget checked in test_retrieval_ref_cpu.py): the indices must equal the reference
and the score BITS must equal float32(reference); there is no tolerance.  Rounded fixture (unit fp32 rows, near-duplicate clusters the
16-bit scores cannot order): the indices must equal the fp64 ranking, |score - fp64| <= b with the derived bound
b = (4 ceil(D / 256) + 7) 2^-24 sum_i |q_i g_i|, and the list must be strictly ordered by (its own score descending, index ascending).

Every call writes into sentinel buffers.  The entry points take no leading dimension (row q of a list starts at element q k), so the
"padding columns" of the other exact tests become PAD = 8 sentinel elements in front of the first row and behind the GUARD = 32 guard
rows that follow the last one; all of them must keep the sentinel.  The batched workspace holds random bytes (the streaming one zeros, as
the header asked until this test showed that nothing reads it before writing: test_stream_workspace_need_not_be_zero) and ends in 256
guard bytes that must survive.  A second identical call must give the same bits; in the scan the candidate set of a query follows the
order in which the workgroups publish their maxima, so there a query at the edge of its capacity may be flagged in one call and complete
in the next -- the comparison is then over the queries complete in both.

A raw entry point may flag a query (out_idx[q, 0] == -2) or must return its complete expected list; the queries that MUST be flagged
(retrieval_ref.Fixture.must_flag) and those that must NOT be (Case.complete) are asserted.  reid_cosine_topk_exact then has to complete
every list.  The branch a case reaches is asserted through reid_topk_scan_ok / reid_topk_stream_ok, the knobs, and the conditions
restated in retrieval_ref.py (scan_ok, filter_tile, kth_form, stream_merge_in_lds) next to the case lists.

Worst share of the derived bound b that a returned score used (rounded fixture, 8 x 9001, k = 10, MI355X; the fp32 re-score is the
same arithmetic in both flavors, so the two columns agree), and the exact fixtures.  No assertion failed when the tests first ran, so
there is no "before" column: retrieval.hip and retrieval.py are unchanged; include/reid_hip.h was corrected (see the last test).

    path                                       D = 256  bf16 / f16    D = 512  bf16 / f16    exact fixtures
    scan + select_fast_kernel (raw)                 0.111 / 0.111          0.046 / 0.046     bits equal
    tiled + select_fast_kernel (raw)                0.111 / 0.111          0.046 / 0.046     bits equal
    tiled + select_kernel (TOPK_TILE = 9, raw)      0.111 / 0.111          0.046 / 0.046     bits equal
    ... then reid_cosine_topk_exact                 0.141 / 0.141          0.048 / 0.048     bits equal
    reid_cosine_topk_stream                         0.141 / 0.141          0.048 / 0.048     bits equal
    GalleryIndex.topk (default dispatch)            0.141 / 0.141                            bits equal
    reid_cosine_topk_exact(_slots) called directly                                           bits equal
(the raw rows leave out query 0, whose 3000-row cluster overflows the candidate list; the exact pass and the stream include it)

Two kernel mutations tried once while writing this file, then removed: b[2] for b[3] in dot4_acc fails 158 of these 161 tests; -1e8
for -1e9 as the score of an excluded row fails 28 of them and none of the retrieval tests of test_kernels_gpu.py.
"""
import contextlib

import numpy as np
import pytest
import torch

import retrieval_ref as R
from helpers import is_sentinel, sentinel_buffer

pytestmark = pytest.mark.gpu

MARK = -7777                       # sentinel of the int32 outputs
PAD, GUARD = 8, 32
WS_GUARD, WS_BYTE = 256, 0xA5
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
RAW_CASES = R.all_cases(CUS)
ROUNDED = sorted(R.ROUNDED_SEEDS)


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


@contextlib.contextmanager
def knobs(pairs):
    from prcv2025reid_amd import _lib
    try:
        for name, value in pairs:
            _lib.check(_lib.lib().reid_set_knob(name.encode(), value))
        yield
    finally:
        for name, _ in pairs:
            _lib.check(_lib.lib().reid_set_knob(name.encode(), -1))


class Out:
    """out_idx / out_score [Nq, k] inside flat sentinel buffers: PAD elements | Nq k | GUARD k | PAD."""

    def __init__(self, Nq, k):
        n = PAD + (Nq + GUARD) * k + PAD
        self.ints = torch.full((n,), MARK, dtype=torch.int32, device='cuda')
        self.flts = sentinel_buffer(1, n, torch.float32)[0]
        self.idx = self.ints[PAD:PAD + Nq * k].view(Nq, k)
        self.sc = self.flts[PAD:PAD + Nq * k].view(Nq, k)
        self.end = PAD + Nq * k

    def guards_intact(self):
        return (bool((self.ints[:PAD] == MARK).all()) and bool((self.ints[self.end:] == MARK).all())
                and bool(is_sentinel(self.flts[:PAD]).all()) and bool(is_sentinel(self.flts[self.end:]).all()))

    def untouched(self):
        return bool((self.ints == MARK).all()) and bool(is_sentinel(self.flts).all())

    def lists(self):
        return self.idx.cpu().numpy(), self.sc.cpu().numpy()


def workspace(need, zero=False):
    g = torch.Generator(device='cuda').manual_seed(need)
    buf = torch.randint(0, 256, (need + WS_GUARD,), generator=g, device='cuda', dtype=torch.uint8)
    if zero:
        buf[:need] = 0
    buf[need:] = WS_BYTE
    return buf


def ws_guard_intact(buf):
    return bool((buf[-WS_GUARD:] == WS_BYTE).all())


class Dev:
    """The fixture's operands on the device: fp32 rows, their 16-bit copies (exact for the exact fixtures) and the id vectors."""

    def __init__(self, fx, ops, rows=None):
        Q = fx.Q if rows is None else fx.Q[rows]
        self.Qf = torch.from_numpy(np.array(Q)).float().cuda()
        self.Gf = torch.from_numpy(np.array(fx.G)).float().cuda()
        assert torch.equal(self.Qf.double().cpu(), torch.from_numpy(np.array(Q))), 'operands are fp32 values'
        self.Qb, self.Gb = ops.to_t16(self.Qf), ops.to_t16(self.Gf)
        if fx.exact:
            assert torch.equal(self.Qb.float(), self.Qf) and torch.equal(self.Gb.float(), self.Gf), 'operand not representable in 16 bits'
        self.exq = self.exg = None
        if fx.exq is not None:
            self.exq = torch.from_numpy(np.array(fx.exq if rows is None else fx.exq[rows])).cuda()
            self.exg = torch.from_numpy(np.array(fx.exg)).cuda()
        self.Nq, self.Ng, self.k = self.Qf.shape[0], fx.Ng, fx.k


def call_twice(ops, d, path, same_flags=True):
    """The raw entry point of `path` twice, into fresh sentinel buffers and workspaces; returns the first call's buffers."""
    outs = []
    for _ in range(2):
        out = Out(d.Nq, d.k)
        if path == 'stream':
            ws = workspace(ops.topk_stream_ws_bytes(d.k), zero=True)
            ops.cosine_topk_stream(d.Qf, d.Gf, d.k, ws, out.idx, out.sc, exclude_q=d.exq, exclude_g=d.exg)
        else:
            need = ops.topk_ws_bytes(d.Nq, d.Ng, d.k)
            assert need == R.topk_ws_bytes(d.Nq, d.Ng, d.k)
            ws = workspace(need)
            ops.cosine_topk(d.Qb, d.Gb, d.Qf, d.Gf, d.k, ws, out.idx, out.sc, exclude_q=d.exq, exclude_g=d.exg)
        torch.cuda.synchronize()
        assert out.guards_intact(), 'output guard overwritten'
        assert ws_guard_intact(ws), 'workspace guard overwritten'
        outs.append(out)
    a, b = outs
    if same_flags:
        assert torch.equal(a.ints, b.ints) and torch.equal(a.flts.view(torch.int32), b.flts.view(torch.int32)), 'second call differs'
    else:
        both = ((a.idx[:, 0] != -2) & (b.idx[:, 0] != -2))
        assert torch.equal(a.idx[both], b.idx[both]) and torch.equal(a.sc[both].view(torch.int32), b.sc[both].view(torch.int32))
    return a


def check_lists(fx, idx, sc, rows=None, may_flag=True, must_flag=(), complete=()):
    """Every query is flagged or holds its complete expected list; returns (flagged, worst share of the bound used)."""
    want_i = fx.idx if rows is None else fx.idx[rows]
    want_s = fx.score if rows is None else fx.score[rows]
    flagged = idx[:, 0] == -2
    assert may_flag or not flagged.any(), np.flatnonzero(flagged)
    assert flagged[np.asarray(must_flag, np.int64)].all(), ('not flagged', [q for q in must_flag if not flagged[q]])
    assert not flagged[np.asarray(complete, np.int64)].any(), ('flagged', [q for q in complete if flagged[q]])
    assert (idx[flagged, 1:] == MARK).all() and (sc[flagged, 0] == 0).all(), 'a flagged query has a marker, a zero score and nothing else'
    done = ~flagged
    assert (idx[done] >= 0).all()
    bad = np.argwhere(idx[done] != want_i[done])
    assert bad.size == 0, (np.flatnonzero(done)[bad[:5, 0]], bad[:5, 1], idx[done][bad[:5, 0], bad[:5, 1]], want_i[done][bad[:5, 0], bad[:5, 1]])
    if fx.exact:
        assert np.array_equal(R.bits(sc[done]), R.bits(want_s[done])), np.argwhere(R.bits(sc[done]) != R.bits(want_s[done]))[:5]
        return flagged, 0.0
    bound = fx.bound if rows is None else fx.bound[rows]
    share = np.abs(sc[done].astype(np.float64) - want_s[done]) / bound[done]
    assert share.max() <= 1.0, share.max()
    s, i = sc[done], idx[done]
    assert ((s[:, :-1] > s[:, 1:]) | ((s[:, :-1] == s[:, 1:]) & (i[:, :-1] < i[:, 1:]))).all(), 'returned list not in its own order'
    return flagged, float(share.max())


def exact_pass(ops, d, out):
    scratch = workspace(4 * d.Nq * d.Ng)
    ops.cosine_topk_exact(d.Qf, d.Gf, d.k, scratch[:-WS_GUARD].view(torch.float32), out.idx, out.sc, exclude_q=d.exq, exclude_g=d.exg)
    torch.cuda.synchronize()
    assert out.guards_intact() and ws_guard_intact(scratch)


def assert_branch(ops, c):
    """The path the case is meant to take is the one the library takes (under the case's knobs)."""
    scan = ops.topk_scan_ok(c.Nq, c.Ng, c.D, c.k)
    if c.path == 'scan':
        assert scan and R.scan_ok(c.Nq, c.Ng, c.D, c.k, CUS)
    elif c.path == 'tiled':
        assert not scan
        if ('TOPK_SCAN', 0) not in c.knobs:
            assert not R.scan_ok(c.Nq, c.Ng, c.D, c.k, CUS)
    else:
        assert ops.topk_stream_ok(c.Nq, c.Ng, c.D, c.k) and R.stream_ok(c.Nq, c.Ng, c.D, c.k)


# ---- 1. raw entry points on the exact fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RAW_CASES, ids=[c.id for c in RAW_CASES])
def test_raw_entry_point_exact(ops, case):
    fx = case.fixture()
    d = Dev(fx, ops)
    with knobs(case.knobs):
        assert_branch(ops, case)
        out = call_twice(ops, d, case.path, same_flags=case.path != 'scan')
    idx, sc = out.lists()
    if case.path == 'stream':
        check_lists(fx, idx, sc, may_flag=False)
        return
    complete = [fx.kind.index(kd) for kd in case.complete]
    flagged, _ = check_lists(fx, idx, sc, must_flag=fx.must_flag(case.fast_select), complete=complete)
    exact_pass(ops, d, out)
    check_lists(fx, *out.lists(), may_flag=False)
    print(f'\n{case.id} [{flavor()}]: {int(flagged.sum())} of {fx.Nq} flagged by the raw call; bits equal')


def test_dispatch_of_the_cases_covers_every_branch():
    """The conditions restated in retrieval_ref.py, over the case lists: every filter tile, threshold kernel, select kernel, streaming
    template and merge form is reached by some case."""
    tiled = [c for c in RAW_CASES if c.path == 'tiled']
    assert {R.filter_tile(c.Nq, c.Ng) for c in tiled} == {'64x256', '128x128', '128x256'}
    assert {R.kth_form(c.k) for c in tiled} == {'kth_fast<2>', 'kth_fast<4>', 'kth_kernel'}
    assert {c.fast_select for c in tiled} == {True, False} and any(c.k > 32 for c in tiled) and any(('TOPK_TILE', 9) in c.knobs for c in tiled)
    assert {c.D for c in tiled} >= {64, 192, 320, 768, 1024} and {c.Ng for c in tiled} >= {R.SAMPLE, R.SAMPLE + 1, R.SAMPLE + 300, 13}
    assert any(c.k == c.Ng for c in tiled) and any(c.k == 1024 for c in tiled)
    stream = [c for c in RAW_CASES if c.path == 'stream']
    assert {(c.Nq, c.D) for c in stream} >= {(n, D) for n in (1, 2, 3, 4) for D in (256, 512, 768, 1024)}
    assert {R.stream_merge_in_lds(c.Nq, c.Ng, c.k) for c in stream} == {True, False} and {c.k for c in stream} >= {1, 10, 32}
    scan = [c for c in RAW_CASES if c.path == 'scan']
    assert {(c.D, c.excl is None) for c in scan} == {(256, True), (256, False), (512, True), (512, False)}
    grid = max(CUS & ~7, 8)
    steps = {min(-(-((c.Ng + 63) // 64) // grid), 4) for c in scan}           # most steps a workgroup takes
    assert steps >= {1, 2, 4}, steps


# ---- 2. the rounded fixture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['scan', 'tiled', 'select_kernel', 'stream'])
@pytest.mark.parametrize('key', ROUNDED, ids=[f'{k[0]}x{k[1]}x{k[2]}-k{k[3]}' for k in ROUNDED])
def test_raw_entry_point_rounded(ops, key, path):
    Nq, Ng, D, k = key
    fx = R.rounded_fixture(*key)
    if path == 'stream':                                          # four queries: both clusters and the bit-identical pair
        d = Dev(fx, ops, rows=slice(0, 4))
        assert ops.topk_stream_ok(4, Ng, D, k)
        out = call_twice(ops, d, 'stream')
        _, share = check_lists(fx, *out.lists(), rows=slice(0, 4), may_flag=False)
        print(f'\nrounded {key} stream [{flavor()}]: worst share of b {share:.3f}')
        return
    d = Dev(fx, ops)
    pairs = {'scan': (), 'tiled': R.NO_SCAN, 'select_kernel': R.NO_SCAN + (('TOPK_TILE', 9),)}[path]
    with knobs(pairs):
        assert ops.topk_scan_ok(Nq, Ng, D, k) == (path == 'scan') and R.scan_ok(Nq, Ng, D, k, CUS)
        out = call_twice(ops, d, path, same_flags=path != 'scan')
    # query 0's cluster (3000 rows within the filter margin) exceeds the capacity of 256; query 1's (150) fits it and the 512 survivors
    flagged, share = check_lists(fx, *out.lists(), must_flag=[0], complete=[1] if path != 'scan' else [])
    exact_pass(ops, d, out)
    _, share2 = check_lists(fx, *out.lists(), may_flag=False)
    print(f'\nrounded {key} {path} [{flavor()}]: worst share of b {share:.3f} raw ({int(flagged.sum())} flagged), {share2:.3f} after the exact pass')


# ---- 3. the exact pass called directly ------------------------------------------------------------------------------------------------------
def prefilled(Nq, k, flag):
    """Recognisable lists (index 1000 + q k + r, score q + r / 64) with the queries of `flag` marked -2."""
    out = Out(Nq, k)
    out.idx[:] = (1000 + torch.arange(Nq * k, dtype=torch.int32, device='cuda')).view(Nq, k)
    out.sc[:] = (torch.arange(Nq, device='cuda').view(-1, 1) + torch.arange(k, device='cuda').view(1, -1) / 64.0).float()
    out.idx[torch.as_tensor(flag, device='cuda'), 0] = -2
    return out


def check_partial(fx, before, after, resolved, kept):
    """Queries `resolved` hold the expected list, every other query its bits of before the call (a kept marker included)."""
    bi, bs = before
    ai, as_ = after
    rest = np.setdiff1d(np.arange(fx.Nq), resolved)
    assert np.array_equal(ai[rest], bi[rest]) and np.array_equal(R.bits(as_[rest]), R.bits(bs[rest])), 'an unflagged or unlisted query was written'
    assert (ai[kept, 0] == -2).all()
    assert np.array_equal(ai[resolved], fx.idx[resolved]) and np.array_equal(R.bits(as_[resolved]), R.bits(fx.score[resolved]))


@pytest.mark.parametrize('shape', [(40, 900, 256, 10, 0, 'main'), (9, 1500, 320, 33, 1, 'dense')], ids=['40x900x256', '9x1500x320'])
def test_exact_pass_touches_flagged_queries_only(ops, shape):
    fx = R.exact_fixture(*shape)
    d = Dev(fx, ops)
    flag = np.arange(0, fx.Nq, 3)
    out = prefilled(fx.Nq, fx.k, flag)
    before = out.lists()
    exact_pass(ops, d, out)
    check_partial(fx, before, out.lists(), flag, [])
    again = prefilled(fx.Nq, fx.k, flag)
    exact_pass(ops, d, again)
    assert torch.equal(out.ints, again.ints) and torch.equal(out.flts.view(torch.int32), again.flts.view(torch.int32))


def run_slots(ops, d, out, n_slots):
    """reid_cosine_topk_exact_slots with `slots` and the scratch of n_slots rows inside guarded buffers; returns slots[0]."""
    sl = torch.full((1 + n_slots + 64,), MARK, dtype=torch.int32, device='cuda')
    scratch = workspace(4 * n_slots * d.Ng)
    ops.cosine_topk_exact_slots(d.Qf, d.Gf, d.k, n_slots, sl, scratch[:-WS_GUARD].view(torch.float32), out.idx, out.sc, exclude_q=d.exq,
                                exclude_g=d.exg)
    torch.cuda.synchronize()
    assert out.guards_intact() and ws_guard_intact(scratch) and bool((sl[1 + n_slots:] == MARK).all())
    count = int(sl[0])
    listed = sl[1:1 + min(count, n_slots)].cpu().numpy()
    return count, listed


def test_exact_slots_with_a_short_list(ops):
    """n_slots smaller than the number flagged: the listed queries are resolved, the others keep the marker and every other bit, and
    slots[0] reports how many were flagged."""
    fx = R.exact_fixture(40, 900, 256, 10, 0, 'main')
    d = Dev(fx, ops)
    flag = np.arange(0, fx.Nq, 3)                                 # 14 queries
    out = prefilled(fx.Nq, fx.k, flag)
    before = out.lists()
    count, listed = run_slots(ops, d, out, 5)
    assert count == len(flag) > 5 and len(set(listed)) == 5 and set(listed) <= set(flag)
    check_partial(fx, before, out.lists(), np.sort(listed), np.setdiff1d(flag, listed))
    count, listed = run_slots(ops, d, out, 5)                     # the second call takes five of the remaining nine
    assert count == len(flag) - 5 and len(set(listed)) == 5
    left = np.flatnonzero(out.lists()[0][:, 0] == -2)
    count, listed = run_slots(ops, d, out, fx.Nq)                 # n_slots >= Nq: no marker survives
    assert count == len(flag) - 10 == len(left) and sorted(listed) == list(left)
    check_partial(fx, before, out.lists(), flag, [])
    assert run_slots(ops, d, out, fx.Nq)[0] == 0


def test_exact_slots_beyond_256_flagged(ops):
    """300 flagged queries at Ng = 64, D = 64: the workgroup rows walk the list with a stride of 256."""
    fx = R.exact_fixture(320, 64, 64, 10, 0, 'main')
    d = Dev(fx, ops)
    flag = np.setdiff1d(np.arange(320), np.arange(7, 320, 16))   # 300 queries
    assert len(flag) == 300
    out = prefilled(fx.Nq, fx.k, flag)
    before = out.lists()
    count, listed = run_slots(ops, d, out, fx.Nq)
    assert count == 300 and sorted(listed) == list(flag)
    check_partial(fx, before, out.lists(), flag, [])


# ---- 4. GalleryIndex -------------------------------------------------------------------------------------------------------------------------
def index_topk(fx, **kw):
    from prcv2025reid_amd.retrieval import GalleryIndex
    G = torch.from_numpy(np.array(fx.G)).float().cuda()
    Q = torch.from_numpy(np.array(fx.Q)).float().cuda()
    ids = {} if fx.exq is None else dict(img_ids=torch.from_numpy(np.array(fx.exg)).cuda())
    index = GalleryIndex(G, normalized=True, **ids)
    for name, value in kw.items():
        setattr(index, name, value)
    qid = None if fx.exq is None else torch.from_numpy(np.array(fx.exq)).cuda()
    idx, sc = index.topk(Q, k=fx.k, normalized=True, query_img_ids=qid)
    torch.cuda.synchronize()
    return index, idx.cpu().numpy(), sc.cpu().numpy()


@pytest.mark.parametrize('shape', [(128, 2561, 512, 10, 0, 'main'), (3, 777, 512, 10, 4, 'dense'), (257, 1100, 256, 10, 2, 'dense'),
                                   (1, 6144, 512, 1, 0, 'main')], ids=['scan', 'stream', 'tiled', 'one-query'])
def test_gallery_index_default_dispatch_exact(ops, shape):
    fx = R.exact_fixture(*shape)
    _, idx, sc = index_topk(fx)
    assert (idx >= 0).all()
    check_lists(fx, idx, sc, may_flag=False)


@pytest.mark.parametrize('key', ROUNDED[:1], ids=['8x9001'])
def test_gallery_index_default_dispatch_rounded(ops, key):
    fx = R.rounded_fixture(*key)
    _, idx, sc = index_topk(fx)
    assert (idx >= 0).all()
    _, share = check_lists(fx, idx, sc, may_flag=False)
    print(f'\nrounded {key} GalleryIndex [{flavor()}]: worst share of b {share:.3f}')


def test_gallery_index_chunked_call(ops):
    """Just over 2^26 pairs with a scratch budget of 1000 rows: the call is cut into query chunks of 1000, 1000 and 100, and the queries
    that overflow (the planted ones, from query 1500 on) sit in the second chunk.  The unchunked large call (flags compacted on the device)
    must give the same lists."""
    Nq, Ng, D, k = 2100, 32000, 64, 10
    assert Nq * Ng > 1 << 26
    fx = R.exact_fixture(Nq, Ng, D, k, 0, 'main', False, 1500)
    assert 1000 <= fx.must_flag(True).min() and fx.must_flag(True).max() < 2000 and len(fx.must_flag(True)) >= 3
    index, idx, sc = index_topk(fx, exact_scratch_bytes=1000 * Ng * 4)
    assert index._slots is None                                   # (the chunks took the small-problem form)
    assert (idx >= 0).all()
    check_lists(fx, idx, sc, may_flag=False)
    index, idx, sc = index_topk(fx)
    assert int(index._slots[0]) >= len(fx.must_flag(True))
    assert (idx >= 0).all()
    check_lists(fx, idx, sc, may_flag=False)


# ---- 5. refused calls, and what the streaming workspace may hold ----------------------------------------------------------------------------------
def test_refused_calls_write_nothing(ops):
    from prcv2025reid_amd import _lib
    fx = R.exact_fixture(3, 777, 512, 10, 4, 'dense')
    d = Dev(fx, ops)
    out = Out(8, 1100)
    ws = workspace(ops.topk_ws_bytes(8, 2000, 1024))
    sws = workspace(ops.topk_stream_ws_bytes(1), zero=True)
    lib, s = _lib.lib(), _lib.stream_ptr()
    p = lambda t: None if t is None else t.data_ptr()

    def batched(Nq, Ng, Dd, k, exq, exg):
        return lib.reid_cosine_topk(p(d.Qb), p(d.Gb), p(d.Qf), p(d.Gf), Nq, Ng, Dd, k, p(exq), p(exg), p(ws), p(out.idx), p(out.sc), s)

    def stream(Nq, Ng, Dd, k, exq, exg):
        return lib.reid_cosine_topk_stream(p(d.Qf), p(d.Gf), Nq, Ng, Dd, k, p(exq), p(exg), p(sws), p(out.idx), p(out.sc), s)

    for fn, args, msg in ((batched, (3, 9, 512, 10, None, None), 'k=10'), (batched, (3, 777, 512, 1025, None, None), 'k=1025'),
                          (batched, (3, 777, 96, 10, None, None), 'D=96 must be a multiple of 64'),
                          (batched, (3, 777, 512, 10, d.exq, None), 'go together'), (batched, (3, 777, 512, 10, None, d.exg), 'go together'),
                          (stream, (3, 777, 320, 10, None, None), 'outside the streaming form'),
                          (stream, (5, 100, 512, 10, None, None), 'outside the streaming form'),
                          (stream, (3, 777, 512, 33, None, None), 'outside the streaming form'),
                          (stream, (3, 777, 512, 10, d.exq, None), 'go together'), (stream, (3, 777, 512, 10, None, d.exg), 'go together')):
        with pytest.raises(_lib.ReidHipError, match='rc=-1: reid_cosine_topk.*' + msg):
            _lib.check(fn(*args))
    assert not ops.topk_stream_ok(3, 777, 320, 10) and not ops.topk_stream_ok(5, 777, 512, 10) and not ops.topk_stream_ok(3, 777, 512, 33)
    torch.cuda.synchronize()
    assert out.untouched() and ws_guard_intact(ws) and ws_guard_intact(sws)


def test_stream_workspace_need_not_be_zero(ops):
    """include/reid_hip.h: the streaming workspace is scratch -- every list entry the merge reads was written by the scan of the same
    call.  Random bytes in it give the bits of a zeroed one."""
    fx = R.exact_fixture(3, 16400, 512, 16, 2, 'main')
    d = Dev(fx, ops)
    out = Out(d.Nq, d.k)
    ws = workspace(ops.topk_stream_ws_bytes(d.k))
    ops.cosine_topk_stream(d.Qf, d.Gf, d.k, ws, out.idx, out.sc, exclude_q=d.exq, exclude_g=d.exg)
    torch.cuda.synchronize()
    assert out.guards_intact() and ws_guard_intact(ws)
    check_lists(fx, *out.lists(), may_flag=False)
