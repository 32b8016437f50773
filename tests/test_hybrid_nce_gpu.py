"""GPU: the hybrid memory of SpCL (csrc/hybrid_nce.hip) -- the class means and the refreshed rows of the table BIT FOR BIT against the
fp32 loop of hybrid_nce_ref.py, the loss and dx (reid_cluster_nce_fwd / _bwd against the table of means) and the moved entries
against the fp64 reference within its derived bounds, in both library flavours (the kernels are fp32: the same bits in both) -- and the
loss behind the public call, inside the model, in the graphed step and behind jaccard_dbscan.

Entries, table and every output live between guard elements that hold a sentinel pattern and must keep it; the padding columns of a
padded entry matrix hold NaN.

With ONE class lse = l_y: loss and gradient are 0 by definition, so the grid's C = 1 cases assert exact zeros where the others assert
that what they compare stands 50 bounds above its bound (tests/test_hybrid_nce_cpu.py checks the same on the CPU)."""
import types

import numpy as np
import pytest
import torch

import hybrid_nce_ref as H
from helpers import SENTINEL32
from test_cluster_nce_gpu import GUARD, Table, bits, check_forward, dev, guarded, run_bwd, run_fwd, strided, untouched
from test_hybrid_nce_cpu import DLOSS, GRID, TAU, grid_case

pytestmark = pytest.mark.gpu

U = H.U
_CASE = {}                               # case key -> inputs on the CPU with their fp64 reference (shared by the flavours)


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


class Mem:
    """The memory as the kernels see it: entries [M, D] (leading dimension D + pad, NaN padding) and table [C, D] between guards."""

    def __init__(self, ops, V, cls, C=None, pad=0):
        M, D = V.shape
        order, offsets, counts = H.csr(cls, C)
        self.M, self.D, self.C, self.pad = M, D, len(counts), pad
        self.bV, flat = guarded(M * (D + pad))
        wide = flat.view(M, D + pad)
        wide.fill_(float('nan'))
        self.wide, self.V = wide, wide[:, :D]
        self.V.copy_(torch.from_numpy(V))
        self.table = Table(np.zeros((self.C, D), dtype=np.float32))
        self.table.buf.fill_(SENTINEL32)                             # (the means kernel must write every row itself)
        self.T = self.table.t
        self.order, self.offsets, self.cls = dev(order), dev(offsets), np.asarray(cls)
        ops.class_means(self.V, self.order, self.offsets, self.T)
        torch.cuda.synchronize()
        self.intact()

    def intact(self):
        assert untouched(self.bV, self.M * (self.D + self.pad)) and self.table.intact(), 'guard elements overwritten'
        if self.pad:
            assert bool(torch.isnan(self.wide[:, self.D:]).all()), 'padding columns overwritten'

    def entries(self):
        return self.V.cpu().numpy().copy()


def run_update(ops, o, mem, index, momentum):
    """Both kernels of the update, in stream order, with what the forward ``o`` left."""
    ops.hybrid_update_instances(index, o['valid'], o['row_loss'], o['ws'], mem.V, momentum, S=o['S'])
    ops.hybrid_refresh_classes(o['labels'], o['valid'], o['row_loss'], mem.V, mem.order, mem.offsets, mem.T, S=o['S'])
    torch.cuda.synchronize()
    mem.intact()


def forward(ops, mem, x, index, valid, tau, pad=0, with_grad=True):
    return run_fwd(ops, x, H.gather_labels(index, mem.cls), valid, mem.table, tau, with_grad, pad)


def check_dx(dx, f, D, C, tau, dloss, T):
    g = dx.double().cpu().numpy()
    want = f['dx'] * dloss                                       # (the reference was formed with dloss = 1)
    bound = H.dx_bound(f, D, C, tau, dloss, H.table_norm(T))[:, None]
    assert bool((np.abs(g - want) <= bound).all()), float((np.abs(g - want) / bound).max())
    assert not g[~f['used']].any()
    return f'{np.abs(g - want).max():.3e} / {np.abs(want).max():.3e} / {bound[f["used"]].max() if f["used"].any() else 0.0:.3e}'


def check_update(mem, V0, T0, f, momentum):
    """The memory after ONE update from (V0, T0) with the forward ``f``: entries within the blend recurrence's bound, the table rows of
    the touched classes bit-equal to the numpy means of the entries read back, everything else with unchanged bits."""
    want, err = H.update_instances(V0, f, momentum)
    got = mem.entries()
    inst, classes = H.touched(f, mem.cls)
    d = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    assert np.isfinite(got).all() and bool((d <= err).all()), (d / np.maximum(err, 1e-300)).max()
    for i in range(mem.M):
        if i not in inst:
            assert np.array_equal(got[i].view(np.int32), V0[i].view(np.int32)), f'entry {i} was touched'
    fresh = H.class_means(got, mem.cls, mem.C)
    T = mem.T.cpu().numpy()
    for c in range(mem.C):
        assert np.array_equal(T[c].view(np.int32), (fresh if c in classes else T0)[c].view(np.int32)), (c, c in classes)
    return inst, classes, (d[inst] / err[inst]).max() if inst else 0.0


# ---------------------------------------------------------------------------------------------------------------- 1. the means
LAYOUTS = {'to65': [1, 2, 63, 64, 65, 205], 'to257': [257, 1, 2, 64, 65, 11]}      # class sizes; each fills M = 400 rows


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('D', [32, 96, 512])
def test_class_means_bit_for_bit(ops, D, layout):
    """Class sizes 1, 2, 63, 64, 65 and 257 (below, at and above the rows a thread keeps in flight, and a long tail), their members
    interleaved through M = 400 rows; entries of mixed magnitude and sign so that the order of the additions shows."""
    sizes = LAYOUTS[layout]
    g = np.random.default_rng(D + len(layout))
    cls = np.repeat(np.arange(len(sizes)), sizes)[g.permutation(400)]
    V = (g.standard_normal((400, D)) * np.exp2(g.integers(-6, 7, size=(400, 1)))).astype(np.float32)
    V[cls == 0, 3] = -0.0                                        # (a singleton, or the first members of the 257: the sign of a zero)
    want = H.class_means(V, cls)
    assert np.abs(want - H.class_means64(V, cls)).max() > 0      # the fp32 sums do round: a reordered sum would show
    rev = H.class_means(V[::-1].copy(), cls[::-1].copy())        # the members of every class in descending order
    assert not np.array_equal(rev.view(np.int32), want.view(np.int32))
    mem = Mem(ops, V, cls, pad=0 if D == 96 else 4)
    assert not bool((mem.T.view(torch.int32) == SENTINEL32).any()), 'rows of the table not written'
    assert torch.equal(bits(mem.T), bits(want))
    assert np.array_equal(mem.entries().view(np.int32), V.view(np.int32))                # the entries are read only


# ---------------------------------------------------------------------------------------------------------------- 2. loss and dx
@pytest.mark.parametrize('S,N,C', GRID)
def test_loss_and_dx_against_the_reference(ops, S, N, C):
    key = (S, N, C)
    if key not in _CASE:
        _CASE[key] = grid_case(S, N, C)
    D, V, cls, T, x, index, valid, f = _CASE[key]
    counts = np.bincount(cls, minlength=C)
    hit = counts[f['y'][f['used']]]
    assert f['n_used'] > 0
    if C > 1:                                                    # from the reference alone: every used row stands 50 bounds above its bound
        s_row, s_dx = H.signal(f, D, C, TAU, DLOSS, H.table_norm(T))
        assert s_row >= 50 and s_dx >= 50, (s_row, s_dx)
        assert (hit == 1).any() and (N < 3 or (hit > 1).any())
    mem = Mem(ops, V, cls, C, pad=4 if S == 3 else 0)
    assert torch.equal(bits(mem.T), bits(T))                     # the table the reference used is the device's, bit for bit
    o = forward(ops, mem, x, index, valid, TAU, pad=4 if N == 65 else 0)
    e_row, e_cos, e_loss = check_forward(o, f, D, C, TAU)
    dx = run_bwd(ops, o, DLOSS)
    m_dx = check_dx(dx, f, D, C, TAU, DLOSS, T)
    print(f'measured D={D} C={C} R={S * N}: row {e_row:.3e} / {H.row_bound(D, C, TAU):.3e}  cos {e_cos:.3e} / {H.cos_bound(D):.3e}  '
          f'loss {e_loss:.3e} / {H.loss_bound(D, C, TAU):.3e}  dx error / largest |dx| / bound {m_dx}')
    if C > 1:
        assert float(dx.abs().max()) > 0
    else:
        assert float(o['result'][0]) == 0.0 and float(o['row_loss'].abs().max()) == 0.0 and float(dx.abs().max()) == 0.0
    assert torch.equal(bits(mem.T), bits(T)) and np.array_equal(mem.entries().view(np.int32), V.view(np.int32))      # forward and backward read only


# ---------------------------------------------------------------------------------------------------------------- 3. the update
def update_case(D):
    """S = 3 sides of N = 8 rows over M = 40 instances in 12 classes.  Instance 5 appears twice in a side (n = 0 and n = 2) and so six
    times over the three sides; n = 3 and n = 4 lie outside the memory (-1 and M); row (1, 1) is invalid; instance 7 (n = 6) has a NaN
    row in side 0 and invalid rows in sides 1 and 2: it does not contribute, its entry and its class (a singleton) stay; instance
    12 (n = 5) has a NaN row in side 1 and contributes through sides 0 and 2."""
    g = np.random.default_rng(50 + D)
    M, C = 40, 12
    cls = np.arange(M) % 6                                       # classes 0 .. 5 are clusters, 6 .. 11 one instance each
    for c, i in enumerate((7, 13, 21, 29, 33, 38)):
        cls[i] = 6 + c
    cent = g.standard_normal((C, D))
    V = cent[cls] / np.linalg.norm(cent[cls], axis=1, keepdims=True) + 0.5 * g.standard_normal((M, D)) / np.sqrt(D)
    V = (V / np.linalg.norm(V, axis=1, keepdims=True)).astype(np.float32)
    index = np.array([5, 9, 5, -1, M, 12, 7, 20])
    x = (g.standard_normal((3, 8, D)) * g.uniform(0.5, 3.0, size=(3, 8, 1))).astype(np.float32)
    valid = np.ones((3, 8), dtype=np.uint8)
    valid[1, 1] = valid[1, 6] = valid[2, 6] = 0
    x[0, 6, 2] = np.nan
    x[1, 5, 1] = np.nan
    return V, cls, x, index, valid


@pytest.mark.parametrize('momentum', [0.2, 0.0, 1.0])
@pytest.mark.parametrize('D', [32, 96, 512])
def test_update_against_the_reference(ops, D, momentum):
    V, cls, x, index, valid = update_case(D)
    C = int(cls.max()) + 1
    assert np.bincount(cls, minlength=C).min() >= 1 and (cls == cls[7]).sum() == 1
    mem = Mem(ops, V, cls, C, pad=4 if D == 32 else 0)
    T0 = mem.T.cpu().numpy().copy()
    f = H.forward(x, index, valid, T0, cls, TAU)
    con = H.contributing(f)
    assert [r for r in range(24) if con[r] and f['index'][r] == 5] == [0, 2, 8, 10, 16, 18]
    assert f['used'][6] and not con[6] and f['used'][13] and not con[13] and not f['used'][[3, 4, 9, 14, 22]].any()
    # the order matters: the same rows blended in the reverse order give another entry
    if 0 < momentum < 1:
        a = H.blend_f32(V[5], f['xhat'][[0, 2, 8, 10, 16, 18]], momentum)
        b = H.blend_f32(V[5], f['xhat'][[18, 16, 10, 8, 2, 0]], momentum)
        assert np.abs(a - b).max() > 1e-3 and np.linalg.norm(a - H.update_instances(V, f, momentum)[0][5]) <= 1e-5
    o = forward(ops, mem, x, index, valid, TAU)
    assert not np.isfinite(float(o['result'][0]))                # the NaN rows are used: the step driver skips such a step
    run_update(ops, o, mem, dev(index), momentum)
    inst, classes, ratio = check_update(mem, V, T0, f, momentum)
    assert inst == [5, 9, 12, 20] and classes == [0, 2, 3, 5] and cls[7] == 6
    print(f'measured update D={D} m={momentum}: largest entry deviation / bound {ratio:.3e}')
    got = mem.entries()
    if momentum < 1:
        assert all(not np.array_equal(got[i], V[i]) for i in inst)
    if momentum == 0:                                            # the entry is the last contributing row's unit row
        assert np.abs(got[5] - f['xhat'][18]).max() <= H.R.e_n(D) + U
    assert np.abs(np.linalg.norm(got[inst].astype(np.float64), axis=1) - 1).max() <= H.R.e_n(D) + U


def test_batches_without_a_used_row_move_nothing(ops):
    V, cls, x, index, valid = update_case(96)
    mem = Mem(ops, V, cls)
    T0 = mem.T.cpu().numpy().copy()
    for idx, val in ((index, np.zeros((3, 8), dtype=np.uint8)), (np.full(8, -1), valid), (np.full(8, 40), None)):
        o = forward(ops, mem, np.nan_to_num(x), idx, val, TAU)
        assert o['result'].tolist() == [0.0, 0.0]
        run_update(ops, o, mem, dev(idx), 0.2)
        assert np.array_equal(mem.entries().view(np.int32), V.view(np.int32)) and torch.equal(bits(mem.T), bits(T0))
        assert float(run_bwd(ops, o, 3.0).abs().max()) == 0.0


def test_the_clamp_of_a_blend_that_cancels(ops):
    """x^ = -v exactly (entries +-0.5, an exactly unit row) at m = 0.5: the blend is 0, divided by the 1e-12 clamp it stays 0 -- and
    so does the mean of its singleton class."""
    D, M = 32, 6
    V, cls = H.memory_case(M, D, M, 3)                           # six singletons
    V[2] = 0.0; V[2, [1, 7, 20, 31]] = [0.5, -0.5, 0.5, 0.5]
    x = np.stack([-V[2], 2.0 * V[4]])[None]
    index = np.array([2, 4])
    mem = Mem(ops, V, cls)
    T0 = mem.T.cpu().numpy().copy()
    f = H.forward(x, index, None, T0, cls, TAU)
    assert np.array_equal(f['xhat'][0], -V[2].astype(np.float64))
    o = forward(ops, mem, x, index, None, TAU)
    run_update(ops, o, mem, dev(index), 0.5)
    check_update(mem, V, T0, f, 0.5)
    got = mem.entries()
    assert not got[2].any() and not mem.T[cls[2]].cpu().numpy().any() and np.isfinite(got).all()
    assert np.abs(got[4] - V[4]).max() <= 2 * (H.R.e_n(D) + U)     # blended with itself


def test_leader_rows_beyond_the_first_wave_and_workgroup(ops):
    """S * N = 300 rows at D = 32 (64 threads per refresh workgroup: its scan for an earlier row takes several rounds): class 0's only
    contributing rows are 290 .. 299, instance 3 contributes from rows 130 and 280 only."""
    D, M, N = 32, 30, 300
    V, cls = H.memory_case(M, D, 6, 9)
    zero = np.flatnonzero(cls == 0)
    others = np.array([i for i in range(M) if cls[i] != 0 and i != 3])
    g = np.random.default_rng(1)
    index = others[g.integers(0, len(others), size=N)]
    index[290:] = zero[g.integers(0, len(zero), size=10)]
    if cls[3] != 0:
        index[[130, 280]] = 3
    x = (g.standard_normal((1, N, D)) * 1.5).astype(np.float32)
    mem = Mem(ops, V, cls)
    T0 = mem.T.cpu().numpy().copy()
    f = H.forward(x, index, None, T0, cls, TAU)
    o = forward(ops, mem, x, index, None, TAU)
    run_update(ops, o, mem, dev(index), 0.5)                      # (m / nu < 1 for these blends: the bound stays linear in the rows)
    inst, classes, _ = check_update(mem, V, T0, f, 0.5)
    assert 0 in classes and set(zero.tolist()) & set(inst)


# ---------------------------------------------------------------------------------------------------------------- 4. sequencing
def sequence_case():
    """M = 400 instances, D = 512, the classes of LAYOUTS['to257']: every refresh of class 0 gathers 257 rows."""
    g = np.random.default_rng(8)
    sizes = LAYOUTS['to257']
    cls = np.repeat(np.arange(len(sizes)), sizes)[g.permutation(400)]
    V = g.standard_normal((400, 512))
    V = (V / np.linalg.norm(V, axis=1, keepdims=True)).astype(np.float32)
    batches = []
    for s in range(5):
        index = g.integers(0, 400, size=21)
        index[4] = -1
        x = (g.standard_normal((3, 21, 512)) * g.uniform(0.5, 3.0, size=(3, 21, 1))).astype(np.float32)
        valid = np.ones((3, 21), dtype=np.uint8); valid.reshape(-1)[s::9] = 0
        batches.append((x, index, valid))
    return V, cls, batches


def test_table_equals_the_means_of_the_entries_after_five_updates(ops):
    V, cls, batches = sequence_case()
    runs = []
    for _ in range(2):
        mem, out = Mem(ops, V, cls), []
        for x, index, valid in batches:
            o = forward(ops, mem, x, index, valid, TAU)
            run_update(ops, o, mem, dev(index), 0.2)
            out += [bits(o['row_loss']), bits(o['result']), bits(run_bwd(ops, o, -2.0)), bits(mem.V), bits(mem.T)]
        got = mem.entries()
        assert np.abs(got - V).max() > 1e-3
        assert torch.equal(bits(mem.T), bits(H.class_means(got, cls)))                   # the invariant, over ALL classes
        fresh = Mem(ops, got, cls)                                                       # and against the device's own means from scratch
        assert torch.equal(bits(fresh.T), bits(mem.T))
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))                                 # two runs give the same bits


def test_backward_is_independent_of_a_later_forward_and_update(ops):
    V, cls, batches = sequence_case()
    runs = []
    for later in (False, True):
        mem = Mem(ops, V, cls)
        x, index, valid = batches[0]
        o = forward(ops, mem, x, index, valid, TAU)
        if later:
            run_update(ops, o, mem, dev(index), 0.2)
            x2, index2, valid2 = batches[1]
            run_update(ops, forward(ops, mem, x2, index2, valid2, TAU), mem, dev(index2), 0.2)
            assert np.abs(mem.entries() - V).max() > 1e-3
        runs.append(bits(run_bwd(ops, o, 1.25)))
    assert torch.equal(runs[0], runs[1]) and bool((runs[0] != 0).any())


def test_graph_replay_equals_eager_bit_for_bit(ops):
    """Forward, both update kernels and backward captured once as ONE linear chain on the capture stream and replayed three times give
    the bits of three eager rounds -- loss, row losses, dx, the entries and the table, which every round moves."""
    S, N, D, C, M = 3, 21, 96, 30, 70
    V, cls = H.memory_case(M, D, C, 17)
    x, index, valid = H.batch_case(S, N, D, V, cls, 18)
    order, offsets, _ = H.csr(cls, C)
    xd, idx, vd = dev(x).reshape(S * N, D).contiguous(), dev(index), dev(valid).reshape(-1).contiguous()
    lab, od, fd = dev(H.gather_labels(index, cls)), dev(order), dev(offsets)
    dloss = torch.tensor([0.75], device='cuda')
    keys = ('res', 'row_loss', 'dx', 'V', 'T')

    def buffers():
        b = dict(V=dev(V).clone(), T=torch.empty(C, D, device='cuda'), ws=torch.empty(ops.cluster_nce_ws_floats(S, N, D, C), device='cuda'),
                 row_loss=torch.empty(S * N, device='cuda'), tcos=torch.empty(S * N, device='cuda'), res=torch.empty(2, device='cuda'),
                 dx=torch.empty(S * N, D, device='cuda'))
        ops.class_means(b['V'], od, fd, b['T'])
        return b

    def round_(b):
        ops.cluster_nce_fwd(xd, lab, vd, b['T'], TAU, True, b['ws'], b['row_loss'], b['tcos'], b['res'], S=S)
        ops.hybrid_update_instances(idx, vd, b['row_loss'], b['ws'], b['V'], 0.2, S=S)
        ops.hybrid_refresh_classes(lab, vd, b['row_loss'], b['V'], od, fd, b['T'], S=S)
        ops.cluster_nce_bwd(b['ws'], b['res'], dloss, b['dx'], S=S)

    eager, outs = buffers(), []
    for _ in range(3):
        round_(eager)
        torch.cuda.synchronize()
        outs.append([bits(eager[k]) for k in keys])
    assert not torch.equal(outs[0][3], outs[2][3]) and not torch.equal(outs[0][4], outs[2][4]) and not torch.equal(outs[0][0], outs[2][0])
    graphed = buffers()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        round_(graphed)
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        for k, want in zip(keys, outs[i]):
            assert torch.equal(bits(graphed[k]), want), (i, k)


def test_violated_requirements_are_refused_and_write_nothing(ops):
    import test_hybrid_nce_cpu as T
    from prcv2025reid_amd import _lib
    h = _lib.lib()
    t = {n: torch.full((k,), SENTINEL32, dtype=torch.int32, device='cuda') for n, k in (('V', 1024), ('T', 512), ('ws', 4096), ('row_loss', 16))}
    for n in ('order', 'offsets', 'index', 'labels'):
        t[n] = torch.zeros(16, dtype=torch.int64, device='cuda')
    good = dict(T.good_arguments(), stream=_lib.stream_ptr(), **{n: v.data_ptr() for n, v in t.items()})
    seen = set()
    for entry, over, text in T.violations():
        over = {k: (good[k] + (v & 15) if k in t and isinstance(v, int) else v) for k, v in over.items()}      # misaligned DEVICE pointers
        rc = T.call(h, entry, {**good, **over})
        assert rc == -1, (entry, over, rc)
        assert text.encode() in h.reid_last_error(), (entry, over, h.reid_last_error())
        seen.add(entry)
    torch.cuda.synchronize()
    assert seen == set(T.ENTRY)
    for n, v in t.items():
        assert bool((v == (0 if v.dtype == torch.int64 else SENTINEL32)).all()), f'{n} was written'


# ---------------------------------------------------------------------------------------------------------------- 5. public call
def test_public_call_update_flags_and_errors(ops):
    from prcv2025reid_amd import losses, _lib
    S, N, D, C, M = 3, 7, 96, 9, 25
    V, cls = H.memory_case(M, D, C, 21)
    x, index, valid = H.batch_case(S, N, D, V, cls, 22)
    raw = (V * np.linspace(0.5, 4.0, M)[:, None]).astype(np.float32)             # from_labels normalises
    mem = losses.HybridMemory.from_labels(dev(raw), dev(cls.astype(np.int32)))
    assert (mem.num_instances, mem.dim, mem.num_classes) == (M, D, C) and mem.counts.tolist() == np.bincount(cls).tolist()
    V0 = mem.instances.cpu().numpy().copy()
    assert np.abs(V0.astype(np.float64) - V).max() <= H.R.e_n(D) + 2 * U and torch.equal(mem.labels.cpu(), torch.from_numpy(cls))
    T0 = H.class_means(V0, cls, C)
    assert torch.equal(bits(mem.table), bits(T0))
    f = H.forward(x, index, valid, T0, cls, TAU)
    assert min(H.signal(f, D, C, TAU, -1.5, H.table_norm(T0))) >= 50
    xa = dev(x).requires_grad_(True)
    loss, n_used, rows = losses.hybrid_nce(xa, dev(index), mem, valid=dev(valid) != 0, update=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(mem.instances), bits(V0)) and torch.equal(bits(mem.table), bits(T0))      # update=False
    assert int(n_used) == f['n_used'] and rows['row_loss'].shape == (S, N) and rows['target_cos'].shape == (S, N)
    assert rows['labels'].tolist() == H.gather_labels(index, cls).tolist()
    assert abs(float(loss.detach()) - f['loss']) <= H.loss_bound(D, C, TAU)
    assert np.abs(rows['row_loss'].double().cpu().numpy().reshape(-1) - f['row_loss']).max() <= H.row_bound(D, C, TAU)
    rows['row_loss'].zero_(); rows['target_cos'].zero_(); rows['labels'].zero_()      # copies: writing into them must not reach the backward
    (loss * -1.5).backward()
    assert xa.grad.shape == x.shape
    check_dx(xa.grad.reshape(S * N, D), f, D, C, TAU, -1.5, T0)
    with torch.no_grad():                                        # no_grad: the loss is there, the memory stays
        loss2, _, _ = losses.hybrid_nce(dev(x), dev(index), mem, valid=dev(valid))
    torch.cuda.synchronize()
    assert torch.equal(bits(mem.instances), bits(V0)) and torch.equal(bits(mem.table), bits(T0)) and torch.equal(bits(loss2), bits(loss))
    loss3, _, _ = losses.hybrid_nce(dev(x), dev(index), mem, valid=dev(valid))      # the defaults: tau = 0.05, m = 0.2, update
    torch.cuda.synchronize()
    want, err = H.update_instances(V0, f, 0.2)
    got = mem.instances.cpu().numpy()
    assert torch.equal(bits(loss3), bits(loss)) and bool((np.linalg.norm(got.astype(np.float64) - want, axis=1) <= err).all())
    assert np.abs(got - V0).max() > 1e-3 and torch.equal(bits(mem.table), bits(H.class_means(got, cls, C)))
    moved = bits(mem.instances)
    l1, n1, r1 = losses.hybrid_nce(dev(x)[0], dev(index), mem, valid=dev(valid)[0], update=False)      # one side, flat
    assert r1['row_loss'].shape == (N,) and r1['labels'].shape == (N,) and int(n1) == int(f['used'][:N].sum())
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.hybrid_nce(dev(x)[..., :32], dev(index), mem)
    with pytest.raises(TypeError, match='HybridMemory'):
        losses.hybrid_nce(dev(x), dev(index), mem.table)
    for bad, text in ((dict(temperature=0.0), 'temperature'), (dict(momentum=1.5), 'momentum')):
        with pytest.raises(ValueError, match=text):
            losses.hybrid_nce(dev(x), dev(index), mem, **bad)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.hybrid_nce(torch.from_numpy(x), torch.from_numpy(index), mem)
    with pytest.raises(ValueError, match=r'hybrid_labels\(\)'):
        losses.HybridMemory.from_labels(dev(raw), dev(np.where(cls == 1, -1, cls)))
    assert torch.equal(bits(mem.instances), moved)               # a refused call moves nothing


def test_set_labels_keeps_the_entries_and_rebuilds_the_table(ops):
    from prcv2025reid_amd import losses
    M, D = 60, 96
    V, cls = H.memory_case(M, D, 10, 5)
    mem = losses.HybridMemory.from_labels(dev(V), dev(cls))
    held, V0 = mem.instances, bits(mem.instances)
    new = np.random.default_rng(6).integers(0, 17, size=M)
    new[:17] = np.arange(17)
    mem.set_labels(dev(new))
    assert mem.instances is held and torch.equal(bits(mem.instances), V0)
    assert mem.num_classes == 17 and mem.table.shape == (17, D) and mem.counts.tolist() == np.bincount(new).tolist()
    assert torch.equal(bits(mem.table), bits(H.class_means(mem.instances.cpu().numpy(), new, 17)))
    st = mem.state()
    other = losses.HybridMemory(M, D, 'cuda')
    other.load_state(st)
    assert torch.equal(bits(other.instances), V0) and torch.equal(bits(other.table), bits(mem.table)) and other.num_classes == 17


def test_five_sgd_steps_follow_the_reference_trajectory(ops):
    """A free [64, 32] tensor against a memory of 80 instances in 12 classes, tau = 0.2, lr = 0.2, momentum 0.5.  The fp64 reference
    runs its own trajectory (its table: the fp64 means of its own entries); the bounds are chained as in
    test_cluster_nce_gpu.test_five_sgd_steps_follow_the_reference_trajectory, with a = the largest row deviation of x, av [M] = the
    deviation of every entry, and the table's b_c = the largest av among the members of c (a mean of vectors each off by at most
    that) + n_c u (the n_c - 1 fp32 additions of vectors of norm <= 1 and the division)."""
    from prcv2025reid_amd import losses
    N, D, C, M, tau, lr, m = 64, 32, 12, 80, 0.2, 0.2, 0.5
    V, cls = H.memory_case(M, D, C, 77)
    counts = np.bincount(cls, minlength=C)
    g = np.random.default_rng(78)
    index = g.permutation(M)[:N]
    x = g.standard_normal((1, N, D))
    x = (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    mem = losses.HybridMemory.from_labels(dev(V), dev(cls))
    xg = dev(x[0]).requires_grad_(True)
    x64, V64 = x.astype(np.float64), mem.instances.double().cpu().numpy()
    a, av = 0.0, np.zeros(M)
    Lx = lambda xmin: (1 / tau ** 2 + 6 / tau) / xmin ** 2
    Lc = lambda xmin: (2 / tau ** 2 + 2 / tau) / xmin
    first = None
    for step in range(5):
        T64 = H.class_means64(V64, cls, C)
        b = np.array([av[cls == c].max() for c in range(C)]) + counts * U
        f = H.forward(x64, index, None, T64, cls, tau)
        first = f['loss'] if first is None else first
        xmin = float(np.linalg.norm(x64[0], axis=1).min()) - a
        assert xmin > 0.5
        loss, n_used, _ = losses.hybrid_nce(xg, dev(index), mem, temperature=tau, momentum=m)
        loss.backward()
        e_loss = abs(float(loss.detach()) - f['loss'])
        bound = H.loss_bound(D, C, tau) + a * 2 / (tau * xmin) + b.max() * 2 / tau
        print(f'step {step}: loss {float(loss.detach()):.6f} error {e_loss:.3e} bound {bound:.3e}')
        assert int(n_used) == N and e_loss <= bound, (step, e_loss, bound)
        V64, av_new = H.update_instances(V64, f, m, err0=av, xhat_dev=a / xmin)
        got = mem.instances.cpu().numpy()
        dev_v = np.linalg.norm(got.astype(np.float64) - V64, axis=1)
        assert bool((dev_v <= av_new).all()), (step, (dev_v / np.maximum(av_new, 1e-300)).max())
        assert torch.equal(bits(mem.table), bits(H.class_means(got, cls, C)))
        g_dev = float(np.sqrt(D)) * float(H.dx_bound(f, D, C, tau, 1.0, H.table_norm(T64)).max()) + (Lx(xmin) * a + Lc(xmin) * b.max()) / N
        with torch.no_grad():
            xg.add_(xg.grad, alpha=-lr)
            xg.grad = None
        x64 = x64 - lr * f['dx'][None]
        a = a + lr * g_dev + 2 * U * float(np.linalg.norm(x64[0], axis=1).max())
        av = av_new
        dev_x = float(np.linalg.norm(xg.detach().double().cpu().numpy() - x64[0], axis=1).max())
        assert dev_x <= a, (step, dev_x, a)
    assert f['loss'] < first                                     # the steps descend


# ---------------------------------------------------------------------------------------------------------------- 6. model level
from test_cluster_nce_gpu import BASE_KEYS, _inputs, _term_inputs, _tiny8      # noqa: E402

NEW_KEYS = ['hybrid_nce_loss', 'hybrid_nce_valid_cnt']
INDEX8 = [3, 7, 0, 12, 19, 5, 8, 3]                                # the dataset rows of the batch's 8 instances (row 3 twice)
CLS20 = [0, 1, 0, 1, 3, 1, 0, 2, 0, 1, 0, 1, 4, 0, 1, 5, 0, 1, 0, 1]      # 20 instances: classes 0 and 1 clusters, 2 .. 5 outliers


def _hybrid_memory(D, seed):
    from prcv2025reid_amd.losses import HybridMemory
    g = np.random.default_rng(seed)
    return HybridMemory.from_labels(dev(g.standard_normal((20, D)).astype(np.float32)), torch.tensor(CLS20).cuda())


def test_weight_zero_is_the_model_without_the_fields():
    from helpers import case_config
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    meta, state, batch, make = _tiny8()
    images, masks, labels = _inputs(batch)
    cfg = case_config(meta, device='cuda')
    cfg.compute_dtype = 'bf16'
    bare = types.SimpleNamespace(**{k: v for k, v in vars(cfg).items() if not k.startswith('hybrid_nce_')})
    assert not hasattr(bare, 'hybrid_nce_weight') and hasattr(cfg, 'hybrid_nce_weight')
    old = CLIPBasedMultiModalReIDModel(bare)
    old.set_num_classes(int(meta['num_classes'])); old.load_state_dict(state, strict=True); apply_reference_freeze(old)
    old.contrastive_weight = meta['contrastive_weight']; old.set_epoch(2); old.train(True)
    out_old = old(images=images, texts=batch['texts'], modality_masks=masks)
    L_old = old.compute_loss(out_old, labels)
    new = make(hybrid_nce_weight=0.0, hybrid_nce_source='modalities')
    out_new = new(images=images, texts=batch['texts'], modality_masks=masks)
    L_new = new.compute_loss(out_new, labels)
    assert list(L_old) == list(L_new) == BASE_KEYS and new.hybrid_memory is None and old.hybrid_memory is None
    for k in ('features', 'bn_features', 'logits'):
        assert torch.equal(bits(out_old[k]), bits(out_new[k])), k
    for k in BASE_KEYS[:-1]:
        assert torch.equal(bits(L_old[k]), bits(L_new[k])), k
    assert int(L_old['ce_valid_cnt']) == int(L_new['ce_valid_cnt'])
    # Gradients: the loss side of the backward (what compute_loss decides) is atomic-free and compared bit for bit at the logits; the
    # adapter-gradient kernels behind it add with fp32 atomics, so two backward passes of ONE model already differ in the last bits
    # of the arena gradient: a reordered fp32 sum of n terms moves by at most 2 n u of the terms' magnitude, n = the rows of the
    # batch's token matrices (a few thousand) -> 1e-4 of the largest gradient.
    out_old['logits'].retain_grad(); out_new['logits'].retain_grad()
    old.lora_arena.grad = None; new.lora_arena.grad = None
    L_old['total_loss'].backward(); L_new['total_loss'].backward()
    assert torch.equal(bits(out_old['logits'].grad), bits(out_new['logits'].grad)) and float(out_new['logits'].grad.abs().max()) > 0
    ga, gb = old.lora_arena.grad, new.lora_arena.grad
    assert float(gb.abs().max()) > 0 and float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max())


@pytest.mark.parametrize('source', ['bn', 'modalities'])
def test_model_loss_with_the_hybrid_term(source, tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    meta, state, batch, make = _tiny8()
    images, masks, _ = _inputs(batch)
    assert int(meta['num_classes']) >= 3                         # the CE sees the classes 0, 1 and 2 of the memory
    index = torch.tensor(INDEX8).cuda()
    cls = np.array(CLS20)
    w, tau, m = 0.5, 0.05, 0.2
    model = make(hybrid_nce_weight=w, hybrid_nce_source=source)
    assert model.hybrid_memory is None and (model.hybrid_nce_temperature, model.hybrid_nce_momentum) == (tau, m)
    keys_before = set(model.state_dict())
    out = model(images=images, texts=batch['texts'], modality_masks=masks)
    with pytest.raises(ValueError, match='needs a hybrid memory'):
        model.compute_loss(out, index)
    x, valid = _term_inputs(out, source)
    S, B, D = x.shape
    mem = _hybrid_memory(D, 5)
    V0, T0 = mem.instances.cpu().numpy().copy(), mem.table.cpu().numpy().copy()
    assert torch.equal(bits(T0), bits(H.class_means(V0, cls, 6)))
    # what every other term and the CE must see: the memory's classes of the indices
    model.hybrid_nce_weight = 0.0
    L0 = model.compute_loss(out, torch.from_numpy(cls[INDEX8]).cuda())
    assert list(L0) == BASE_KEYS
    model.set_hybrid_memory(mem)
    model.hybrid_nce_weight = w
    L1 = model.compute_loss(out, index)                          # ``labels`` = dataset instance indices
    assert list(L1) == BASE_KEYS + NEW_KEYS
    assert torch.equal(bits(L1['ce_loss']), bits(L0['ce_loss'])) and torch.equal(bits(L1['sdm_loss']), bits(L0['sdm_loss']))
    assert int(L1['ce_valid_cnt']) == int(L0['ce_valid_cnt'])
    # the previous total plus weight * term, in that order, bit for bit
    assert torch.equal(L1['total_loss'], L0['total_loss'] + w * L1['hybrid_nce_loss'])
    f = H.forward(x.cpu().numpy(), np.array(INDEX8), valid.cpu().numpy().astype(np.uint8), T0, cls, tau)
    assert int(L1['hybrid_nce_valid_cnt']) == f['n_used'] == S * B and f['loss'] > 0
    assert abs(float(L1['hybrid_nce_loss'].detach()) - f['loss']) <= H.loss_bound(D, 6, tau)
    want, err = H.update_instances(V0, f, m)                     # training with gradients: the entries moved, once
    got = model.hybrid_memory.instances.cpu().numpy()
    assert bool((np.linalg.norm(got.astype(np.float64) - want, axis=1) <= err).all())
    hit = sorted(set(INDEX8))
    assert all(np.abs(got[i] - V0[i]).max() > 0 for i in hit)
    assert all(np.array_equal(got[i].view(np.int32), V0[i].view(np.int32)) for i in range(20) if i not in hit)
    assert torch.equal(bits(model.hybrid_memory.table), bits(H.class_means(got, cls, 6)))
    assert torch.equal(bits(model.hybrid_memory.table[[3, 5]]), bits(T0[[3, 5]]))      # classes 3 and 5 are not in the batch
    model.lora_arena.grad = None
    L1['total_loss'].backward()
    assert float(model.lora_arena.grad.abs().max()) > 0
    assert set(model.state_dict()) == keys_before                # the memory is no parameter and no buffer
    # eval() and no_grad(): the loss is there, the memory stays
    before, before_t = bits(model.hybrid_memory.instances), bits(model.hybrid_memory.table)
    with torch.no_grad():
        Ln = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), index)
    model.eval()
    Le = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), index)
    torch.cuda.synchronize()
    assert 'hybrid_nce_loss' in Ln and 'hybrid_nce_loss' in Le
    assert torch.equal(bits(model.hybrid_memory.instances), before) and torch.equal(bits(model.hybrid_memory.table), before_t)
    # a checkpoint round trip keeps the memory
    path = str(tmp_path / 'memory.pth')
    saved = ck.save_checkpoint(model, None, None, 1, 0.0, model.config, path)
    assert saved['hybrid_memory_state_dict']['hybrid_nce_source'] == source
    other = make(hybrid_nce_weight=w, hybrid_nce_source=source)
    assert other.hybrid_memory is None
    ck.load_checkpoint(path, other)
    assert other.hybrid_memory.instances.is_cuda and torch.equal(bits(other.hybrid_memory.instances), before)
    assert torch.equal(bits(other.hybrid_memory.table), before_t) and other.hybrid_memory.labels.tolist() == CLS20
    with pytest.raises(TypeError, match='HybridMemory'):
        model.set_hybrid_memory(mem.table)
    model.set_hybrid_memory(None)
    assert model.hybrid_memory is None


def test_graphed_step_with_the_hybrid_term_matches_eager():
    """The shapes, warm-up, comparison and tolerance of test_cluster_nce_gpu.test_graphed_step_with_the_cluster_term_matches_eager (2
    warm-up steps and 3 replays against 5 eager steps; the rest of the step has atomics, hence the 2e-3): entries and table live on the
    device and are updated in place, so the replays keep moving them -- and the table stays the exact means of the entries."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_triplet_gpu import _tiny
    meta, state, batch_, build = _tiny()
    images = {m: t.cuda() for m, t in batch_['images'].items()}
    masks = dict(batch_['modality_mask'])
    B = batch_['person_id'].shape[0]
    index = torch.tensor((INDEX8 * B)[:B]).cuda()

    def make():
        m = build(hybrid_nce_weight=0.5, hybrid_nce_source='modalities')
        m.set_hybrid_memory(_hybrid_memory(512, 9))
        gs = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in m.get_learnable_params()]
        return m, StepDriver(m, FusedAdamW(gs, weight_decay=1e-4))

    a, da = make()
    start = a.hybrid_memory.instances.clone()
    tok = a.tokenizer(batch_['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
    tok = {k: v.cuda() for k, v in tok.items()}
    g = GraphedStep(da, images, tok, masks, index, warmup=2)
    for _ in range(3):
        La = g.step(images, tok, masks, index)
    torch.cuda.synchronize()
    b, db = make()
    for _ in range(5):
        Lb = db.step(images, tok, masks, index)
    assert da.opt.step_count == db.opt.step_count == 5
    assert float(Lb['hybrid_nce_loss'].detach()) > 0 and int(Lb['hybrid_nce_valid_cnt']) == int(La['hybrid_nce_valid_cnt']) > 0
    for k in ('total_loss', 'hybrid_nce_loss'):
        va, vb = float(La[k].detach()), float(Lb[k].detach())
        assert abs(va - vb) <= 2e-3 * max(1.0, abs(vb)), k
    ca, cb = a.hybrid_memory.instances.double().cpu(), b.hybrid_memory.instances.double().cpu()
    assert float((cb - start.double().cpu()).abs().max()) > 1e-3
    assert bool(((ca - cb).abs() <= 2e-3 * cb.abs().clamp(min=1.0)).all())
    for mdl in (a, b):
        assert torch.equal(bits(mdl.hybrid_memory.table), bits(H.class_means(mdl.hybrid_memory.instances.cpu().numpy(), np.array(CLS20), 6)))


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
def test_clustering_to_memory_end_to_end():
    """The synthetic identities of test_cluster_nce_gpu.test_clustering_to_memory_end_to_end -> jaccard_dbscan (which leaves noise
    rows) -> HybridMemory.from_clustering: every row is in the memory, a noise row as a class of its own whose table row is its entry."""
    from prcv2025reid_amd.cluster import ClusterParams, jaccard_dbscan
    from prcv2025reid_amd.losses import HybridMemory, hybrid_nce
    g = np.random.default_rng(12)
    cent = 4.0 * g.standard_normal((28, 32))
    X = np.concatenate([np.repeat(cent, 8, axis=0) + 0.5 * g.standard_normal((224, 32)), 4.0 * g.standard_normal((32, 32))])
    X = X[g.permutation(256)].astype(np.float32)
    Xd = dev(X)
    cl = jaccard_dbscan(torch.cat([Xd, torch.zeros_like(Xd)], dim=1), ClusterParams(k1=10, k2=3, eps=0.6, min_samples=4))
    noise = (cl.labels < 0).cpu().numpy()
    assert cl.n_clusters >= 8 and 0 < noise.sum() < 256
    labels, C = cl.hybrid_labels()
    assert C == cl.n_clusters + noise.sum()
    mem = HybridMemory.from_clustering(Xd, cl)
    assert (mem.num_instances, mem.dim, mem.num_classes) == (256, 32, C) and torch.equal(mem.labels.cpu(), labels.cpu())
    V = mem.instances.cpu().numpy()
    T = H.class_means(V, labels.cpu().numpy(), C)
    assert torch.equal(bits(mem.table), bits(T))
    assert torch.equal(bits(mem.table[labels[torch.from_numpy(noise)].cuda()]), bits(V[noise]))      # an outlier's class vector is its entry
    # every image trains: all 256 rows are used
    index = torch.arange(256).cuda()
    loss, n_used, _ = hybrid_nce(Xd, index, mem, update=False)
    f = H.forward(X[None], np.arange(256), None, T, labels.cpu().numpy(), 0.05)
    assert int(n_used) == 256 == f['n_used'] and abs(float(loss) - f['loss']) <= H.loss_bound(32, C, 0.05)
