"""GPU: the cluster-contrast memory loss (csrc/cluster_nce.hip) against the fp64 reference of cluster_nce_ref.py within its derived
bounds, in both library flavours (the kernels are fp32: the same bits in both), and the loss behind the public call, inside the model, in
the graphed step and behind jaccard_dbscan.

Every output and the table live between 32 guard elements that hold a sentinel pattern and must keep it; padded input rows carry NaN in
their padding, padded output rows the sentinel."""
import types

import numpy as np
import pytest
import torch

import cluster_nce_ref as R
from helpers import SENTINEL32

pytestmark = pytest.mark.gpu

GUARD = 32
U = R.U
_CASE = {}                               # case key -> inputs on the CPU with their fp64 reference (shared by the flavours)


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    from prcv2025reid_amd import ops as o, _lib
    _lib.set_flavor(request.param)
    _lib.check(_lib.lib().reid_check_device(0))
    yield o
    _lib.set_flavor('bf16')


def guarded(n, dtype=torch.float32):
    """([GUARD + n + GUARD] sentinel buffer of int32, its middle n elements viewed as ``dtype``)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL32, dtype=torch.int32, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(dtype)


def untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL32).all()) and bool((buf[GUARD + n:] == SENTINEL32).all())


def strided(x, pad):
    """The rows of x [..., D] as a [rows, D] view of a [rows, D + pad] buffer whose padding columns are NaN."""
    x2 = x.reshape(-1, x.shape[-1])
    if pad == 0:
        return x2.contiguous()
    buf = torch.full((x2.shape[0], x2.shape[1] + pad), float('nan'), device=x.device)
    buf[:, :x2.shape[1]] = x2
    return buf[:, :x2.shape[1]]


def bits(t):
    t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t
    return t.detach().cpu().contiguous().view(torch.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Table:
    """table [K, D] between guards."""

    def __init__(self, init):
        K, D = init.shape
        self.buf, flat = guarded(K * D)
        self.t = flat.view(K, D)
        self.t.copy_(torch.as_tensor(init))

    def intact(self):
        return untouched(self.buf, self.t.numel())


def run_fwd(ops, x, labels, valid, table, tau, with_grad=True, pad=0):
    """The forward of x [S, N, D] (numpy) against ``table``; every output between guards."""
    S, N, D = x.shape
    K = table.t.shape[0]
    o = dict(S=S, N=N, D=D, K=K, x2=strided(dev(x), pad), labels=dev(labels), valid=None if valid is None else dev(valid).reshape(-1).contiguous())
    o['b_ws'], o['ws'] = guarded(ops.cluster_nce_ws_floats(S, N, D, K))
    o['b_row_loss'], o['row_loss'] = guarded(S * N)
    o['b_target_cos'], o['target_cos'] = guarded(S * N)
    o['b_result'], o['result'] = guarded(2)
    ops.cluster_nce_fwd(o['x2'], o['labels'], o['valid'], table.t, tau, with_grad, o['ws'], o['row_loss'], o['target_cos'], o['result'], S=S)
    torch.cuda.synchronize()
    for k in ('ws', 'row_loss', 'target_cos', 'result'):
        assert untouched(o['b_' + k], o[k].numel()), f'{k}: guard elements overwritten'
        if k != 'ws':                    # (ws holds pieces only some rows or only the gradient pass write)
            assert not bool((o[k].view(torch.int32) == SENTINEL32).any()), f'{k}: elements not written'
    assert table.intact()
    return o


def run_update(ops, o, table, momentum, mode):
    ops.cluster_nce_update(o['labels'], o['valid'], o['row_loss'], o['target_cos'], o['ws'], table.t, momentum, mode, S=o['S'])
    torch.cuda.synchronize()
    assert table.intact()


def run_bwd(ops, o, dloss, pad=4):
    """dx [S*N, D] between guard rows and sentinel padding columns."""
    rows, D = o['S'] * o['N'], o['D']
    buf = torch.full((rows + 2 * GUARD, D + pad), SENTINEL32, dtype=torch.int32, device='cuda').view(torch.float32)
    dx = buf[GUARD:GUARD + rows, :D]
    ops.cluster_nce_bwd(o['ws'], o['result'], torch.tensor([dloss], dtype=torch.float32, device='cuda'), dx, S=o['S'])
    torch.cuda.synchronize()
    raw = buf.view(torch.int32)
    assert bool((raw[:GUARD] == SENTINEL32).all()) and bool((raw[GUARD + rows:] == SENTINEL32).all()), 'dx: guard rows overwritten'
    assert bool((raw[GUARD:GUARD + rows, D:] == SENTINEL32).all()), 'dx: padding columns overwritten'
    assert not bool((raw[GUARD:GUARD + rows, :D] == SENTINEL32).any()), 'dx: elements not written'
    return dx


def check_forward(o, f, D, K, tau, exact=False):
    """Loss, row losses, target cosines and n_used of a forward against the reference ``f``; returns the measured maxima."""
    rl, tc = o['row_loss'].double().cpu().numpy(), o['target_cos'].double().cpu().numpy()
    assert float(o['result'][1]) == f['n_used']
    e_row = np.abs(rl - f['row_loss']).max()
    e_cos = np.abs(tc - f['target_cos']).max()
    e_loss = abs(float(o['result'][0]) - f['loss'])
    assert e_row <= R.row_bound(D, K, tau, exact), (e_row, R.row_bound(D, K, tau, exact))
    assert e_cos <= R.cos_bound(D, exact), (e_cos, R.cos_bound(D, exact))
    assert e_loss <= R.loss_bound(D, K, tau, exact), (e_loss, R.loss_bound(D, K, tau, exact))
    assert not rl[~f['used']].any() and not tc[~f['used']].any()
    return e_row, e_cos, e_loss


def check_dx(dx, f, D, K, tau, dloss, table, exact=False):
    """dx within its per-row bound of the reference; returns 'max |error| / max |dx| / largest bound' for the log."""
    g = dx.double().cpu().numpy()
    want = f['dx'] * dloss                                       # (the reference was formed with dloss = 1)
    bound = R.dx_bound(f, D, K, tau, dloss, float(np.abs(table).max()), exact)[:, None]
    assert bool((np.abs(g - want) <= bound).all()), float((np.abs(g - want) / bound).max())
    assert not g[~f['used']].any()
    return f'{np.abs(g - want).max():.3e} / {np.abs(want).max():.3e} / {bound[f["used"]].max() if f["used"].any() else 0.0:.3e}'


# ---------------------------------------------------------------------------------------------------------------- 1. one batch
def shape_of(ops, name, D, which):
    """The K or R a symbolic name stands for: the tiles and the split boundaries come from cluster_nce_plan."""
    row_tile, class_tile, _, _ = ops.cluster_nce_plan(1, 1, D)
    if which == 'K':
        if name in ('split2', 'split3'):
            want = int(name[-1])
            K = 1
            while ops.cluster_nce_plan(1, K, D)[2] < want:
                K += 1
            assert ops.cluster_nce_plan(1, K, D)[2] == want and ops.cluster_nce_plan(1, K - 1, D)[2] == want - 1
            return K
        if name == 'tiles2':             # the first K at which a workgroup walks two class tiles (for 1 row as for 65: the same plan)
            K = 1
            while ops.cluster_nce_plan(1, K, D)[3] < 2:
                K += class_tile
            assert ops.cluster_nce_plan(1, K, D)[3] == 2 and ops.cluster_nce_plan(1, K - 1, D)[3] == 1
            assert ops.cluster_nce_plan(row_tile + 1, K, D)[3] == 2
            return K
        return {'one': 1, 'two': 2, 'tile-1': class_tile - 1, 'tile': class_tile, 'tile+1': class_tile + 1}[name]
    return {'one': (1, 1), 'three': (3, 1), 'tile-1': (3, (row_tile - 1) // 3), 'tile+1': (1, row_tile + 1)}[name]      # (S, N)


@pytest.mark.parametrize('rows', ['one', 'three', 'tile-1', 'tile+1'])
@pytest.mark.parametrize('classes', ['one', 'two', 'tile-1', 'tile', 'tile+1', 'split2', 'split3', 'tiles2'])
@pytest.mark.parametrize('D', [32, 96, 512])
def test_kernels_against_the_reference(ops, D, classes, rows):
    K = shape_of(ops, classes, D, 'K')
    S, N = shape_of(ops, rows, D, 'R')
    assert S * N in (1, 3, ops.cluster_nce_plan(1, 1, D)[0] - 1, ops.cluster_nce_plan(1, 1, D)[0] + 1)
    tau, pad, dloss = 0.05, (4 if D != 96 else 0), -0.7
    key = (S, N, D, K)
    if key not in _CASE:
        x, labels, valid, table = R.random_case(S, N, D, K, 1000 * D + 10 * K + N)
        _CASE[key] = (x, labels, valid, table, R.forward(x, labels, valid, table, tau))
    x, labels, valid, table, f = _CASE[key]
    assert f['n_used'] > 0 and (N < 5 or K < 2 or not f['used'].all())
    # what is compared stands far above what it is compared within: a loss or a gradient of zeros, a dropped class tile or split fails
    s_row, s_dx = R.signal_ratios(f, D, K, tau, dloss, float(np.abs(table).max()))
    assert K == 1 or (s_row >= 5 and s_dx >= 5), (s_row, s_dx)
    assert K < 63 or (s_row >= 500 and s_dx >= 50), (s_row, s_dx)
    t = Table(table)
    o = run_fwd(ops, x, labels, valid, t, tau, True, pad)
    assert torch.equal(bits(t.t), bits(table))                   # the forward reads the table only
    e_row, e_cos, e_loss = check_forward(o, f, D, K, tau)
    dx = run_bwd(ops, o, dloss)
    m_dx = check_dx(dx, f, D, K, tau, dloss, table)
    print(f'measured D={D} K={K} R={S * N}: row {e_row:.3e} / {R.row_bound(D, K, tau):.3e}  cos {e_cos:.3e} / {R.cos_bound(D):.3e}  '
          f'loss {e_loss:.3e} / {R.loss_bound(D, K, tau):.3e}  dx error / largest |dx| / bound {m_dx}  '
          f'(largest row loss {f["row_loss"].max():.3e})')
    assert K == 1 or float(dx.abs().max()) > 0
    # without gradients: one pass over the table, the same loss bits
    o2 = run_fwd(ops, x, labels, valid, t, tau, False, pad)
    assert torch.equal(bits(o2['result']), bits(o['result'])) and torch.equal(bits(o2['row_loss']), bits(o['row_loss']))


def test_exact_operands(ops):
    """Entries in {0, +-0.5, +-1}, exactly unit rows, 1 / tau = 16: every norm, dot product and logit is exact; only exp, log and the sums
    round, and the bound is the much tighter one of that."""
    N, D, K, tau = 70, 64, 100, 0.0625
    x, labels, table = R.exact_case(N, D, K, 5)
    f = R.forward(x, labels, None, table, tau)
    t = Table(table)
    o = run_fwd(ops, x, labels, None, t, tau)
    assert np.array_equal(o['target_cos'].cpu().numpy().astype(np.float64), f['target_cos'])       # exact, not merely close
    e_row, _, e_loss = check_forward(o, f, D, K, tau, exact=True)
    assert 10 * R.row_bound(D, K, tau, exact=True) < R.row_bound(D, K, tau)
    r_dx = check_dx(run_bwd(ops, o, 1.0), f, D, K, tau, 1.0, table, exact=True)
    print(f'measured exact D={D} K={K} R={N}: row {e_row:.3e} / {R.row_bound(D, K, tau, True):.3e}  loss {e_loss:.3e} / '
          f'{R.loss_bound(D, K, tau, True):.3e}  dx error / largest |dx| / bound {r_dx}')


@pytest.mark.parametrize('D', [32, 512])
def test_target_and_maximum_in_different_class_tiles(ops, D):
    """K at which every workgroup walks TWO class tiles (cluster_nce_plan's class tiles per split = 2): the running maximum and sum are
    carried from one tile to the next, and the gradient pass stages the second tile over the p tile of the first.  Row 0 sits on a
    centroid of its split's second tile with its label in the first, row 1 the other way round, row 2 has its maximum in another
    split than its label, row 3 two equal maxima in the two tiles of one split; the other rows are random directions."""
    row_tile, class_tile, _, _ = ops.cluster_nce_plan(1, 1, D)
    K = 1
    while ops.cluster_nce_plan(1, K, D)[3] < 2:
        K += class_tile
    S, N, tau, dloss = 1, 12, 0.05, 1.3
    _, _, splits, per_split = ops.cluster_nce_plan(S * N, K, D)
    assert per_split == 2 and splits * per_split * class_tile >= K > (splits - 1) * per_split * class_tile
    x, labels, _, table = R.random_case(S, N, D, K, 5 + D)
    T = class_tile
    labels[:4] = [3, T + 9, 5, 2 * T + 1]                        # tiles 0, 1, 0, 2 (splits 0, 0, 0, 1)
    x[0, 0] = 2.0 * table[T + 7]                                 # maximum in tile 1, label in tile 0 (one split)
    x[0, 1] = 0.5 * table[11]                                    # maximum in tile 0, label in tile 1
    x[0, 2] = 1.5 * table[4 * T + 2]                             # maximum in tile 4 = split 2
    table[T + 20] = table[20]                                    # two equal centroids in tiles 0 and 1
    x[0, 3] = table[20]
    f = R.forward(x, labels, None, table, tau)
    cos = f['xhat'][:4] @ table.astype(np.float64).T
    assert [int(c.argmax()) // T for c in cos[:3]] == [1, 0, 4] and cos[3, 20] == cos[3, T + 20] == cos[3].max()
    assert f['row_loss'][:4].min() > 10 and min(R.signal_ratios(f, D, K, tau, dloss, float(np.abs(table).max()))) >= 100
    t = Table(table)
    o = run_fwd(ops, x, labels, None, t, tau, True, 4)
    e_row, e_cos, e_loss = check_forward(o, f, D, K, tau)
    m_dx = check_dx(run_bwd(ops, o, dloss), f, D, K, tau, dloss, table)
    print(f'measured two tiles per split D={D} K={K}: row {e_row:.3e} / {R.row_bound(D, K, tau):.3e}  loss {e_loss:.3e} / '
          f'{R.loss_bound(D, K, tau):.3e}  dx error / largest |dx| / bound {m_dx}')
    o2 = run_fwd(ops, x, labels, None, t, tau, False, 0)
    assert torch.equal(bits(o2['row_loss']), bits(o['row_loss']))


def test_graph_replay_equals_eager_bit_for_bit(ops):
    """The term is atomic-free: forward, update and backward captured once as ONE linear chain on the capture stream and replayed three
    times give the bits of three eager rounds -- loss, row losses, dx and the table, which every round moves."""
    S, N, D, K, tau, m = 3, 21, 96, 65, 0.05, 0.1
    x, labels, valid, table = R.random_case(S, N, D, K, 17)
    xd, ld, vd = dev(x).reshape(S * N, D).contiguous(), dev(labels), dev(valid).reshape(-1).contiguous()
    dloss = torch.tensor([0.75], device='cuda')

    def buffers():
        return dict(table=dev(table).clone(), ws=torch.empty(ops.cluster_nce_ws_floats(S, N, D, K), device='cuda'), row_loss=torch.empty(S * N, device='cuda'),
                    tcos=torch.empty(S * N, device='cuda'), res=torch.empty(2, device='cuda'), dx=torch.empty(S * N, D, device='cuda'))

    def round_(b):
        ops.cluster_nce_fwd(xd, ld, vd, b['table'], tau, True, b['ws'], b['row_loss'], b['tcos'], b['res'], S=S)
        ops.cluster_nce_update(ld, vd, b['row_loss'], b['tcos'], b['ws'], b['table'], m, 'mean', S=S)
        ops.cluster_nce_bwd(b['ws'], b['res'], dloss, b['dx'], S=S)

    eager, outs = buffers(), []
    for _ in range(3):
        round_(eager)
        torch.cuda.synchronize()
        outs.append([bits(eager[k]) for k in ('res', 'row_loss', 'dx', 'table')])
    assert not torch.equal(outs[0][3], outs[2][3]) and not torch.equal(outs[0][0], outs[2][0])      # the rounds differ: the table moves
    graphed = buffers()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        round_(graphed)
    graphed['table'].copy_(dev(table))                               # (capture launches nothing; start from the same table all the same)
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        for k, want in zip(('res', 'row_loss', 'dx', 'table'), outs[i]):
            assert torch.equal(bits(graphed[k]), want), (i, k)


def test_one_class_gives_zero_loss_and_zero_gradient(ops):
    x, labels, valid, table = R.make_case(2, 9, 96, 1, 4, noise=False)
    t = Table(table)
    o = run_fwd(ops, x, labels, valid, t, 0.05)
    assert float(o['result'][0]) == 0.0 and float(o['result'][1]) == int((valid != 0).sum()) and float(o['row_loss'].abs().max()) == 0.0
    assert float(run_bwd(ops, o, 2.5).abs().max()) == 0.0


def test_small_temperature_stays_finite(ops):
    """tau = 0.01 with x^ = C_y: a logit of 100 next to -100 (and 0s)."""
    D, K = 32, 70
    table = np.zeros((K, D), dtype=np.float32)
    table[0, 0], table[1, 0] = 1.0, -1.0
    table[2:, 1] = 1.0
    x = np.zeros((1, 2, D), dtype=np.float32)
    x[0, 0, 0], x[0, 1, 0] = 3.0, 3.0
    labels = np.array([0, 1])
    f = R.forward(x, labels, None, table, 0.01)
    t = Table(table)
    o = run_fwd(ops, x, labels, None, t, 0.01)
    rl = o['row_loss'].cpu().numpy()
    assert np.isfinite(rl).all() and np.isfinite(float(o['result'][0])) and rl[0] == 0.0 and abs(rl[1] - 200.0) <= R.row_bound(D, K, 0.01)
    check_forward(o, f, D, K, 0.01)
    assert bool(torch.isfinite(run_bwd(ops, o, 1.0)).all())


def test_zero_row_hits_the_clamp(ops):
    S, N, D, K, tau = 1, 6, 32, 5, 0.05
    x, labels, valid, table = R.make_case(S, N, D, K, 8, noise=False)
    x[0, 2] = 0.0
    f = R.forward(x, labels, None, table, tau)
    assert f['inv'][2] == 1e12 and abs(f['row_loss'][2] - np.log(K)) <= 1e-12
    t = Table(table)
    o = run_fwd(ops, x, labels, None, t, tau)
    check_forward(o, f, D, K, tau)
    dx = run_bwd(ops, o, 1.0)
    assert bool(torch.isfinite(dx).all()) and float(dx[2].abs().max()) > 1e9
    check_dx(dx, f, D, K, tau, 1.0, table)


def test_unused_rows_and_a_batch_without_a_used_row(ops):
    S, N, D, K, tau = 3, 7, 32, 4, 0.05
    x, labels, valid, table = R.make_case(S, N, D, K, 2)
    f = R.forward(x, labels, valid, table, tau)
    assert labels[1] == -1 and labels[N - 2] == K and not valid.all() and 0 < f['n_used'] < S * N
    t = Table(table)
    o = run_fwd(ops, x, labels, valid, t, tau)
    check_forward(o, f, D, K, tau)
    dx = run_bwd(ops, o, 1.0)
    assert float(dx[torch.from_numpy(~f['used']).cuda()].abs().max()) == 0.0 and float(dx.abs().max()) > 0
    for lab, val in ((labels, np.zeros((S, N), dtype=np.uint8)), (np.full(N, K), None), (np.full(N, -1), valid)):
        for mode in ('mean', 'hard'):
            t = Table(table)
            o = run_fwd(ops, x, lab, val, t, tau)
            assert o['result'].tolist() == [0.0, 0.0] and float(o['row_loss'].abs().max()) == 0.0
            run_update(ops, o, t, 0.1, mode)
            assert torch.equal(bits(t.t), bits(table))
            assert float(run_bwd(ops, o, 3.0).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. the update
@pytest.mark.parametrize('mode', ['mean', 'hard'])
def test_update_against_the_reference(ops, mode):
    """Label 0 has three contributing rows spread over two sides (rows 0 and 3 of side 0, row 15 of side 1; its rows 7, 8 and 11 are
    invalid): the ascending order matters, since the blend does not commute.  Labels 5 and 6 are absent; row 12 (label 3) is NaN."""
    S, N, D, K, tau, m = 2, 8, 96, 7, 0.05, 0.3
    x, _, _, table = R.make_case(S, N, D, K, 6, noise=False, spread=4.0)
    labels2 = np.array([0, 1, 2, 0, 3, 4, 1, 0])
    valid = np.ones((S, N), dtype=np.uint8)
    valid[0, 7] = valid[1, 0] = valid[1, 3] = 0
    x[1, 4, 7] = np.nan                                          # row 12: used, not contributing; label 3 keeps row 4
    f = R.forward(x, labels2, valid, table, tau)
    con = R.contributing(f)
    assert [r for r in range(S * N) if con[r] and f['y'][r] == 0] == [0, 3, 15] and f['used'][12] and not con[12]
    assert R.hard_pick_gap(f) > 2 * R.cos_bound(D)
    want, err = R.update(table, f, m, mode)
    c = table[0].astype(np.float64)
    for r in (15, 3, 0):                                         # the reverse order gives another centroid
        c = m * c + (1 - m) * f['xhat'][r]
        c = c / np.linalg.norm(c)
    assert mode == 'hard' or np.abs(c - want[0]).max() > 1e-3
    t = Table(table)
    o = run_fwd(ops, x, labels2, valid, t, tau)
    assert not np.isfinite(float(o['result'][0]))                # the NaN row is used: the step driver skips such a step
    run_update(ops, o, t, m, mode)
    got = t.t.double().cpu().numpy()
    assert np.isfinite(got).all()
    dev2 = np.linalg.norm(got - want, axis=1)
    print(f'measured update {mode} D={D}: centroid deviation {dev2.max():.3e}, largest deviation / bound {(dev2[:5] / err[:5]).max():.3e} (bounds up to {err.max():.3e})')
    assert bool((dev2 <= err).all()), (dev2 / np.maximum(err, 1e-300)).max()
    for k in range(K):
        moved = not torch.equal(bits(t.t[k]), bits(table[k]))
        assert moved == (k in (0, 1, 2, 3, 4)), k                # labels 5 and 6 are absent: their bits stay
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= R.e_n(D) + U
    # the NaN row moved nothing: the same table as without it
    valid2 = valid.copy(); valid2[1, 4] = 0
    t2 = Table(table)
    run_update(ops, run_fwd(ops, np.nan_to_num(x), labels2, valid2, t2, tau), t2, m, mode)
    assert torch.equal(bits(t2.t), bits(t.t))


def test_leader_beyond_the_first_64_rows(ops):
    """130 rows: label 2's only contributing row is row 120, label 1's are rows 121 .. 129; label 0's spread over all three 64-row groups."""
    S, N, D, K, tau = 1, 130, 32, 3, 0.05
    x, _, _, table = R.make_case(S, N, D, K, 9, noise=False)
    labels = np.array([0] * 120 + [2] + [1] * 9)
    f = R.forward(x, labels, None, table, tau)
    want, err = R.update(table, f, 0.5, 'mean')                  # (m / nu < 1 for these blends: the bound stays linear in the rows)
    t = Table(table)
    o = run_fwd(ops, x, labels, None, t, tau)
    check_forward(o, f, D, K, tau)
    run_update(ops, o, t, 0.5, 'mean')
    assert bool((np.linalg.norm(t.t.double().cpu().numpy() - want, axis=1) <= err).all())
    assert all(not torch.equal(bits(t.t[k]), bits(table[k])) for k in range(K))


def test_backward_is_independent_of_a_later_forward_and_update(ops):
    S, N, D, K, tau = 3, 21, 96, 65, 0.05
    x, labels, valid, table = R.make_case(S, N, D, K, 31)
    x2, labels2, valid2, _ = R.make_case(S, N, D, K, 32)
    runs = []
    for later in (False, True):
        t = Table(table)
        o = run_fwd(ops, x, labels, valid, t, tau)
        if later:
            run_update(ops, o, t, 0.1, 'mean')
            o2 = run_fwd(ops, x2, labels2, valid2, t, tau)
            run_update(ops, o2, t, 0.1, 'hard')
            assert not torch.equal(bits(t.t), bits(table))
        runs.append(bits(run_bwd(ops, o, 1.25)))
    assert torch.equal(runs[0], runs[1]) and bool((runs[0] != 0).any())


def test_two_runs_give_the_same_bits(ops):
    S, N, D, K, tau = 3, 21, 512, 129, 0.05
    runs = []
    for _ in range(2):
        _, _, _, table = R.make_case(S, N, D, K, 40)
        t, out = Table(table), []
        for s in (1, 2, 3):
            x, labels, valid, _ = R.make_case(S, N, D, K, 40 + s)
            o = run_fwd(ops, x, labels, valid, t, tau)
            run_update(ops, o, t, 0.1, 'mean' if s != 2 else 'hard')
            out += [bits(o['row_loss']), bits(o['target_cos']), bits(o['result']), bits(run_bwd(ops, o, -2.0)), bits(t.t)]
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and bool((runs[0][-1] != 0).any())


# ---------------------------------------------------------------------------------------------------------------- 3. centroids
def test_from_labels_against_the_reference(ops):
    from prcv2025reid_amd import losses
    g = np.random.default_rng(3)
    n, D, K = 150, 96, 9
    labels = g.integers(-1, K, size=n)
    labels[:K] = np.arange(K)
    feats = (g.standard_normal((n, D)) + 2.0 * g.standard_normal((K + 1, D))[labels + 1]).astype(np.float32)
    want, err = R.centroids(feats, labels)
    mem = losses.ClusterMemory.from_labels(dev(feats), dev(labels))
    assert (mem.num_clusters, mem.dim) == (K, D) and mem.centroids.shape == (K, D) and mem.centroids.is_cuda
    dev_c = np.linalg.norm(mem.centroids.double().cpu().numpy() - want, axis=1)
    print(f'measured centroids D={D}: deviation {dev_c.max():.3e}, largest deviation / bound {(dev_c / err).max():.3e} (bounds up to {err.max():.3e})')
    assert bool((dev_c <= err).all())
    # a row view with a leading dimension, and int32 labels
    wide = torch.full((n, D + 4), float('nan'), device='cuda'); wide[:, :D] = dev(feats)
    mem2 = losses.ClusterMemory.from_labels(wide[:, :D], dev(labels.astype(np.int32)))
    assert torch.equal(bits(mem2.centroids), bits(mem.centroids))
    with pytest.raises(ValueError, match='cluster 4 has no row'):
        losses.ClusterMemory.from_labels(dev(feats), dev(np.where(labels == 4, -1, labels)))
    with pytest.raises(ValueError, match='no row has a cluster'):
        losses.ClusterMemory.from_labels(dev(feats), dev(np.full(n, -1)))
    with pytest.raises(ValueError, match='feats'):
        losses.ClusterMemory.from_labels(dev(feats), dev(labels[:-1]))


def test_violated_requirements_are_refused_and_write_nothing(ops):
    import test_cluster_nce_cpu as T
    from prcv2025reid_amd import _lib
    S, N, D, K = 2, 5, 32, 4
    h = _lib.lib()
    t = {n: torch.full((k,), SENTINEL32, dtype=torch.int32, device='cuda') for n, k in
         (('x', 2 * S * N * D), ('table', 2 * K * D), ('ws', 4096), ('row_loss', S * N), ('target_cos', S * N), ('result', 2), ('dloss', 1),
          ('dx', 2 * S * N * D), ('feats', 2 * S * N * D))}
    t['labels'] = torch.zeros(N, dtype=torch.int64, device='cuda')
    t['order'] = torch.zeros(S * N, dtype=torch.int64, device='cuda')
    t['offsets'] = torch.zeros(K + 1, dtype=torch.int64, device='cuda')
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
        assert bool((v == (0 if n in ('labels', 'order', 'offsets') else SENTINEL32)).all()), f'{n} was written'


# ---------------------------------------------------------------------------------------------------------------- 4. public call
def test_public_call_update_flags_and_errors(ops):
    from prcv2025reid_amd import losses, _lib
    S, N, D, K, tau = 3, 7, 96, 5, 0.05
    x, labels, valid, table = R.random_case(S, N, D, K, 21)
    f = R.forward(x, labels, valid, table, tau)
    assert min(R.signal_ratios(f, D, K, tau, -1.5, float(np.abs(table).max()))) >= 100      # loss and gradient far above their bounds
    mem = losses.ClusterMemory(K, D, 'cuda')
    mem.load_state({'centroids': torch.from_numpy(table)})
    before = bits(mem.centroids)
    xa = dev(x).requires_grad_(True)
    loss, n_used, rows = losses.cluster_nce(xa, dev(labels), mem, valid=dev(valid) != 0, update=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(mem.centroids), before)              # update=False
    assert int(n_used) == f['n_used'] and rows['row_loss'].shape == (S, N) and rows['target_cos'].shape == (S, N)
    assert abs(float(loss.detach()) - f['loss']) <= R.loss_bound(D, K, tau)
    rows['row_loss'].zero_(); rows['target_cos'].zero_()         # copies: writing into them must not reach the backward
    (loss * -1.5).backward()
    assert xa.grad.shape == x.shape
    check_dx(xa.grad.reshape(S * N, D), f, D, K, tau, -1.5, table)
    with torch.no_grad():                                        # no_grad: the loss is there, the table stays
        loss2, _, _ = losses.cluster_nce(dev(x), dev(labels), mem, valid=dev(valid))
    torch.cuda.synchronize()
    assert torch.equal(bits(mem.centroids), before) and torch.equal(bits(loss2), bits(loss))
    loss3, _, _ = losses.cluster_nce(dev(x), dev(labels), mem, valid=dev(valid), momentum=0.2, mode='hard')
    torch.cuda.synchronize()
    want, err = R.update(table, f, 0.2, 'hard')
    assert R.hard_pick_gap(f) > 2 * R.cos_bound(D) and not torch.equal(bits(mem.centroids), before) and torch.equal(bits(loss3), bits(loss))
    assert bool((np.linalg.norm(mem.centroids.double().cpu().numpy() - want, axis=1) <= err).all())
    moved = bits(mem.centroids)
    l1, n1, r1 = losses.cluster_nce(dev(x)[0], dev(labels), mem, valid=dev(valid)[0], update=False)      # one side, flat
    assert r1['row_loss'].shape == (N,) and int(n1) == int(f['used'][:N].sum())
    with pytest.raises(_lib.ReidHipError, match='D='):
        losses.cluster_nce(dev(x)[..., :32], dev(labels), mem)
    with pytest.raises(TypeError, match='ClusterMemory'):
        losses.cluster_nce(dev(x), dev(labels), mem.centroids)
    for bad, text in ((dict(temperature=0.0), 'temperature'), (dict(momentum=1.5), 'momentum'), (dict(mode='soft'), 'mode')):
        with pytest.raises(ValueError, match=text):
            losses.cluster_nce(dev(x), dev(labels), mem, **bad)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.cluster_nce(torch.from_numpy(x), torch.from_numpy(labels), mem)
    assert torch.equal(bits(mem.centroids), moved)               # a refused call moves nothing


def test_five_sgd_steps_follow_the_reference_trajectory(ops):
    """A free [64, 32] tensor against 8 clusters, tau = 0.2, lr = 0.2, momentum 0.5, 'mean'.  The fp64 reference runs its own
    trajectory; the bounds are chained: with a = the largest row deviation of x and b = the largest centroid deviation so far,
      loss      loss_bound + a * 2 / (tau xmin) + b * 2 / tau          (|d row_loss / dx| = |H| <= 2 / (tau |x|); sum_c |p_c - [c = y]| <= 2)
      gradient  sqrt(D) * dx_bound + (Lx a + Lc b) / n per row, Lx = (1 / tau^2 + 6 / tau) / xmin^2 (the covariance of unit vectors has
                norm <= 1: dG/dx^ <= 1 / tau^2; the projection and the two 1 / |x| factors of |G| <= 2 / tau), Lc = (2 / tau^2 + 2 / tau) / xmin
      x         a' = a + lr * (that) + 2 u xmax (the fp32 step);  table: the reference's recurrence with err0 = b and x^ off by a / xmin."""
    from prcv2025reid_amd import losses
    N, D, K, tau, lr, m = 64, 32, 8, 0.2, 0.2, 0.5
    x, labels, _, table = R.make_case(1, N, D, K, 77, noise=False)
    x = (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    mem = losses.ClusterMemory(K, D, 'cuda')
    mem.load_state({'centroids': torch.from_numpy(table)})
    xg = dev(x[0]).requires_grad_(True)
    x64, C64 = x.astype(np.float64), table.astype(np.float64)
    a, b = 0.0, np.zeros(K)
    Lx = lambda xmin: (1 / tau ** 2 + 6 / tau) / xmin ** 2
    Lc = lambda xmin: (2 / tau ** 2 + 2 / tau) / xmin
    for step in range(5):
        f = R.forward(x64, labels, None, C64, tau)
        xmin = float(np.linalg.norm(x64[0], axis=1).min()) - a
        assert xmin > 0.5
        loss, n_used, _ = losses.cluster_nce(xg, dev(labels), mem, temperature=tau, momentum=m)
        loss.backward()
        e_loss = abs(float(loss.detach()) - f['loss'])
        bound = R.loss_bound(D, K, tau) + a * 2 / (tau * xmin) + b.max() * 2 / tau
        print(f'step {step}: loss {float(loss.detach()):.6f} error {e_loss:.3e} bound {bound:.3e}')
        assert int(n_used) == N and e_loss <= bound, (step, e_loss, bound)
        C64, b_new = R.update(C64, f, m, 'mean', err0=b, xhat_dev=a / xmin)
        dev_c = np.linalg.norm(mem.centroids.double().cpu().numpy() - C64, axis=1)
        assert bool((dev_c <= b_new).all()), (step, (dev_c / b_new).max())
        g_dev = float(np.sqrt(D)) * float(R.dx_bound(f, D, K, tau, 1.0, float(np.abs(C64).max())).max()) + (Lx(xmin) * a + Lc(xmin) * b.max()) / N
        with torch.no_grad():
            xg.add_(xg.grad, alpha=-lr)
            xg.grad = None
        x64 = x64 - lr * f['dx'][None]
        a = a + lr * g_dev + 2 * U * float(np.linalg.norm(x64[0], axis=1).max())
        b = b_new
        dev_x = float(np.linalg.norm(xg.detach().double().cpu().numpy() - x64[0], axis=1).max())
        assert dev_x <= a, (step, dev_x, a)
    assert f['loss'] < R.forward(x, labels, None, table, tau)['loss']          # the steps descend


# ---------------------------------------------------------------------------------------------------------------- 5. model level
BASE_KEYS = ['total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt']
NEW_KEYS = ['cluster_nce_loss', 'cluster_nce_valid_cnt']


def _tiny8(**over):
    """The tiny frozen model with a batch of 8 instances (4 identities x 2, every modality present), as tests/test_loss_terms_gpu.py."""
    from helpers import load_case, case_inputs
    from prcv2025reid_amd.synthetic import synthetic_batch
    from test_model_gpu import build_model
    z, meta = load_case('tiny_train_frozen')
    cfg, arch, state, _, _ = case_inputs(meta)
    batch = synthetic_batch(4, 2, arch, seed=7, mask_drop=0.0, num_classes=int(meta['num_classes']))
    return meta, state, batch, (lambda **kw: build_model(meta, state, True, **{**over, **kw}))


def _inputs(batch):
    return ({m: t.cuda() for m, t in batch['images'].items()}, {m: t.cuda() for m, t in batch['modality_mask'].items()}, batch['person_id'].cuda())


def _memory(K, D, seed):
    from prcv2025reid_amd.losses import ClusterMemory
    g = np.random.default_rng(seed)
    t = g.standard_normal((K, D))
    mem = ClusterMemory(K, D, 'cuda')
    mem.load_state({'centroids': torch.from_numpy((t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32))})
    return mem


def _term_inputs(out, source):
    """(x [S, B, D], valid [S, B]) the model's term must have used."""
    raw, fm = out['raw_modality_features'], out['feature_masks']
    if source == 'bn':
        return out['bn_features'].detach()[None], (torch.stack([t.cuda() for t in fm.values()]) > 0).any(0)[None]
    mods = [m for m in raw if m in fm]
    mods = [m for m in mods if m == 'vis'] + [m for m in mods if m != 'vis']
    assert mods[0] == 'vis' and len(mods) >= 2
    return torch.stack([raw[m].detach() for m in mods]), torch.stack([fm[m].cuda() > 0 for m in mods])


def test_weight_zero_is_the_model_without_the_fields():
    from helpers import case_config
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel, apply_reference_freeze
    meta, state, batch, make = _tiny8()
    images, masks, labels = _inputs(batch)
    cfg = case_config(meta, device='cuda')
    cfg.compute_dtype = 'bf16'
    bare = types.SimpleNamespace(**{k: v for k, v in vars(cfg).items() if not k.startswith('cluster_nce_')})
    assert not hasattr(bare, 'cluster_nce_weight') and hasattr(cfg, 'cluster_nce_weight')
    old = CLIPBasedMultiModalReIDModel(bare)
    old.set_num_classes(int(meta['num_classes'])); old.load_state_dict(state, strict=True); apply_reference_freeze(old)
    old.contrastive_weight = meta['contrastive_weight']; old.set_epoch(2); old.train(True)
    L_old = old.compute_loss(old(images=images, texts=batch['texts'], modality_masks=masks), labels)
    new = make(cluster_nce_weight=0.0, cluster_nce_source='modalities')
    L_new = new.compute_loss(new(images=images, texts=batch['texts'], modality_masks=masks), labels)
    assert list(L_old) == list(L_new) == BASE_KEYS and new.cluster_memory is None and old.cluster_memory is None
    for k in BASE_KEYS[:-1]:
        assert torch.equal(bits(L_old[k]), bits(L_new[k])), k
    assert int(L_old['ce_valid_cnt']) == int(L_new['ce_valid_cnt'])


@pytest.mark.parametrize('source', ['bn', 'modalities'])
def test_model_loss_with_the_cluster_term(source, tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    meta, state, batch, make = _tiny8()
    images, masks, labels = _inputs(batch)
    w, tau, m = 0.5, 0.05, 0.1
    model = make(cluster_nce_weight=w, cluster_nce_source=source)
    assert model.cluster_memory is None and (model.cluster_nce_temperature, model.cluster_nce_momentum, model.cluster_nce_mode) == (tau, m, 'mean')
    keys_before = set(model.state_dict())
    out = model(images=images, texts=batch['texts'], modality_masks=masks)
    with pytest.raises(ValueError, match='needs a cluster memory'):
        model.compute_loss(out, labels)
    model.cluster_nce_weight = 0.0
    L0 = model.compute_loss(out, labels)
    assert list(L0) == BASE_KEYS
    x, valid = _term_inputs(out, source)
    S, B, D = x.shape
    K = 6                                                        # labels 0 .. 3 are in the batch, clusters 4 and 5 are absent
    mem = _memory(K, D, 5)
    table = mem.centroids.cpu().numpy().copy()
    model.set_cluster_memory(mem)
    model.cluster_nce_weight = w
    L1 = model.compute_loss(out, labels)
    assert list(L1) == BASE_KEYS + NEW_KEYS
    # the previous total plus weight * term, in that order, bit for bit
    assert torch.equal(L1['total_loss'], L0['total_loss'] + w * L1['cluster_nce_loss'])
    f = R.forward(x.cpu().numpy(), labels.cpu().numpy(), valid.cpu().numpy().astype(np.uint8), table, tau)
    assert int(L1['cluster_nce_valid_cnt']) == f['n_used'] == S * B and f['loss'] > 0
    assert abs(float(L1['cluster_nce_loss'].detach()) - f['loss']) <= R.loss_bound(D, K, tau)
    want, err = R.update(table, f, m, 'mean')                    # training with gradients: the centroids moved, once
    got = model.cluster_memory.centroids.double().cpu().numpy()
    assert bool((np.linalg.norm(got - want, axis=1) <= err).all()) and np.abs(got[:4] - table[:4]).max() > 0
    assert torch.equal(bits(model.cluster_memory.centroids[4:]), bits(table[4:]))
    model.lora_arena.grad = None
    L1['total_loss'].backward()
    assert float(model.lora_arena.grad.abs().max()) > 0
    assert set(model.state_dict()) == keys_before                # the memory is no parameter and no buffer
    # eval() and no_grad(): the loss is there, the memory stays
    before = bits(model.cluster_memory.centroids)
    with torch.no_grad():
        Ln = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), labels)
    model.eval()
    Le = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), labels)
    torch.cuda.synchronize()
    assert 'cluster_nce_loss' in Ln and 'cluster_nce_loss' in Le and torch.equal(bits(model.cluster_memory.centroids), before)
    # a checkpoint round trip keeps the memory
    path = str(tmp_path / 'memory.pth')
    saved = ck.save_checkpoint(model, None, None, 1, 0.0, model.config, path)
    assert saved['cluster_memory_state_dict']['cluster_nce_source'] == source
    other = make(cluster_nce_weight=w, cluster_nce_source=source)
    assert other.cluster_memory is None
    ck.load_checkpoint(path, other)
    assert other.cluster_memory.centroids.is_cuda and torch.equal(bits(other.cluster_memory.centroids), before)
    with pytest.raises(TypeError, match='ClusterMemory'):
        model.set_cluster_memory(mem.centroids)
    model.set_cluster_memory(None)
    assert model.cluster_memory is None


def test_graphed_step_with_the_cluster_term_matches_eager():
    """The shapes, warm-up, comparison and tolerance of test_center_gpu.test_graphed_step_with_the_center_term_matches_eager (2 warm-up
    steps and 3 replays against 5 eager steps; the rest of the step has atomics, hence the 2e-3): the memory lives on the device and is
    updated in place, so the replays keep moving it.  One linear chain; no queue setting is touched."""
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver, GraphedStep
    from test_triplet_gpu import _tiny
    meta, state, batch_, build = _tiny()
    images = {m: t.cuda() for m, t in batch_['images'].items()}
    masks = dict(batch_['modality_mask'])
    labels = batch_['person_id'].cuda()

    def make():
        m = build(cluster_nce_weight=0.5, cluster_nce_source='modalities')
        m.set_cluster_memory(_memory(5, 512, 9))
        gs = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in m.get_learnable_params()]
        return m, StepDriver(m, FusedAdamW(gs, weight_decay=1e-4))

    a, da = make()
    start = a.cluster_memory.centroids.clone()
    tok = a.tokenizer(batch_['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
    tok = {k: v.cuda() for k, v in tok.items()}
    g = GraphedStep(da, images, tok, masks, labels, warmup=2)
    for _ in range(3):
        La = g.step(images, tok, masks, labels)
    torch.cuda.synchronize()
    b, db = make()
    for _ in range(5):
        Lb = db.step(images, tok, masks, labels)
    assert da.opt.step_count == db.opt.step_count == 5
    assert float(Lb['cluster_nce_loss'].detach()) > 0 and int(Lb['cluster_nce_valid_cnt']) == int(La['cluster_nce_valid_cnt']) > 0
    for k in ('total_loss', 'cluster_nce_loss'):
        va, vb = float(La[k].detach()), float(Lb[k].detach())
        assert abs(va - vb) <= 2e-3 * max(1.0, abs(vb)), k
    ca, cb = a.cluster_memory.centroids.double().cpu(), b.cluster_memory.centroids.double().cpu()
    assert float((cb - start.double().cpu()).abs().max()) > 1e-3
    assert bool(((ca - cb).abs() <= 2e-3 * cb.abs().clamp(min=1.0)).all())


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_clustering_to_memory_end_to_end():
    """Synthetic identities (N = 256, D = 32: 28 identities x 8 rows around Gaussian centroids, 32 scattered rows) -> jaccard_dbscan ->
    ClusterMemory.from_clustering -> the centroids are the reference's means of kept().  The neighbour search of the clustering takes
    D in multiples of 64: it gets the rows padded with 32 zero columns (the same cosines), the memory the 32 columns themselves."""
    from prcv2025reid_amd.cluster import ClusterParams, jaccard_dbscan
    from prcv2025reid_amd.losses import ClusterMemory, cluster_nce
    g = np.random.default_rng(12)
    cent = 4.0 * g.standard_normal((28, 32))
    X = np.concatenate([np.repeat(cent, 8, axis=0) + 0.5 * g.standard_normal((224, 32)), 4.0 * g.standard_normal((32, 32))])
    X = X[g.permutation(256)].astype(np.float32)
    Xd = dev(X)
    cl = jaccard_dbscan(torch.cat([Xd, torch.zeros_like(Xd)], dim=1), ClusterParams(k1=10, k2=3, eps=0.6, min_samples=4))
    index, kept_labels = cl.kept()
    assert cl.n_clusters >= 8 and 64 <= index.numel() <= 256
    mem = ClusterMemory.from_clustering(Xd, cl)
    assert (mem.num_clusters, mem.dim) == (cl.n_clusters, 32)
    want, err = R.centroids(X[index.cpu().numpy()], kept_labels.cpu().numpy())
    assert bool((np.linalg.norm(mem.centroids.double().cpu().numpy() - want, axis=1) <= err).all())
    # the pseudo-labels (noise -1 included) drive the loss: only the kept rows are used
    loss, n_used, _ = cluster_nce(Xd, cl.labels.cuda(), mem, update=False)
    f = R.forward(X[None], cl.labels.cpu().numpy(), None, mem.centroids.cpu().numpy(), 0.05)
    assert int(n_used) == index.numel() == f['n_used'] and abs(float(loss) - f['loss']) <= R.loss_bound(32, cl.n_clusters, 0.05)
