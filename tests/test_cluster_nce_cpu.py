"""CPU: the cluster-contrast loss's fp64 reference (cluster_nce_ref.py) against torch autograd and against the literal sequential
update loop, the 'hard' pick and its tie rule, the config defaults and what _read_loss_settings makes of them, the new entry points in
the header and in _lib.SIGNATURES, the argument checks of the C entry points (refused before any launch, so no device is needed), the
state of ClusterMemory, and the checkpoint keys with a stand-in model (the real one needs the HIP device)."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cluster_nce_ref as R
from test_cabi_cpu import ctype_of, header_macro, header_prototypes
from test_ema_cpu import _Model, _tiny, OLD_KEYS

NEW = ['reid_cluster_nce_ws_floats', 'reid_cluster_nce_plan', 'reid_cluster_nce_fwd', 'reid_cluster_nce_update', 'reid_cluster_nce_bwd',
       'reid_cluster_centroids']


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('shape,tau,spread', [((1, 9, 32, 5), 0.05, 0.5), ((3, 7, 96, 70), 0.2, 0.5), ((2, 16, 512, 130), 0.01, 6.0)])
def test_reference_loss_and_dx_against_autograd(shape, tau, spread):
    S, N, D, K = shape
    x, labels, valid, table = R.make_case(S, N, D, K, 11 + N, spread=spread)     # (tau = 0.01: rows far from their centroid, or p_y = 1 to the last bit)
    f = R.forward(x, labels, valid, table, tau, dloss=-1.5)
    assert 0 < f['n_used'] < S * N
    xa = torch.from_numpy(x).double().requires_grad_(True)
    C = torch.from_numpy(table).double()
    used = torch.from_numpy(f['used'])
    y = torch.from_numpy(f['y'])
    logits = F.normalize(xa.reshape(S * N, D), dim=1, eps=1e-12) @ C.T / tau
    rows = F.cross_entropy(logits[used], y[used], reduction='none')
    L = rows.mean()
    (L * -1.5).backward()
    assert abs(f['loss'] - float(L.detach())) <= 1e-12 * (1 + abs(float(L.detach())))
    assert np.abs(f['row_loss'][f['used']] - rows.detach().numpy()).max() <= 1e-11 / tau
    g = xa.grad.reshape(S * N, D).numpy()
    assert np.abs(g).max() > 0 and np.abs(f['dx'] - g).max() <= 1e-11 * np.abs(g).max() / tau
    assert not f['dx'][~f['used']].any() and not f['row_loss'][~f['used']].any() and not f['target_cos'][~f['used']].any()


def test_reference_edge_cases():
    x, labels, valid, table = R.make_case(1, 6, 32, 1, 3, noise=False)
    f = R.forward(x, labels, None, table, 0.05)                  # K = 1: the softmax has one class
    assert f['n_used'] == 6 and abs(f['loss']) <= 1e-12 and np.abs(f['dx']).max() <= 1e-9
    x, labels, valid, table = R.make_case(1, 6, 32, 4, 4, noise=False)
    x[0, 2] = 0.0                                                # the 1e-12 clamp: x^ = 0, every logit 0
    f = R.forward(x, labels, None, table, 0.05)
    assert abs(f['row_loss'][2] - np.log(4)) <= 1e-12 and f['inv'][2] == 1e12 and np.isfinite(f['dx']).all()
    f0 = R.forward(x, np.full(6, -1), None, table, 0.05)         # no used row
    assert (f0['loss'], f0['n_used']) == (0.0, 0) and not f0['dx'].any()
    new, err = R.update(table, f0, 0.1, 'mean')
    assert np.array_equal(new, table.astype(np.float64)) and not err.any()
    x[0, 0, 0] = 1.0; x[0, 0, 1:] = 0.0                          # tau = 0.01 with x^ = C_y: a logit of 100 next to -100
    t2 = np.zeros((2, 32), dtype=np.float32); t2[0, 0] = 1.0; t2[1, 0] = -1.0
    f = R.forward(x[:, :1], np.array([0]), None, t2, 0.01)
    assert np.isfinite(f['loss']) and 0 <= f['loss'] < 1e-80 and f['lse'][0] == 100.0


@pytest.mark.parametrize('momentum', [0.1, 0.5])
def test_reference_update_against_the_literal_loop(momentum):
    S, N, D, K = 3, 12, 32, 5
    x, labels, valid, table = R.make_case(S, N, D, K, 5)
    x[1, 5, 3] = np.nan                                          # row 17: used, not contributing
    f = R.forward(x, labels, valid, table, 0.05)
    con = R.contributing(f)
    assert f['used'][17] and not con[17] and con.sum() == f['n_used'] - 1
    new, err = R.update(table, f, momentum, 'mean')
    lit = R.literal_update(table, f, momentum)
    assert np.isfinite(new).all() and np.abs(new - lit).max() <= 1e-15
    present = set(f['y'][con].tolist())
    assert 0 < len(present) <= K
    for k in range(K):
        assert (err[k] > 0) == (k in present)
        if k not in present:
            assert np.array_equal(new[k], table[k].astype(np.float64))
        else:
            assert abs(np.linalg.norm(new[k]) - 1) <= 1e-15 and np.abs(new[k] - table[k]).max() > 0
    # the bound grows with the rows applied to a centroid, and linearly while m / nu <= 1
    n_rows = {k: int((con & (f['y'] == k)).sum()) for k in present}
    one = (R.e_n(D) + 4 * R.U) / 0.5 + R.e_n(D) + R.U
    assert all(err[k] <= 2.5 * n_rows[k] * one for k in present)


def test_hard_mode_picks_the_smallest_cosine_and_ties_go_to_the_lowest_row():
    D, K = 32, 3
    table = np.zeros((K, D), dtype=np.float32)
    table[0, 0] = table[1, 1] = table[2, 2] = 1.0
    x = np.zeros((2, 4, D), dtype=np.float32)
    labels = np.array([0, 0, 1, 2])
    # label 0: rows 0, 1, 4, 5 with cosines 0.8, 0.6, 0.6, 1.0 -> row 1 (the lower of the two 0.6); label 1: rows 2, 6, one invalid
    for r, c in ((0, 0.8), (1, 0.6), (4, 0.6), (5, 1.0)):
        x.reshape(8, D)[r, 0] = c; x.reshape(8, D)[r, 5] = np.sqrt(1 - c * c)
    x.reshape(8, D)[4, 5] = 0.0; x.reshape(8, D)[4, 6] = 0.8     # row 4: the same cosine from another direction
    x.reshape(8, D)[2, 1] = 1.0; x.reshape(8, D)[6, 1] = -1.0; x.reshape(8, D)[3, 2] = 1.0; x.reshape(8, D)[7, 2] = 1.0
    valid = np.ones((2, 4), dtype=np.uint8); valid[1, 2] = 0       # row 6 (cosine -1) is invalid: row 2 is label 1's only row
    f = R.forward(x, labels, valid, table, 0.05)
    assert np.allclose(f['target_cos'][[0, 1, 4, 5]], [0.8, 0.6, 0.6, 1.0], atol=1e-7) and f['target_cos'][1] == f['target_cos'][4]
    new, _ = R.update(table, f, 0.5, 'hard')
    want0 = 0.5 * table[0] + 0.5 * f['xhat'][1]
    assert np.abs(new[0] - want0 / np.linalg.norm(want0)).max() <= 1e-15 and new[0][5] > 0 and new[0][6] == 0
    assert np.abs(new[1] - table[1]).max() <= 1e-15              # blended with itself
    mean, _ = R.update(table, f, 0.5, 'mean')
    assert np.abs(mean[0] - new[0]).max() > 1e-3
    assert R.hard_pick_gap(f) == 0.0                             # the tie: such a case must not be compared against fp32 picks


def test_reference_centroids():
    g = np.random.default_rng(2)
    feats = g.standard_normal((20, 32)).astype(np.float32)
    labels = np.array([0, 1, 2, -1, 0, 1, 2, -1, 0, 0, 1, 2, 2, 2, -1, 0, 1, 1, 0, 2])
    C, err = R.centroids(feats, labels)
    assert C.shape == (3, 32) and np.abs(np.linalg.norm(C, axis=1) - 1).max() <= 1e-15 and (err > 0).all() and err.max() < 1e-4
    want = F.normalize(torch.stack([torch.from_numpy(feats).double()[torch.from_numpy(labels) == k].mean(0) for k in range(3)]), dim=1)
    assert np.abs(C - want.numpy()).max() <= 1e-15
    with pytest.raises(ValueError, match='cluster 1 has no row'):
        R.centroids(feats, np.where(labels == 1, -1, labels))


def test_bounds_are_formulas_of_the_shape():
    # the logit bound: the dot product of two unit rows plus the two normalisations, over tau
    assert R.e_logit(512, 0.05) == ((512 + 2 * (512 / 2 + 4)) * R.U + 3 * R.U) / 0.05
    assert R.row_bound(512, 1000, 0.05) < 3e-3 and R.row_bound(32, 2, 0.05) < 5e-4      # (of logits up to 20: small enough to mean something)
    assert 10 * R.row_bound(64, 100, 0.0625, exact=True) < R.row_bound(64, 100, 0.0625)      # the exact case's bound is much tighter
    assert R.loss_bound(96, 65, 0.05) > R.row_bound(96, 65, 0.05) > R.e_lse(96, 65, 0.05) > R.e_logit(96, 0.05)


# ---------------------------------------------------------------------------------------------------------------- configuration
def settings_of(config):
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel
    model = types.SimpleNamespace()
    CLIPBasedMultiModalReIDModel._read_loss_settings(model, config)
    return model


def test_config_defaults_and_loss_settings():
    from prcv2025reid_amd.config import TrainingConfig
    c = TrainingConfig()
    assert (c.cluster_nce_weight, c.cluster_nce_temperature, c.cluster_nce_momentum, c.cluster_nce_mode, c.cluster_nce_source) == \
        (0.0, 0.05, 0.1, 'mean', 'bn')
    for cfg in (c, types.SimpleNamespace()):                    # a config without the fields gets the defaults
        m = settings_of(cfg)
        assert (m.cluster_nce_weight, m.cluster_nce_temperature, m.cluster_nce_momentum, m.cluster_nce_mode, m.cluster_nce_source) == \
            (0.0, 0.05, 0.1, 'mean', 'bn')
    m = settings_of(TrainingConfig(cluster_nce_weight=0.5, cluster_nce_temperature=0.07, cluster_nce_momentum=0.2, cluster_nce_mode='hard',
                                   cluster_nce_source='modalities'))
    assert (m.cluster_nce_weight, m.cluster_nce_temperature, m.cluster_nce_momentum, m.cluster_nce_mode, m.cluster_nce_source) == \
        (0.5, 0.07, 0.2, 'hard', 'modalities')
    for bad, text in ((dict(cluster_nce_mode='soft'), "mode must be 'mean' or 'hard'"), (dict(cluster_nce_source='fused'), "cluster_nce_source must be 'bn' or 'modalities'"),
                      (dict(cluster_nce_temperature=0.0), 'temperature must be > 0'), (dict(cluster_nce_temperature=float('inf')), 'temperature'),
                      (dict(cluster_nce_momentum=-0.1), r'momentum must be in \[0, 1\]'), (dict(cluster_nce_momentum=1.5), 'momentum')):
        with pytest.raises(ValueError, match=text):
            settings_of(TrainingConfig(**bad))


def test_the_pinned_names_did_not_move():
    from prcv2025reid_amd.model import AUX_TERMS, LOSS_FIELDS
    assert [n for n, _ in AUX_TERMS] == ['triplet', 'cross_triplet', 'hc_triplet', 'xbm', 'center']
    assert not any(n.startswith('cluster_nce') for n in LOSS_FIELDS)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_and_bound():
    from prcv2025reid_amd import _lib
    protos = header_prototypes()
    names = list(_lib.SIGNATURES)
    at = names.index('reid_center_bwd') + 1
    assert names[at:at + len(NEW)] == NEW and list(protos)[at:at + len(NEW)] == NEW
    for name in NEW:
        ret, params = protos[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert (restype, list(argtypes)) == (ctype_of(ret), [ctype_of(p) for p in params]), name
    assert header_macro('REID_ABI_VERSION') == _lib.ABI_VERSION == 201
    assert (header_macro('REID_CLUSTER_NCE_MEAN'), header_macro('REID_CLUSTER_NCE_HARD')) == (_lib.CLUSTER_NCE_MODES['mean'], _lib.CLUSTER_NCE_MODES['hard'])


def good_arguments():
    base = 0x10000                                            # never dereferenced: every call is refused before a launch
    names = ('x', 'labels', 'table', 'ws', 'row_loss', 'target_cos', 'result', 'dloss', 'dx', 'feats', 'order', 'offsets')
    return dict(S=2, N=5, D=32, K=4, ldx=32, lddx=32, ldf=32, rows=10, tau=0.05, with_grad=1, momentum=0.1, mode=0, stream=None, valid=None,
                **{n: base * (i + 1) for i, n in enumerate(names)})


ORDER = {'fwd': ('x', 'ldx', 'labels', 'valid', 'S', 'N', 'D', 'table', 'K', 'tau', 'with_grad', 'ws', 'row_loss', 'target_cos', 'result', 'stream'),
         'update': ('labels', 'valid', 'S', 'N', 'D', 'row_loss', 'target_cos', 'ws', 'table', 'K', 'momentum', 'mode', 'stream'),
         'bwd': ('S', 'N', 'D', 'ws', 'result', 'dloss', 'dx', 'lddx', 'stream'),
         'centroids': ('feats', 'ldf', 'rows', 'order', 'offsets', 'K', 'D', 'table', 'stream'),
         'ws': ('S', 'N', 'D', 'K')}
ENTRY = {'fwd': 'reid_cluster_nce_fwd', 'update': 'reid_cluster_nce_update', 'bwd': 'reid_cluster_nce_bwd', 'centroids': 'reid_cluster_centroids',
         'ws': 'reid_cluster_nce_ws_floats'}


def violations():
    """(entry, overrides, a piece of the error text) of every requirement of include/reid_hip.h."""
    out = []
    for e in ('fwd', 'update', 'bwd', 'ws'):
        out += [(e, dict(S=0), 'S=0'), (e, dict(S=10), 'S=10'), (e, dict(N=0), 'N=0'), (e, dict(N=8193), 'N=8193'), (e, dict(D=16), 'D=16'),
                (e, dict(D=48), 'D=48'), (e, dict(D=1056), 'D=1056')]
    for e in ('fwd', 'update', 'ws', 'centroids'):
        out += [(e, dict(K=0), 'K=0'), (e, dict(K=2 ** 26, D=32), 'K * D beyond 2^31')]
    out += [('fwd', {n: None}, 'null pointer') for n in ('x', 'labels', 'table', 'ws', 'row_loss', 'target_cos', 'result')]
    out += [('update', {n: None}, 'null pointer') for n in ('labels', 'row_loss', 'target_cos', 'ws', 'table')]
    out += [('bwd', {n: None}, 'null pointer') for n in ('ws', 'result', 'dloss', 'dx')]
    out += [('centroids', {n: None}, 'null pointer') for n in ('feats', 'order', 'offsets', 'table')]
    out += [('fwd', dict(ldx=28), 'ldx=28'), ('fwd', dict(ldx=34), 'ldx=34'), ('bwd', dict(lddx=30), 'lddx=30'), ('centroids', dict(ldf=16), 'ldf=16'),
            ('fwd', dict(N=8192, S=9, ldx=2 ** 16), 'beyond 2^31'), ('centroids', dict(rows=0), 'rows=0'), ('centroids', dict(D=8), 'D=8'),
            ('fwd', dict(x=0x10004), '16-byte aligned'), ('fwd', dict(table=0x20008), '16-byte aligned'), ('fwd', dict(ws=0x4000c), '16-byte aligned'),
            ('update', dict(table=0x20004), '16-byte aligned'), ('bwd', dict(dx=0x90004), '16-byte aligned'), ('centroids', dict(feats=0xa0004), '16-byte aligned'),
            ('fwd', dict(tau=0.0), 'tau='), ('fwd', dict(tau=-1.0), 'tau='), ('fwd', dict(tau=float('nan')), 'tau='), ('fwd', dict(tau=float('inf')), 'tau='),
            ('fwd', dict(with_grad=2), 'with_grad=2'), ('update', dict(momentum=-0.5), 'momentum='), ('update', dict(momentum=1.5), 'momentum='),
            ('update', dict(momentum=float('nan')), 'momentum='), ('update', dict(mode=2), 'mode=2')]
    return out


def call(h, entry, args):
    return getattr(h, ENTRY[entry])(*[args[n] for n in ORDER[entry]])


def test_library_refuses_bad_arguments_before_any_launch():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    good = good_arguments()
    for path in _lib.LIB_PATHS.values():
        h = _lib.bind(ctypes.CDLL(path))
        plan = (ctypes.c_int32 * 4)()
        assert h.reid_cluster_nce_plan(64, 1000, 512, ctypes.cast(plan, ctypes.c_void_p)) == 0 and tuple(plan) == (64, 64, 16, 1)
        assert h.reid_cluster_nce_plan(320, 32768, 512, ctypes.cast(plan, ctypes.c_void_p)) == 0 and tuple(plan) == (64, 64, 64, 8)
        assert h.reid_cluster_nce_plan(1, 65, 32, ctypes.cast(plan, ctypes.c_void_p)) == 0 and tuple(plan) == (64, 64, 2, 1)
        assert h.reid_cluster_nce_plan(73728, 65, 32, ctypes.cast(plan, ctypes.c_void_p)) == 0 and tuple(plan) == (64, 64, 1, 2)
        for bad, text in (((0, 4, 32, ctypes.cast(plan, ctypes.c_void_p)), b'R=0'), ((1, 0, 32, ctypes.cast(plan, ctypes.c_void_p)), b'K=0'),
                          ((1, 4, 40, ctypes.cast(plan, ctypes.c_void_p)), b'D=40'), ((1, 4, 32, None), b'null pointer')):
            assert h.reid_cluster_nce_plan(*bad) == -1 and text in h.reid_last_error() and b'reid_cluster_nce_plan' in h.reid_last_error()
        # H, x^ and four per-row arrays, the (max, sum) pairs and the sum_c p C partials of the plan's splits, each a multiple of 4 floats
        assert h.reid_cluster_nce_ws_floats(2, 5, 32, 4) == 2 * 10 * 32 + 4 * 12 + 2 * 1 * 10 + 1 * 10 * 32
        assert h.reid_cluster_nce_ws_floats(1, 8, 32, 129) == 2 * 8 * 32 + 4 * 8 + 2 * 3 * 8 + 3 * 8 * 32
        seen = set()
        for entry, over, text in violations():
            rc = call(h, entry, {**good, **over})
            assert rc == -1, (entry, over, rc)
            assert text.encode() in h.reid_last_error() and ENTRY[entry].encode() in h.reid_last_error(), (entry, over, h.reid_last_error())
            seen.add(entry)
        assert seen == set(ENTRY)


def test_cpu_tensors_and_bad_arguments_are_refused():
    from prcv2025reid_amd import losses, ops, _lib
    x, labels, valid, table = (torch.from_numpy(a) for a in R.make_case(2, 5, 32, 4, 1))
    mem = losses.ClusterMemory(4, 32, 'cpu')
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.cluster_nce(x, labels, mem)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.cluster_nce(x[0], labels, None, valid=valid[0])
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.ClusterMemory.from_labels(x[0], labels)
    with pytest.raises(_lib.ReidHipError):
        ops.cluster_nce_fwd(x[0], labels, None, table, 0.05, True, torch.zeros(4096), torch.zeros(5), torch.zeros(5), torch.zeros(2))
    for bad, text in ((dict(mode='soft'), 'mode'), (dict(temperature=0.0), 'temperature'), (dict(momentum=2.0), 'momentum')):
        with pytest.raises(ValueError, match=text):
            losses.cluster_nce_args('cluster_nce', **{**dict(temperature=0.05, momentum=0.1, mode='mean'), **bad})


def test_cluster_memory_state_round_trip():
    from prcv2025reid_amd.losses import ClusterMemory
    a = ClusterMemory(6, 32, 'cpu')
    assert a.centroids.shape == (6, 32) and a.centroids.dtype == torch.float32 and float(a.centroids.abs().max()) == 0.0
    a.centroids.copy_(torch.randn(6, 32, generator=torch.Generator().manual_seed(1)))
    st = a.state()
    assert set(st) == {'centroids'} and st['centroids'].device.type == 'cpu' and st['centroids'].data_ptr() != a.centroids.data_ptr()
    b = ClusterMemory(6, 32, 'cpu')
    held = b.centroids
    b.load_state(st)
    assert b.centroids is held and torch.equal(b.centroids, a.centroids)      # in place: a captured graph's pointer stays valid
    with pytest.raises(ValueError, match='centroids'):
        ClusterMemory(5, 32, 'cpu').load_state(st)
    with pytest.raises(ValueError, match='centroids'):
        ClusterMemory(6, 64, 'cpu').load_state(st)
    b.reset()
    assert b.centroids is held and float(b.centroids.abs().max()) == 0.0
    for bad in ((0, 32), (4, 16), (4, 48), (4, 1056), (2 ** 26, 32)):
        with pytest.raises(ValueError):
            ClusterMemory(*bad, 'cpu')


# ---------------------------------------------------------------------------------------------------------------- checkpoint
class _Memory:
    """What checkpoint.py asks of model.cluster_memory."""
    def __init__(self, t):
        self.centroids = t

    def state(self):
        return {'centroids': self.centroids.clone()}


def test_checkpoint_round_trips_the_cluster_memory(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    from prcv2025reid_amd.losses import ClusterMemory
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    table = F.normalize(torch.randn(7, 32, generator=torch.Generator().manual_seed(2)), dim=1)
    m.cluster_memory = _Memory(table.clone()); m.cluster_nce_source = 'modalities'
    path = str(tmp_path / 'c' / 'memory.pth')
    ck.save_checkpoint(m, None, None, 2, 0.5, cfg, path)
    back = torch.load(path, map_location='cpu', weights_only=False)
    assert set(back) == OLD_KEYS | {'cluster_memory_state_dict'}
    assert set(back['cluster_memory_state_dict']) == {'centroids', 'cluster_nce_source'}
    assert back['cluster_memory_state_dict']['cluster_nce_source'] == 'modalities' and torch.equal(back['cluster_memory_state_dict']['centroids'], table)
    # into a model without a memory: made on load; into one that has one: filled in place; another shape: refused
    m2 = _Model(arch, {k: v + 1.0 for k, v in sd.items()}, 5)
    m2.cluster_memory = None
    info = ck.load_checkpoint(path, m2)
    assert info['epoch'] == 2 and 'cluster_memory_state_dict' not in info
    assert isinstance(m2.cluster_memory, ClusterMemory) and torch.equal(m2.cluster_memory.centroids, table)
    m3 = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    m3.cluster_memory = ClusterMemory(7, 32, 'cpu'); held = m3.cluster_memory.centroids
    ck.load_checkpoint(path, m3)
    assert m3.cluster_memory.centroids is held and torch.equal(held, table)
    m3.cluster_memory = ClusterMemory(7, 64, 'cpu')
    with pytest.raises(ValueError, match='centroids'):
        ck.load_checkpoint(path, m3)


def test_checkpoint_without_a_memory_keeps_the_old_keys(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    path = str(tmp_path / 'c' / 'plain.pth')
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, path)
    m.cluster_memory = None
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, str(tmp_path / 'c' / 'none.pth'))
    for f in ('plain.pth', 'none.pth'):
        assert set(torch.load(str(tmp_path / 'c' / f), map_location='cpu', weights_only=False)) == OLD_KEYS
    m.cluster_memory = 'untouched'
    ck.load_checkpoint(path, m)                               # a checkpoint without the key leaves the model's memory alone
    assert m.cluster_memory == 'untouched'
