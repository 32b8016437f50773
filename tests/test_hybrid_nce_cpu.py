"""CPU: the hybrid memory loss's reference (hybrid_nce_ref.py) against SpCL's literal [R, M] form under torch fp64 autograd, the fp32
table formula and blend loop, that the GPU tests' cases stand far above their bounds, Clustering.hybrid_labels(), the config defaults and
what _read_loss_settings makes of them, the new entry points in the header and in _lib.SIGNATURES, the argument checks of the C entry
points (refused before any launch, so no device is needed), the state of HybridMemory, and the checkpoint keys with a stand-in model."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hybrid_nce_ref as H
from test_cabi_cpu import ctype_of, header_macro, header_prototypes
from test_ema_cpu import _Model, _tiny, OLD_KEYS

NEW = ['reid_class_means', 'reid_hybrid_update_instances', 'reid_hybrid_refresh_classes']
# the (S, N, C) grid and the D of every case of tests/test_hybrid_nce_gpu.py::test_loss_and_dx_against_the_reference
GRID = [(S, N, C) for S in (1, 3) for N in (1, 3, 65) for C in (1, 64, 65, 129)]
TAU, DLOSS = 0.05, -0.7


def grid_case(S, N, C):
    """(D, V, cls, T, x, index, valid, f) of one case of the grid: M = 2 C + 7 instances (C = 1: one class of 9)."""
    D = 96 if S == 3 else 64
    M = 2 * C + 7
    V, cls = H.memory_case(M, D, C, 100 * C + N)
    T = H.class_means(V, cls, C)
    x, index, valid = H.batch_case(S, N, D, V, cls, 10 * C + N + S)
    return D, V, cls, T, x, index, valid, H.forward(x, index, valid, T, cls, TAU)


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('shape', [(1, 9, 32, 5, 12), (3, 7, 96, 70, 150), (2, 16, 512, 130, 300)])
def test_reference_is_spcl_literal_form_under_autograd(shape):
    """SpCL's own code: sim = x^ @ V.T over ALL M instances, aggregated by class with index_add_, divided by the class counts, a
    masked softmax over the classes, the NLL of the instance's class."""
    S, N, D, C, M = shape
    V, cls = H.memory_case(M, D, C, 7 + N)
    x, index, valid = H.batch_case(S, N, D, V, cls, 3 + N)
    T64 = H.class_means64(V, cls, C)
    f = H.forward(x, index, valid, T64, cls, TAU, dloss=-1.5)
    assert 0 < f['n_used'] < S * N
    xa = torch.from_numpy(x).double().requires_grad_(True)
    Vt, ct = torch.from_numpy(V).double(), torch.from_numpy(cls)
    sim = (F.normalize(xa.reshape(S * N, D), dim=1, eps=1e-12) @ Vt.T / TAU).T                      # [M, R]
    agg = torch.zeros(C, S * N, dtype=torch.float64).index_add_(0, ct, sim)
    nums = torch.zeros(C, 1, dtype=torch.float64).index_add_(0, ct, torch.ones(M, 1, dtype=torch.float64))
    mask = (nums > 0).double()
    agg = (agg / (mask * nums + (1 - mask))).T                                                       # [R, C]
    e = torch.exp(agg - agg.max(dim=1, keepdim=True).values.detach()) * mask.T
    p = e / (e.sum(dim=1, keepdim=True) + 1e-300)
    used, y = torch.from_numpy(f['used']), torch.from_numpy(f['y'])
    rows = -torch.log(p[used, y[used]])
    L = rows.mean()
    (L * -1.5).backward()
    assert abs(f['loss'] - float(L.detach())) <= 1e-12 * (1 + abs(float(L.detach())))
    assert np.abs(f['row_loss'][f['used']] - rows.detach().numpy()).max() <= 1e-11 / TAU
    g = xa.grad.reshape(S * N, D).numpy()
    assert np.abs(g).max() > 0 and np.abs(f['dx'] - g).max() <= 1e-11 * np.abs(g).max() / TAU
    assert not f['dx'][~f['used']].any() and not f['row_loss'][~f['used']].any()
    # the fp32 table is the fp64 one to a few roundings per member
    n = np.bincount(cls, minlength=C)[:, None]
    assert np.abs(H.class_means(V, cls, C).astype(np.float64) - T64).max() <= (n.max() + 1) * H.U


def test_table_formula_in_fp32():
    V = np.array([[1.0, -0.0, 2.0 ** -24, 0.75], [1.0, 0.0, 1.0, 0.25], [2.0 ** -24, -0.0, 2.0 ** -24, 0.5], [3.0, 5.0, -7.0, -0.0]], dtype=np.float32)
    cls = np.array([0, 0, 0, 1])
    T = H.class_means(V, cls)
    # ascending, one by one, every addition rounded: (1 + 1) + 2^-24 = 2 in fp32; 2^-24 + 1 = 1 (ties to even), 1 + 2^-24 = 1
    assert T[0].tolist() == [np.float32(2.0) / np.float32(3.0), 0.0, np.float32(1.0) / np.float32(3.0), 0.5]
    assert np.array_equal(T[1].view(np.int32), V[3].view(np.int32))                  # a singleton is its entry bit for bit, the -0 included
    assert not np.signbit(T[0][1]) and np.signbit(T[1][3])                           # (-0 + 0) + -0 = +0 where three members meet
    order, offsets, counts = H.csr(np.array([2, 0, 2, 1, 0, 2]))
    assert order.tolist() == [1, 4, 3, 0, 2, 5] and offsets.tolist() == [0, 2, 3, 6] and counts.tolist() == [2, 1, 3]
    with pytest.raises(AssertionError, match='class 1 has no member'):
        H.class_means(V, np.array([0, 0, 2, 2]))


def test_blend_loop_in_fp32_and_its_order():
    g = np.random.default_rng(4)
    rows = g.standard_normal((3, 32))
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    v = rows[0]
    a, b = H.blend_f32(v, rows[1:], 0.2), H.blend_f32(v, rows[1:][::-1], 0.2)
    assert abs(np.linalg.norm(a.astype(np.float64)) - 1) <= H.R.e_n(32) + H.U and np.abs(a - b).max() > 1e-2          # the blend does not commute
    assert np.array_equal(H.blend_f32(v, [-v], 0.5), np.zeros(32, dtype=np.float32))                        # the 1e-12 clamp: 0 / 1e-12
    assert np.abs(H.blend_f32(v, rows[1:2], 0.0) - rows[1]).max() <= H.R.e_n(32) + H.U                      # m = 0: the row itself, renormalised
    assert np.abs(H.blend_f32(v, rows[1:], 1.0) - v).max() <= 2 * (H.R.e_n(32) + H.U)                       # m = 1: the entry stays, renormalised twice
    # the fp64 recurrence of update_instances is the same loop within its bound
    V = rows.copy()
    f = dict(used=np.ones(2, dtype=bool), row_loss=np.ones(2), index=np.array([0, 0]), xhat=rows[1:].astype(np.float64),
             target_cos=np.zeros(2))
    want, err = H.update_instances(V, f, 0.2)
    assert np.linalg.norm(a - want[0]) <= err[0] and err[1] == err[2] == 0 and np.array_equal(want[1:], V[1:].astype(np.float64))


@pytest.mark.parametrize('S,N,C', GRID)
def test_gpu_cases_stand_far_above_their_bounds(S, N, C):
    """What tests/test_hybrid_nce_gpu.py compares stands at least 50 bounds above the bound it is compared within, for every used row
    -- except with ONE class, where lse = l_y and the loss and the gradient are 0 by definition (the GPU test asserts exact zeros)."""
    D, V, cls, T, x, index, valid, f = grid_case(S, N, C)
    counts = np.bincount(cls, minlength=C)
    assert f['n_used'] > 0 and counts.min() >= 1 and H.table_norm(T) <= 1 + 4 * H.U
    hit = counts[f['y'][f['used']]]
    if C > 1:
        assert (hit == 1).any() and (N < 3 or (hit > 1).any())                      # outlier singletons and multi-member classes both hit
        s_row, s_dx = H.signal(f, D, C, TAU, DLOSS, H.table_norm(T))
        assert s_row >= 50 and s_dx >= 50, (s_row, s_dx)
        assert np.abs(f['dx']).max() > 0
    else:
        assert np.abs(f['row_loss']).max() <= 1e-12 and np.abs(f['dx']).max() <= 1e-9
    if N >= 5:
        assert not f['used'].all() and (f['index'] == -1).any()


# ---------------------------------------------------------------------------------------------------------------- hybrid_labels
def _clustering(labels, n_clusters):
    from prcv2025reid_amd.cluster import Clustering
    z = torch.zeros(0)
    return Clustering(labels=torch.tensor(labels, dtype=torch.int64), core=z, n_clusters=n_clusters, rounds=0, rowptr=z, cols=z)


def test_hybrid_labels():
    lab, C = _clustering([1, 0, 1, 2, 0], 3).hybrid_labels()                        # no noise
    assert lab.tolist() == [1, 0, 1, 2, 0] and C == 3 and lab.dtype == torch.int64
    lab, C = _clustering([-1, -1, -1], 0).hybrid_labels()                           # all noise: every row a class of its own
    assert lab.tolist() == [0, 1, 2] and C == 3
    cl = _clustering([-1, 1, 0, -1, 1, -1, 0], 2)                                   # interleaved: the rank among the noise rows, ascending
    lab, C = cl.hybrid_labels()
    assert lab.tolist() == [2, 1, 0, 3, 1, 4, 0] and C == 5
    assert cl.labels.tolist() == [-1, 1, 0, -1, 1, -1, 0]                           # the clustering itself is unchanged
    assert torch.bincount(lab, minlength=C).min() >= 1


# ---------------------------------------------------------------------------------------------------------------- configuration
def settings_of(config):
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel
    model = types.SimpleNamespace()
    CLIPBasedMultiModalReIDModel._read_loss_settings(model, config)
    return model


def test_config_defaults_and_loss_settings():
    from prcv2025reid_amd.config import TrainingConfig
    names = ('hybrid_nce_weight', 'hybrid_nce_temperature', 'hybrid_nce_momentum', 'hybrid_nce_source')
    c = TrainingConfig()
    assert tuple(getattr(c, n) for n in names) == (0.0, 0.05, 0.2, 'bn')
    for cfg in (c, types.SimpleNamespace()):                    # a config without the fields gets the defaults
        assert tuple(getattr(settings_of(cfg), n) for n in names) == (0.0, 0.05, 0.2, 'bn')
    m = settings_of(TrainingConfig(hybrid_nce_weight=0.5, hybrid_nce_temperature=0.07, hybrid_nce_momentum=0.1, hybrid_nce_source='modalities'))
    assert tuple(getattr(m, n) for n in names) == (0.5, 0.07, 0.1, 'modalities')
    for bad, text in ((dict(hybrid_nce_source='fused'), "hybrid_nce_source must be 'bn' or 'modalities'"),
                      (dict(hybrid_nce_temperature=0.0), 'temperature must be > 0'), (dict(hybrid_nce_temperature=float('inf')), 'temperature'),
                      (dict(hybrid_nce_momentum=-0.1), r'momentum must be in \[0, 1\]'), (dict(hybrid_nce_momentum=1.5), 'momentum')):
        with pytest.raises(ValueError, match=text):
            settings_of(TrainingConfig(**bad))


def test_the_pinned_names_did_not_move():
    from prcv2025reid_amd.model import AUX_TERMS, LOSS_FIELDS
    assert [n for n, _ in AUX_TERMS] == ['triplet', 'cross_triplet', 'hc_triplet', 'xbm', 'center']
    assert not any(n.startswith('hybrid_nce') for n in LOSS_FIELDS) and len(LOSS_FIELDS) == 18


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_and_bound():
    from prcv2025reid_amd import _lib
    protos = header_prototypes()
    names = list(_lib.SIGNATURES)
    at = names.index('reid_smooth_ap_bwd') + 1                   # behind the ClusterNCE block and the Smooth-AP block that follows it
    assert names[at:at + len(NEW)] == NEW and list(protos)[at:at + len(NEW)] == NEW
    for name in NEW:
        ret, params = protos[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert (restype, list(argtypes)) == (ctype_of(ret), [ctype_of(p) for p in params]), name
    assert header_macro('REID_ABI_VERSION') == _lib.ABI_VERSION == 201


def good_arguments():
    base = 0x10000                                            # never dereferenced: every call is refused before a launch
    names = ('V', 'order', 'offsets', 'T', 'index', 'labels', 'row_loss', 'ws')
    return dict(S=2, N=5, D=32, C=4, M=10, ldv=32, momentum=0.2, stream=None, valid=None, **{n: base * (i + 1) for i, n in enumerate(names)})


ORDER = {'means': ('V', 'ldv', 'M', 'order', 'offsets', 'C', 'D', 'T', 'stream'),
         'instances': ('index', 'valid', 'S', 'N', 'D', 'row_loss', 'ws', 'V', 'ldv', 'M', 'momentum', 'stream'),
         'refresh': ('labels', 'valid', 'S', 'N', 'D', 'row_loss', 'V', 'ldv', 'M', 'order', 'offsets', 'T', 'C', 'stream')}
ENTRY = {'means': 'reid_class_means', 'instances': 'reid_hybrid_update_instances', 'refresh': 'reid_hybrid_refresh_classes'}


def violations():
    """(entry, overrides, a piece of the error text) of every requirement of include/reid_hip.h."""
    out = []
    for e in ('instances', 'refresh'):
        out += [(e, dict(S=0), 'S=0'), (e, dict(S=10), 'S=10'), (e, dict(N=0), 'N=0'), (e, dict(N=8193), 'N=8193')]
    for e in ENTRY:
        out += [(e, dict(D=16), 'D=16'), (e, dict(D=48), 'D=48'), (e, dict(D=1056, ldv=1056), 'D=1056'), (e, dict(M=0), 'M=0'), (e, dict(ldv=28), 'ldv=28'),
                (e, dict(ldv=34), 'ldv=34'), (e, dict(V=0x10004), '16-byte aligned')]
    for e in ('means', 'refresh'):
        out += [(e, dict(C=0), 'K=0'), (e, dict(C=2 ** 26, D=32), 'K * D beyond 2^31'), (e, dict(T=0x40008), '16-byte aligned')]
    out += [('means', {n: None}, 'null pointer') for n in ('V', 'order', 'offsets', 'T')]
    out += [('instances', {n: None}, 'null pointer') for n in ('index', 'row_loss', 'ws', 'V')]
    out += [('refresh', {n: None}, 'null pointer') for n in ('labels', 'row_loss', 'V', 'order', 'offsets', 'T')]
    out += [('instances', dict(ws=0x8000c), '16-byte aligned'), ('instances', dict(momentum=-0.5), 'momentum='), ('instances', dict(momentum=1.5), 'momentum='),
            ('instances', dict(momentum=float('nan')), 'momentum=')]
    return out


def call(h, entry, args):
    return getattr(h, ENTRY[entry])(*[args[n] for n in ORDER[entry]])


def test_library_refuses_bad_arguments_before_any_launch():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    good = good_arguments()
    for path in _lib.LIB_PATHS.values():
        h = _lib.bind(ctypes.CDLL(path))
        seen = set()
        for entry, over, text in violations():
            rc = call(h, entry, {**good, **over})
            assert rc == -1, (entry, over, rc)
            assert text.encode() in h.reid_last_error() and ENTRY[entry].encode() in h.reid_last_error(), (entry, over, h.reid_last_error())
            seen.add(entry)
        assert seen == set(ENTRY)


def test_cpu_tensors_and_bad_arguments_are_refused():
    from prcv2025reid_amd import losses, ops, _lib
    V, cls = H.memory_case(12, 32, 5, 1)
    x, index, valid = (torch.from_numpy(a) for a in H.batch_case(2, 5, 32, V, cls, 1))
    mem = losses.HybridMemory(12, 32, 'cpu')
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.hybrid_nce(x, index, mem)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.hybrid_nce(x[0], index, None, valid=valid[0])
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.HybridMemory.from_labels(torch.from_numpy(V), torch.from_numpy(cls))
    with pytest.raises(_lib.ReidHipError):
        ops.class_means(mem.instances, mem.order, mem.offsets, mem.table)
    for bad, text in ((dict(temperature=0.0), 'temperature'), (dict(momentum=2.0), 'momentum')):
        with pytest.raises(ValueError, match=text):
            losses.hybrid_nce_args('hybrid_nce', **{**dict(temperature=0.05, momentum=0.2), **bad})


def test_hybrid_memory_state_and_labels_on_the_cpu():
    from prcv2025reid_amd.losses import HybridMemory
    a = HybridMemory(6, 32, 'cpu')
    assert a.instances.shape == (6, 32) and a.instances.dtype == torch.float32 and (a.num_classes, a.table.shape) == (1, (1, 32))
    assert a.labels.tolist() == [0] * 6 and a.counts.tolist() == [6] and a.order.tolist() == list(range(6)) and a.offsets.tolist() == [0, 6]
    a.instances.copy_(F.normalize(torch.randn(6, 32, generator=torch.Generator().manual_seed(1)), dim=1))
    held = a.instances
    a.set_labels(torch.tensor([2, 0, 2, 1, 0, 2]))
    assert a.instances is held and a.num_classes == 3 and a.table.shape == (3, 32)
    assert a.order.tolist() == [1, 4, 3, 0, 2, 5] and a.offsets.tolist() == [0, 2, 3, 6] and a.counts.tolist() == [2, 1, 3]
    assert a.classes_of(torch.tensor([0, 5, -1, 6, 3])).tolist() == [2, 2, -1, -1, 1]
    st = a.state()
    assert set(st) == {'instances', 'labels'} and st['instances'].data_ptr() != a.instances.data_ptr() and st['labels'].tolist() == [2, 0, 2, 1, 0, 2]
    b = HybridMemory(6, 32, 'cpu')
    held_b = b.instances
    b.load_state(st)
    assert b.instances is held_b and torch.equal(b.instances, a.instances) and torch.equal(b.labels, a.labels) and b.num_classes == 3
    with pytest.raises(ValueError, match='instances'):
        HybridMemory(5, 32, 'cpu').load_state(st)
    with pytest.raises(ValueError, match=r'hybrid_labels\(\)'):
        a.set_labels(torch.tensor([0, 1, -1, 1, 0, 0]))
    with pytest.raises(ValueError, match='class 1 has no instance'):
        a.set_labels(torch.tensor([0, 2, 2, 0, 0, 0]))
    with pytest.raises(ValueError, match='one per instance'):
        a.set_labels(torch.tensor([0, 1]))
    assert a.num_classes == 3                                  # a refused re-labelling changes nothing
    for bad in ((0, 32), (4, 16), (4, 48), (4, 1056)):
        with pytest.raises(ValueError):
            HybridMemory(*bad, 'cpu')


# ---------------------------------------------------------------------------------------------------------------- checkpoint
class _Memory:
    """What checkpoint.py asks of model.hybrid_memory."""
    def __init__(self, v, labels):
        self.instances, self.labels = v, labels

    def state(self):
        return {'instances': self.instances.clone(), 'labels': self.labels.clone()}


def test_checkpoint_round_trips_the_hybrid_memory(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    from prcv2025reid_amd.losses import HybridMemory
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    V = F.normalize(torch.randn(7, 32, generator=torch.Generator().manual_seed(2)), dim=1)
    labels = torch.tensor([0, 1, 0, 2, 3, 1, 0])
    m.hybrid_memory = _Memory(V.clone(), labels.clone()); m.hybrid_nce_source = 'modalities'
    path = str(tmp_path / 'c' / 'memory.pth')
    ck.save_checkpoint(m, None, None, 2, 0.5, cfg, path)
    back = torch.load(path, map_location='cpu', weights_only=False)
    assert set(back) == OLD_KEYS | {'hybrid_memory_state_dict'}
    assert set(back['hybrid_memory_state_dict']) == {'instances', 'labels', 'hybrid_nce_source'}
    assert back['hybrid_memory_state_dict']['hybrid_nce_source'] == 'modalities' and torch.equal(back['hybrid_memory_state_dict']['instances'], V)
    # into a model without a memory: made on load; into one that has one: filled in place; another shape: refused
    m2 = _Model(arch, {k: v + 1.0 for k, v in sd.items()}, 5)
    m2.hybrid_memory = None
    info = ck.load_checkpoint(path, m2)
    assert info['epoch'] == 2 and 'hybrid_memory_state_dict' not in info
    assert isinstance(m2.hybrid_memory, HybridMemory) and torch.equal(m2.hybrid_memory.instances, V) and torch.equal(m2.hybrid_memory.labels, labels)
    assert m2.hybrid_memory.num_classes == 4
    m3 = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    m3.hybrid_memory = HybridMemory(7, 32, 'cpu'); held = m3.hybrid_memory.instances
    ck.load_checkpoint(path, m3)
    assert m3.hybrid_memory.instances is held and torch.equal(held, V)
    m3.hybrid_memory = HybridMemory(7, 64, 'cpu')
    with pytest.raises(ValueError, match='instances'):
        ck.load_checkpoint(path, m3)


def test_checkpoint_without_a_memory_keeps_the_old_keys(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    path = str(tmp_path / 'c' / 'plain.pth')
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, path)
    m.hybrid_memory = None
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, str(tmp_path / 'c' / 'none.pth'))
    for f in ('plain.pth', 'none.pth'):
        assert set(torch.load(str(tmp_path / 'c' / f), map_location='cpu', weights_only=False)) == OLD_KEYS
    m.hybrid_memory = 'untouched'
    ck.load_checkpoint(path, m)                               # a checkpoint without the key leaves the model's memory alone
    assert m.hybrid_memory == 'untouched'
