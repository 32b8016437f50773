"""CPU: the Smooth-AP loss's fp64 reference (smooth_ap_ref.py) against torch autograd on the sigmoid definition written naively, its
tau -> 0 limit against the evaluator's exact AP, the zero row sums of ds, the inactive anchors, duplicate gallery rows, the config
defaults and what _read_loss_settings makes of them, the new entry points in the header and in _lib.SIGNATURES, and the argument checks
of the C entry points (refused before any launch, so no device is needed)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import smooth_ap_ref as R
from metrics_at_k_ref import rows_ref
from test_cabi_cpu import ctype_of, header_macro, header_prototypes

NEW = ['reid_smooth_ap_ws_floats', 'reid_smooth_ap_fwd', 'reid_smooth_ap_bwd']


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('P,N,Mg,D,tau,invalid,normalize', [(1, 5, 7, 8, 0.1, 0.0, True), (2, 6, 5, 12, 0.05, 0.25, True), (1, 4, 6, 8, 0.5, 0.0, False)])
def test_reference_against_autograd_on_the_naive_definition(P, N, Mg, D, tau, invalid, normalize):
    q, g, ql, gl, qv, gv = R.make_case(P, N, Mg, D, 3, 5 + N, invalid=invalid)
    gs = np.array([1.0, -0.5, 2.0][:P])
    f = R.forward(q, g, ql, gl, qv, gv, tau, normalize, gscale=gs)
    assert f['flag'].sum() > 0 and (f['n_active'] > 0).any()
    qt, gt = torch.from_numpy(q).double().requires_grad_(True), torch.from_numpy(g).double().requires_grad_(True)
    L = R.naive_loss_torch(qt, gt, ql, gl, qv, gv, tau, normalize)
    (L * torch.from_numpy(gs)).sum().backward()
    assert np.abs(f['loss'] - L.detach().numpy()).max() <= 1e-13
    scale = max(np.abs(qt.grad.numpy()).max(), np.abs(gt.grad.numpy()).max())
    assert scale > 0
    assert np.abs(f['dq'] - qt.grad.numpy()).max() <= 1e-12 * scale / tau and np.abs(f['dg'] - gt.grad.numpy()).max() <= 1e-12 * scale / tau
    if qv is not None:
        assert not f['dq'][qv == 0].any() and not f['dg'][gv == 0].any()


def test_reference_ring_form_against_autograd():
    P, N, D, M, tau = 2, 4, 8, 7, 0.1
    ring = R.Ring(M, P + 1, D)
    for step in range(2):                                        # 8 rows into 7 slots: the second enqueue wraps
        q, g, ql, _, qv, gv = R.make_case(P, N, N, D, 3, 40 + step, invalid=0.2)
        ring.enqueue(q, g, ql, qv, gv)
    assert ring.cursor == 1 and ring.written == 8
    mem = (ring.rows, ring.labels, ring.valid)
    f = R.forward(q, g, ql, ql, qv, gv, tau, ring=mem)
    qt, gt = torch.from_numpy(q).double().requires_grad_(True), torch.from_numpy(g).double().requires_grad_(True)
    L = R.naive_loss_torch(qt, gt, ql, ql, qv, gv, tau, ring=mem)
    L.sum().backward()
    assert f['flag'].sum() > 0 and np.abs(f['loss'] - L.detach().numpy()).max() <= 1e-13
    scale = np.abs(qt.grad.numpy()).max()
    assert scale > 0 and np.abs(f['dq'] - qt.grad.numpy()).max() <= 1e-11 * scale and np.abs(f['dg'] - gt.grad.numpy()).max() <= 1e-11 * scale


def test_small_temperature_limit_is_the_exact_ap():
    """12 anchors x 40 gallery rows, D = 32: at tau = 1e-6 the reference's AP_a is the AP of the stable descending ranking (the
    evaluator's, metrics_at_k_ref.rows_ref with K >= G).  The scores are fp32 values whose smallest gap is asserted: a gap of 3e-5 is
    30 tau, and a sigmoid 30 from its step is within e^-30 ~ 1e-13 of it."""
    r = np.random.default_rng(0)
    a, c = R.unit_rows(r.standard_normal((12, 32)))[0], R.unit_rows(r.standard_normal((40, 32)))[0]
    s = (a @ c.T).astype(np.float32)
    gaps = np.diff(np.sort(s.astype(np.float64), axis=1), axis=1).min()
    assert gaps >= 1e-5, gaps
    a_lab, c_lab = r.integers(0, 5, 12), r.integers(0, 5, 40)
    valid = np.ones(40, bool); valid[[3, 17]] = False
    worst = 0.0
    for i in range(12):
        pos = valid & (c_lab == a_lab[i])
        assert 0 < pos.sum() < valid.sum()
        got = R.rank_anchor(s[i].astype(np.float64), np.zeros(40), pos, valid, 1e-6, 32, with_bounds=False)['ap']
        ref = rows_ref(s[i][valid], c_lab[valid], a_lab[i], [40])
        want = float(ref['sum_at'][0]) / int(ref['npos'])
        assert int(ref['hits'][0]) == int(ref['npos']) == pos.sum() and abs(want - R.exact_ap(s[i], pos, valid)) <= 1e-15
        worst = max(worst, abs(got - want))
    print(f'smallest score gap {gaps:.3e}, largest |AP(tau = 1e-6) - exact AP| {worst:.3e}')
    assert worst <= 1e-12


def test_every_row_of_ds_sums_to_zero():
    q, g, ql, gl, qv, gv = R.make_case(2, 9, 11, 16, 3, 21, invalid=0.2)
    f = R.forward(q, g, ql, gl, qv, gv, 0.05)
    for d0, d1 in f['dirs']:
        for d in (d0, d1):
            assert (d['ap'] >= 0).any() and np.abs(d['ds']).max() > 1e-3
            assert np.abs(d['ds'].sum(1)).max() <= 1e-13 * np.abs(d['ds']).max() * d['ds'].shape[1]


def test_inactive_anchors():
    D = 8
    r = np.random.default_rng(4)
    q, g = r.standard_normal((1, 5, D)), r.standard_normal((4, D))
    ql, gl = np.array([0, 1, 2, 0, 7]), np.array([0, 0, 1, 2])
    qv, gv = np.array([[1, 1, 1, 0, 1]], np.uint8), np.array([1, 1, 0, 1], np.uint8)
    f = R.forward(q, g, ql, gl, qv, gv, 0.1)
    # q 0: two positives, one negative (g 3): active.  q 1: its only positive (g 2) is invalid.  q 2: active.  q 3: invalid.  q 4: no positive.
    assert (f['q_ap'][0] >= 0).tolist() == [True, False, True, False, False] and f['q_npos'][0].tolist() == [2, 0, 1, 0, 0]
    # an inactive anchor has no score gradient of its own (a valid one still is a gallery row of the other direction); an invalid row has none
    assert not f['dirs'][0][0]['ds'][[1, 3, 4]].any() and f['dirs'][0][0]['ds'][[0, 2]].any(1).all()
    assert not f['dq'][0, 3].any() and f['dq'][0, 0].any() and not f['dirs'][0][1]['ds'][:, 3].any()
    assert f['n_active'][0].tolist() == [2.0, float((f['g_ap'][0] >= 0).sum())] and f['g_ap'][0][2] == -1.0 and not f['dg'][2].any()
    # no negative: every valid gallery row is a positive -> AP is identically 1, inactive in both directions: flag 0, loss 0
    f = R.forward(q, g, np.zeros(5, np.int64), np.zeros(4, np.int64), qv, gv, 0.1)
    assert f['flag'][0] == 0 and f['loss'][0] == 0 and not f['dq'].any() and not f['dg'].any() and (f['q_ap'] == -1).all()
    assert f['q_npos'][0].tolist() == [3, 3, 3, 0, 3]


def test_duplicate_gallery_rows_give_one_half():
    """Two identical positives and no other row near: sigma(0) = 1/2 between them, so R+ = R = 1.5 + (the rows above) for both."""
    D = 8
    a = np.zeros((1, 1, D)); a[0, 0, 0] = 1.0
    g = np.zeros((3, D)); g[0, 0] = g[1, 0] = 1.0; g[0, 1] = g[1, 1] = 0.5; g[2, 0] = -1.0
    f = R.forward(a, g, np.array([0]), np.array([0, 0, 1]), tau=0.01)
    d = f['dirs'][0][0]
    assert d['s'][0, 0] == d['s'][0, 1] and abs(f['q_ap'][0, 0] - 1.0) <= 1e-15           # both rank 1.5 of 1.5: AP = 1 exactly
    f = R.forward(a, g, np.array([0]), np.array([0, 1, 1]), tau=0.01)                     # now the twin is a negative
    assert abs(f['q_ap'][0, 0] - 1.0 / 1.5) <= 1e-15


def test_bounds_are_formulas_of_the_shape():
    assert R.e_unit(512) == ((8 * 2 + 6) / 2 + 3) * R.U and R.n_sum(257) == 5 + 7 and R.tau32(0.01) == float(np.float32(0.01))
    q, g, ql, gl, _, _ = R.make_case(1, 8, 65, 32, 4, 9)
    lo, hi = R.forward(q, g, ql, gl, tau=0.1), R.forward(q, g, ql, gl, tau=0.01)
    assert 0 < lo['e_loss'][0] < hi['e_loss'][0] < 1e-3                                   # a smaller tau amplifies the score error
    assert (hi['e_dq'] >= 0).all() and hi['e_dq'].max() < 0.05 * np.abs(hi['dq']).max()


# ---------------------------------------------------------------------------------------------------------------- configuration
def settings_of(config):
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel
    model = types.SimpleNamespace()
    CLIPBasedMultiModalReIDModel._read_loss_settings(model, config)
    return model


FIELDS = ('smooth_ap_weight', 'smooth_ap_temperature', 'smooth_ap_size', 'smooth_ap_normalize', 'smooth_ap_start_epoch')


def test_config_defaults_and_loss_settings():
    from prcv2025reid_amd.config import TrainingConfig
    c = TrainingConfig()
    assert tuple(getattr(c, n) for n in FIELDS) == (0.0, 0.01, 0, True, 0)
    for cfg in (c, types.SimpleNamespace()):                    # a config without the fields gets the defaults
        assert tuple(getattr(settings_of(cfg), n) for n in FIELDS) == (0.0, 0.01, 0, True, 0)
    m = settings_of(TrainingConfig(smooth_ap_weight=0.5, smooth_ap_temperature=0.02, smooth_ap_size=4096, smooth_ap_normalize=False, smooth_ap_start_epoch=3))
    assert tuple(getattr(m, n) for n in FIELDS) == (0.5, 0.02, 4096, False, 3)
    for bad, text in ((dict(smooth_ap_temperature=0.0), 'temperature must be > 0'), (dict(smooth_ap_temperature=float('inf')), 'temperature'),
                      (dict(smooth_ap_temperature=float('nan')), 'temperature'), (dict(smooth_ap_size=-1), 'smooth_ap_size'),
                      (dict(smooth_ap_size=8193), 'smooth_ap_size'), (dict(smooth_ap_size=2.5), 'smooth_ap_size')):
        with pytest.raises(ValueError, match=text):
            settings_of(TrainingConfig(**bad))


def test_the_pinned_names_did_not_move():
    from prcv2025reid_amd.model import AUX_TERMS, LOSS_FIELDS
    assert [n for n, _ in AUX_TERMS] == ['triplet', 'cross_triplet', 'hc_triplet', 'xbm', 'center']
    assert not any(n.startswith('smooth_ap') for n in LOSS_FIELDS) and len(LOSS_FIELDS) == 18


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_and_bound():
    from prcv2025reid_amd import _lib
    protos = header_prototypes()
    names = list(_lib.SIGNATURES)
    at = names.index('reid_cluster_centroids') + 1               # directly behind the ClusterNCE block
    assert names[at:at + len(NEW)] == NEW and list(protos)[at:at + len(NEW)] == NEW
    for name in NEW:
        ret, params = protos[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert (restype, list(argtypes)) == (ctype_of(ret), [ctype_of(p) for p in params]), name
    assert header_macro('REID_ABI_VERSION') == _lib.ABI_VERSION == 201


def good_arguments():
    base = 0x10000                                            # never dereferenced: every call is refused before a launch
    names = ('q', 'g', 'q_label', 'g_label', 'q_valid', 'g_valid', 'rows', 'rows1', 'mem_label', 'mem_valid', 'mem_valid1', 'q_ap', 'q_npos', 'g_ap',
             'g_npos', 'ws', 'result', 'gscale', 'dq', 'dg')
    a = dict(P=2, N=5, Mg=5, D=32, ldq=32, ldg=32, lddq=32, lddg=32, tau=0.01, normalize=1, eps=1e-12, Ga=9, Gb=9, ldga=32, ldgb=32, gallery_grad=0,
             with_grad=1, stream=None, **{n: base * (i + 1) for i, n in enumerate(names)})
    # the ring form: the galleries are a memory's sides
    a.update(ga='rows', ga_label='mem_label', ga_valid='mem_valid', gb='rows1', gb_label='mem_label', gb_valid='mem_valid1')
    return a


ORDER = {'fwd': ('q', 'ldq', 'g', 'ldg', 'q_label', 'g_label', 'q_valid', 'g_valid', 'P', 'N', 'Mg', 'D', 'tau', 'normalize', 'eps', 'ga', 'ldga', 'ga_label',
                 'ga_valid', 'Ga', 'gb', 'ldgb', 'gb_label', 'gb_valid', 'Gb', 'gallery_grad', 'with_grad', 'q_ap', 'q_npos', 'g_ap', 'g_npos', 'ws', 'result',
                 'stream'),
         'bwd': ('q_valid', 'g_valid', 'P', 'N', 'Mg', 'D', 'ws', 'gscale', 'dq', 'lddq', 'dg', 'lddg', 'stream'),
         'ws': ('P', 'N', 'Mg', 'D', 'Ga', 'Gb', 'with_grad')}
ENTRY = {'fwd': 'reid_smooth_ap_fwd', 'bwd': 'reid_smooth_ap_bwd', 'ws': 'reid_smooth_ap_ws_floats'}
BATCH_FORM = dict(gallery_grad=1, ga='g', ldga=32, ga_label='g_label', ga_valid='g_valid', Ga=5, gb='q', ldgb=32, gb_label='q_label', gb_valid='q_valid', Gb=5)


def violations():
    """(entry, overrides, a piece of the error text) of every requirement of include/reid_hip.h."""
    out = []
    for e in ('fwd', 'bwd', 'ws'):
        out += [(e, dict(P=0), 'P=0'), (e, dict(P=9), 'P=9'), (e, dict(N=0), 'N=0'), (e, dict(N=8193), 'N=8193'), (e, dict(Mg=0), 'Mg=0'),
                (e, dict(Mg=8193), 'Mg=8193'), (e, dict(D=0), 'D=0'), (e, dict(D=30), 'D=30'), (e, dict(D=1028), 'D=1028')]
    for e in ('fwd', 'ws'):
        out += [(e, dict(Ga=0), 'Ga=0'), (e, dict(Ga=8193), 'Ga=8193'), (e, dict(Gb=0), 'Gb=0'), (e, dict(Gb=8193), 'Gb=8193'), (e, dict(with_grad=2), 'with_grad=2')]
    out += [('fwd', {n: None}, 'null pointer') for n in ('q', 'g', 'q_label', 'g_label', 'rows', 'rows1', 'mem_label', 'q_ap', 'q_npos', 'g_ap', 'g_npos', 'ws', 'result')]
    out += [('bwd', {n: None}, 'null pointer') for n in ('ws', 'gscale', 'dq', 'dg')]
    out += [('fwd', dict(ldq=28), 'ldq=28'), ('fwd', dict(ldq=34), 'ldq=34'), ('fwd', dict(ldg=30), 'ldg=30'), ('fwd', dict(ldga=28), 'ldga=28'),
            ('fwd', dict(ldgb=33), 'ldgb=33'), ('fwd', dict(N=8192, P=8, ldq=2 ** 16), 'beyond 2^31'), ('fwd', dict(Gb=8192, P=8, ldgb=2 ** 16), 'beyond 2^31'),
            ('bwd', dict(lddq=30), 'lddq=30'), ('bwd', dict(lddg=16), 'lddg=16'), ('bwd', dict(N=8192, P=8, lddq=2 ** 16), 'beyond 2^31'),
            ('fwd', dict(tau=0.0), 'tau='), ('fwd', dict(tau=-0.01), 'tau='), ('fwd', dict(tau=float('nan')), 'tau='), ('fwd', dict(tau=float('inf')), 'tau='),
            ('fwd', dict(normalize=2), 'normalize=2'), ('fwd', dict(eps=-1.0), 'eps='), ('fwd', dict(gallery_grad=2), 'gallery_grad=2'),
            ('fwd', dict(q=0x10004), '16-byte aligned'), ('fwd', dict(g=0x20008), '16-byte aligned'), ('fwd', dict(rows=0x7000c), '16-byte aligned'),
            ('fwd', dict(rows1=0x80004), '16-byte aligned'), ('fwd', dict(ws=0x100004), '16-byte aligned'), ('bwd', dict(ws=0x100008), '16-byte aligned'),
            ('bwd', dict(dq=0x130004), '16-byte aligned'), ('bwd', dict(dg=0x140004), '16-byte aligned')]
    # the batch form takes the batch itself as its galleries, nothing else
    for k, v in (('ga', 'rows'), ('gb', 'rows1'), ('ga_label', 'q_label'), ('gb_label', 'g_label'), ('ga_valid', None), ('gb_valid', None), ('Ga', 4), ('Gb', 4),
                 ('ldga', 36), ('ldgb', 36)):
        out.append(('fwd', {**BATCH_FORM, k: v}, 'gallery_grad=1 needs the batch itself'))
    return out


def call(h, entry, args):
    def value(n):
        v = args[n]
        return args[v] if isinstance(v, str) else v          # a gallery argument names the buffer it points to
    return getattr(h, ENTRY[entry])(*[value(n) for n in ORDER[entry]])


def test_library_refuses_bad_arguments_before_any_launch():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    good = good_arguments()
    for path in _lib.LIB_PATHS.values():
        h = _lib.bind(ctypes.CDLL(path))
        # Hq, Hg | unit rows, two fp32 and one fp64 value per row | the score rows | their gradients; every piece a multiple of 4 floats
        R_, r4 = 2 * 5 + 5, lambda n: (n + 3) // 4 * 4
        small = R_ * 32 + 2 * r4(R_) + r4(2 * R_) + r4(2 * 5 * 9) + r4(2 * 5 * 9)
        assert h.reid_smooth_ap_ws_floats(2, 5, 5, 32, 9, 9, 0) == small
        assert h.reid_smooth_ap_ws_floats(2, 5, 5, 32, 9, 9, 1) == small + (2 * 5 + 2 * 5) * 32 + 2 * r4(2 * 5 * 9)
        seen = set()
        for entry, over, text in violations():
            rc = call(h, entry, {**good, **over})
            assert rc == -1, (entry, over, rc)
            assert text.encode() in h.reid_last_error() and ENTRY[entry].encode() in h.reid_last_error(), (entry, over, h.reid_last_error())
            seen.add(entry)
        assert seen == set(ENTRY)


def test_cpu_tensors_and_bad_arguments_are_refused():
    from prcv2025reid_amd import losses, ops, _lib
    q, g, ql, gl, _, _ = (None if a is None else torch.from_numpy(a) for a in R.make_case(2, 5, 5, 32, 3, 1))
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.smooth_ap(q, g, ql, gl)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.smooth_ap_xbm(q, g, ql, None)
    with pytest.raises(_lib.ReidHipError):
        ops.smooth_ap_fwd(q.reshape(10, 32), g, ql, gl, None, None, 0.01, True, 1e-12, True, torch.zeros(10), torch.zeros(10, dtype=torch.int32),
                          torch.zeros(10), torch.zeros(10, dtype=torch.int32), torch.zeros(1 << 16), torch.zeros(8), P=2)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            losses.smooth_ap(q, g, ql, gl, temperature=bad)
        with pytest.raises(ValueError, match='temperature'):
            losses.smooth_ap_xbm(q, g, ql, None, temperature=bad)
