"""CPU: the center loss's references against each other (center_ref.py: the float32 loop against the fp64 form), the config defaults,
the CPU-tensor error, the argument checks of the C entry points (refused before any launch, so no device is needed), the state of
ClassCenters, and the checkpoint round trip of ``center_state_dict`` with a stand-in model (the real one needs the HIP device)."""
import ctypes

import numpy as np
import pytest
import torch

import center_ref as R
from test_ema_cpu import _Model, _tiny, OLD_KEYS


@pytest.mark.parametrize('shape', [(2, 5, 260, 4), (5, 16, 512, 6), (1, 7, 4, 3)])
def test_loop_form_equals_the_fp64_form(shape):
    S, N, D, C = shape
    loop = np.zeros((C, D), dtype=np.float32)
    c64 = torch.zeros(C, D, dtype=torch.float64)
    moved = set()
    for s in range(1, 6):
        x, labels, valid = R.stream_step(S, N, D, C, s)
        f = R.loop_forward(x, labels, valid, loop)
        xa = x.double().requires_grad_(True)
        L, n, d2 = R.ref64_loss(xa, labels, valid, torch.from_numpy(loop))
        assert f['n_used'] == n > 0
        assert abs(float(f['loss']) - float(L.detach())) <= R.loss_bound(D) * float(L.detach())
        assert bool(((torch.from_numpy(f['d2']).double() - d2).abs() <= R.d2_bound(D) * d2).all())
        # the gradient, with an upstream factor that is not 1
        (L * 0.75).backward()
        dx = R.loop_backward(f['diff'], f['used'], f['n_used'], 0.75)
        g = xa.grad.reshape(S * N, D)
        assert float(g.abs().max()) > 0
        assert float((torch.from_numpy(dx).double() - g).abs().max()) <= 1e-6 * float(g.abs().max())
        # the update: both forms step from their own table
        c64 = R.ref64_update(x, labels, valid, c64, 0.5)
        loop = R.loop_update(f['diff'], f['d2'], labels, f['used'], loop, 0.5)
        moved |= {int(j) for r, j in enumerate(labels.repeat(S).tolist()) if f['used'][r]}
    assert float((torch.from_numpy(loop).double() - c64).abs().max()) <= 1e-6 * float(c64.abs().max())
    assert len(moved) >= min(C, 2) and float(c64.abs().max()) > 0.1


def test_update_skips_non_finite_rows_and_absent_classes():
    S, N, D, C = 2, 5, 8, 4
    x, labels, valid, centers = R.make_case(S, N, D, C, 3)
    labels = torch.tensor([0, 0, 1, 2, 2]); valid = torch.ones(S, N, dtype=torch.uint8)
    x[0, 0, 3] = float('nan'); x[1, 3, 0] = float('inf')
    f = R.loop_forward(x, labels, valid, centers.numpy())
    assert not np.isfinite(f['loss']) and f['n_used'] == S * N
    new = R.loop_update(f['diff'], f['d2'], labels, f['used'], centers.numpy(), 0.5)
    assert np.isfinite(new).all() and np.array_equal(new[3].view(np.int32), centers.numpy()[3].view(np.int32))
    # the same as a batch without those two rows
    valid2 = valid.clone(); valid2[0, 0] = 0; valid2[1, 3] = 0
    f2 = R.loop_forward(torch.nan_to_num(x, 0.0, 0.0, 0.0), labels, valid2, centers.numpy())
    new2 = R.loop_update(f2['diff'], f2['d2'], labels, f2['used'], centers.numpy(), 0.5)
    assert np.array_equal(new.view(np.int32), new2.view(np.int32))
    c64 = R.ref64_update(x, labels, valid, centers, 0.5)
    assert float((torch.from_numpy(new).double() - c64).abs().max()) <= 1e-6 * float(c64.abs().max())


def test_config_defaults():
    from prcv2025reid_amd.config import TrainingConfig
    c = TrainingConfig()
    assert (c.center_weight, c.center_alpha, c.center_source) == (0.0, 0.5, 'fused')


def test_cpu_tensors_are_refused():
    from prcv2025reid_amd import losses, _lib
    x, labels, valid, _ = R.make_case(2, 5, 8, 4, 1)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.center_loss(x, labels, losses.ClassCenters(4, 8, 'cpu'))
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.center_loss(x[0], labels, None, valid=valid[0])
    with pytest.raises(_lib.ReidHipError):
        from prcv2025reid_amd import ops
        ops.center_fwd(x[0], labels, None, torch.zeros(4, 8), torch.zeros(64), torch.zeros(5), torch.zeros(2))


def test_class_centers_state_round_trip():
    from prcv2025reid_amd.losses import ClassCenters
    a = ClassCenters(6, 12, 'cpu')
    assert a.centers.shape == (6, 12) and a.centers.dtype == torch.float32 and float(a.centers.abs().max()) == 0.0
    a.centers.copy_(torch.randn(6, 12, generator=torch.Generator().manual_seed(1)))
    st = a.state()
    assert set(st) == {'centers'} and st['centers'].device.type == 'cpu' and st['centers'].data_ptr() != a.centers.data_ptr()
    b = ClassCenters(6, 12, 'cpu')
    table = b.centers
    b.load_state(st)
    assert b.centers is table and torch.equal(b.centers, a.centers)          # in place: a captured graph's pointer stays valid
    with pytest.raises(ValueError, match='centres'):
        ClassCenters(5, 12, 'cpu').load_state(st)
    with pytest.raises(ValueError, match='centres'):
        ClassCenters(6, 8, 'cpu').load_state(st)
    b.reset()
    assert b.centers is table and float(b.centers.abs().max()) == 0.0
    for bad in ((0, 8), (4, 6), (4, 0), (4, 1028)):
        with pytest.raises(ValueError):
            ClassCenters(*bad, 'cpu')


def test_library_refuses_bad_arguments_before_any_launch():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    base = 0x10000                                            # never dereferenced: every call below is refused before a launch
    good = dict(S=2, N=5, D=8, C=4, ldx=8, lddx=8, alpha=0.5, stream=None, valid=None,
                **{n: base * (i + 1) for i, n in enumerate(('x', 'labels', 'centers', 'ws', 'd2', 'result', 'dloss', 'dx'))})
    for path in _lib.LIB_PATHS.values():
        h = _lib.bind(ctypes.CDLL(path))
        assert h.reid_center_ws_floats(2, 5, 8) == 2 * 5 * 8 + 2 * 5
        assert h.reid_center_ws_floats(9, 8192, 1024) == 9 * 8192 * 1025
        for entry, over, text in R.violations():
            rc = R.call(h, entry, R.bad_arguments(good, over))
            assert rc == -1, (entry, over, rc)
            assert text.encode() in h.reid_last_error() and b'reid_center_' in h.reid_last_error(), (entry, over, h.reid_last_error())


# ---------------------------------------------------------------------------------------------------------- checkpoint
class _Centers:
    """What checkpoint.py asks of model.centers."""
    def __init__(self, t):
        self.centers = t

    def state(self):
        return {'centers': self.centers.clone()}


def test_checkpoint_round_trips_center_state(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    from prcv2025reid_amd.losses import ClassCenters
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    table = torch.randn(5, 16, generator=torch.Generator().manual_seed(2))
    m.centers = _Centers(table.clone()); m.center_source = 'modalities'
    path = str(tmp_path / 'c' / 'center.pth')
    ck.save_checkpoint(m, None, None, 2, 0.5, cfg, path)
    back = torch.load(path, map_location='cpu', weights_only=False)
    assert set(back) == OLD_KEYS | {'center_state_dict'}
    assert set(back['center_state_dict']) == {'centers', 'center_source'} and back['center_state_dict']['center_source'] == 'modalities'
    assert torch.equal(back['center_state_dict']['centers'], table)
    # into a model without a table: made on load; into one that has a table: filled in place; another shape: refused
    m2 = _Model(arch, {k: v + 1.0 for k, v in sd.items()}, 5)
    m2.centers = None
    info = ck.load_checkpoint(path, m2)
    assert info['epoch'] == 2 and 'center_state_dict' not in info and 'ema_state_dict' not in info
    assert isinstance(m2.centers, ClassCenters) and torch.equal(m2.centers.centers, table)
    m3 = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    m3.centers = ClassCenters(5, 16, 'cpu'); held = m3.centers.centers
    ck.load_checkpoint(path, m3)
    assert m3.centers.centers is held and torch.equal(held, table)
    m3.centers = ClassCenters(5, 8, 'cpu')
    with pytest.raises(ValueError, match='centres'):
        ck.load_checkpoint(path, m3)


def test_checkpoint_without_centers_keeps_the_old_keys(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    path = str(tmp_path / 'c' / 'plain.pth')
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, path)
    m.centers = None
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, str(tmp_path / 'c' / 'none.pth'))
    for f in ('plain.pth', 'none.pth'):
        assert set(torch.load(str(tmp_path / 'c' / f), map_location='cpu', weights_only=False)) == OLD_KEYS
    m.centers = 'untouched'
    ck.load_checkpoint(path, m)                               # a checkpoint without the key leaves the model's table alone
    assert m.centers == 'untouched'
