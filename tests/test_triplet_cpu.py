"""CPU: the fp64 reference of the batch-hard triplet loss (triplet_ref.py) against a plain-loop implementation and against finite
differences, and the argument checks of reid_triplet_hard_fwd / reid_triplet_hard_bwd through the built library (no device)."""
import ctypes

import pytest
import torch

import triplet_ref as R


def _case(seed=0, P=4, K=2, D=6):
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(P).repeat_interleave(K)
    x = torch.randn(P, D, generator=g, dtype=torch.float64)[labels] * 0.7 + torch.randn(P * K, D, generator=g, dtype=torch.float64)
    return x, labels


@pytest.mark.parametrize('margin', [0.3, None])
@pytest.mark.parametrize('with_valid', [False, True])
def test_reference_equals_plain_loops_on_8_rows(margin, with_valid):
    x, labels = _case(1)
    valid = torch.tensor([1, 0, 1, 1, 1, 1, 0, 1], dtype=torch.uint8) if with_valid else None      # row 0 loses its only positive
    x[5] = x[4]                                                                                     # a true duplicate as the only positive
    ref, loop = R.reference(x, labels, valid, margin), R.loop_reference(x, labels, valid, margin)
    assert ref['idx_p'].tolist() == loop['idx_p'] and ref['idx_n'].tolist() == loop['idx_n']
    assert ref['n_active'] == loop['n_active'] == (4 if with_valid else 8)
    if with_valid:
        assert [int(ref['idx_p'][i]) for i in (0, 1, 6, 7)] == [-1] * 4 and [int(ref['idx_n'][i]) for i in (0, 1, 6, 7)] == [-1] * 4
    for k in ('d_ap', 'd_an', 'row_loss'):
        assert torch.allclose(ref[k], torch.tensor(loop[k], dtype=torch.float64), rtol=1e-14, atol=0)
    assert abs(ref['loss'] - loop['loss']) <= 1e-14 * (1 + abs(loop['loss']))
    assert abs(float(ref['d_ap'][4]) - 1e-6) <= 1e-20                                                         # the clamp


def test_reference_tie_goes_to_the_lowest_index():
    x, labels = _case(2, P=3, K=3)
    x[1] = x[0] + 100.0; x[2] = x[1]                      # identity 0: two equal rows, the farthest from row 0
    x[5] = x[0] + 0.001; x[7] = x[5]                      # identities 1 and 2: two equal rows, the nearest to row 0
    ref, loop = R.reference(x, labels, None, 0.3), R.loop_reference(x, labels, None, 0.3)
    d2 = R.pairwise_d2(x)
    assert d2[0, 1] == d2[0, 2] == d2[0].max() and d2[0, 5] == d2[0, 7] == d2[0, 3:].min()
    assert int(ref['idx_p'][0]) == 1 and int(ref['idx_n'][0]) == 5
    assert float(ref['gap_p'][0]) == 0.0 and float(ref['gap_n'][0]) == 0.0
    assert ref['idx_p'].tolist() == loop['idx_p'] and ref['idx_n'].tolist() == loop['idx_n']


@pytest.mark.parametrize('margin', [0.3, None])
def test_reference_gradient_equals_finite_differences(margin):
    x, labels = _case(3)
    valid = torch.tensor([1, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    ref = R.reference(x, labels, valid, margin)
    assert ref['n_active'] >= 5 and float(ref['row_loss'].max()) > 0
    assert float(torch.minimum(ref['gap_p'], ref['gap_n']).min()) > 1e-3                            # the selection is stable under the probe
    if margin is not None:
        z = (ref['d_ap'] - ref['d_an'] + margin)[ref['idx_p'] >= 0]
        assert float(z.abs().min()) > 1e-3                                                          # away from the hinge's kink
    dx = R.gradient(x, ref['idx_p'], ref['idx_n'], margin, dloss=1.7)
    h = 1e-6
    worst = 0.0
    for i in range(x.shape[0]):
        for c in range(x.shape[1]):
            xp, xm = x.clone(), x.clone()
            xp[i, c] += h; xm[i, c] -= h
            fd = 1.7 * (R.reference(xp, labels, valid, margin)['loss'] - R.reference(xm, labels, valid, margin)['loss']) / (2 * h)
            worst = max(worst, abs(fd - float(dx[i, c])))
    assert worst <= 1e-8, worst
    assert float(dx[5].abs().max()) == 0.0                                                          # the invalid row gets no gradient


@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    return {f: _lib.bind(ctypes.CDLL(p)) for f, p in _lib.LIB_PATHS.items()}


@pytest.mark.parametrize('flavor', ['bf16', 'f16'])
def test_entry_points_check_their_arguments_without_a_device(libs, flavor):
    h = libs[flavor]
    buf = (ctypes.c_float * 64)()                         # host memory: only its (16-byte aligned) address is looked at before the refusal
    p = ctypes.addressof(buf)
    p += (-p) % 16
    fwd = lambda x=p, ldx=8, rows=4, D=8, out=p: h.reid_triplet_hard_fwd(x, ldx, p, None, rows, D, 0.3, out, p, p, p, p, p, None)
    bwd = lambda x=p, ldx=8, rows=4, D=8, dx=p, lddx=8: h.reid_triplet_hard_bwd(x, ldx, rows, D, 0.3, p, p, p, p, p, p, dx, lddx, None)
    for call, name in ((fwd, b'reid_triplet_hard_fwd'), (bwd, b'reid_triplet_hard_bwd')):
        assert call(x=None) == -1 and name + b': null pointer' in h.reid_last_error()
        for D in (0, 6, 1028):
            assert call(D=D, ldx=1028) == -1 and name in h.reid_last_error() and b'D=' in h.reid_last_error()
        for rows in (0, 8193):
            assert call(rows=rows) == -1 and b'rows=' in h.reid_last_error()
        assert call(ldx=4) == -1 and b'ldx=4' in h.reid_last_error()                 # ldx < D
        assert call(ldx=10) == -1 and b'ldx=10' in h.reid_last_error()               # not a multiple of 4
        assert call(x=p + 4) == -1 and b'16-byte aligned' in h.reid_last_error()
    assert fwd(out=None) == -1 and b'null pointer' in h.reid_last_error()
    assert bwd(dx=None) == -1 and b'null pointer' in h.reid_last_error()
    assert bwd(lddx=4) == -1 and b'lddx=4' in h.reid_last_error()
    assert bwd(dx=p + 8) == -1 and b'16-byte aligned' in h.reid_last_error()
    assert h.reid_triplet_hard_fwd(p, 1 << 20, p, None, 8192, 8, 0.3, p, p, p, p, p, p, None) == -1 and b'2^31' in h.reid_last_error()
    assert h.reid_triplet_hard_fwd(p, 8, p, None, 4, 8, float('nan'), p, p, p, p, p, p, None) == -1 and b'NaN' in h.reid_last_error()


def test_config_and_head_expose_the_loss():
    from prcv2025reid_amd import _lib, losses
    from prcv2025reid_amd.config import TrainingConfig
    cfg = TrainingConfig()
    assert cfg.triplet_weight == 0.0 and cfg.triplet_margin == 0.3
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.batch_hard_triplet(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))
