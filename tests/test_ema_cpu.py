"""CPU: the weight EMA's reference (tests/ema_ref.py), its C ABI declarations and bindings, the optimizer's keywords and the
checkpoint round trip of ``ema_state_dict`` with a stand-in optimizer (the real one needs the HIP device)."""
import contextlib
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import ema_ref as er
from test_cabi_cpu import header_prototypes, header_struct, layout, ctype_of

NEW_EXPORTS = {'reid_ema_entry_bytes': 0, 'reid_ema_update': 7, 'reid_ema_swap': 3}


def test_weight_schedule_closed_form():
    # warm-up: d_t = (1 + t) / (10 + t) while that is below the decay
    for t, (num, den) in {1: (2, 11), 2: (3, 12), 3: (4, 13)}.items():
        assert er.ema_decay_at(0.999, True, t) == num / den
        assert er.ema_weight(0.999, True, t) == np.float32(1.0 - num / den)
    # the cap takes over once (1 + t) / (10 + t) > (float)0.9 = 0.89999998: at t = 80, where the ratio is 0.9 in double
    d09 = float(np.float32(0.9))
    assert d09 < 0.9 == 81.0 / 90.0
    assert er.ema_decay_at(0.9, True, 79) == 80.0 / 89.0 < d09
    assert er.ema_decay_at(0.9, True, 80) == d09
    assert er.ema_decay_at(0.9, True, 10 ** 6) == d09
    assert er.ema_weight(0.9, True, 80) == er.ema_weight(0.9, False, 1) == np.float32(1.0 - d09)
    # no warm-up: the decay from the first step on
    for t in (1, 2, 3, 1000):
        assert er.ema_decay_at(0.999, False, t) == float(np.float32(0.999))
    assert er.ema_weight(0.999, False, 1).dtype == np.float32


def test_update_against_torch_lerp():
    # torch.lerp evaluates s + w (p - s) for w < 0.5 and p - (p - s)(1 - w) otherwise, and may contract either into a fused
    # multiply-add.  With u = 2^-24: the three-rounding form is within 3u (|p| + |s|) of the exact value (2u on |w (p - s)| <= |p| + |s|,
    # u on the result), lerp's second form, with one more rounding, within 4u (|p| + |s|), contracted forms within less.  Margin: the
    # sum, rounded up to 8u (|p| + |s|) per element.
    u = 2.0 ** -24
    s0, ps = er.kernel_vectors()
    for decay, warmup, t in ((0.9, False, 1), (0.999, False, 1), (0.999, True, 1), (0.999, True, 7)):
        w = er.ema_weight(decay, warmup, t)
        for p, s in zip(ps[0], s0):
            got = er.ema_update(p, s, w)
            want = torch.lerp(torch.from_numpy(s), torch.from_numpy(p), float(w)).numpy()
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            assert (err <= 8 * u * (np.abs(p).astype(np.float64) + np.abs(s))).all(), (decay, warmup, t, float(err.max()))


def test_update_properties():
    p = np.array([1.5, -0.0, 3.0, 1e-40, np.inf], dtype=np.float32)
    assert np.array_equal(er.ema_update(p[:4], p[:4], np.float32(0.1)), p[:4])               # s == p stays put (denormal included)
    with np.errstate(invalid='ignore'):
        assert np.isnan(er.ema_update(p[4:], p[4:], np.float32(0.1))[0])                     # inf - inf
    # the three roundings, spelled out on one element
    s, q, w = np.float32(0.3), np.float32(1.7), np.float32(0.1)
    assert er.ema_update([q], [s], w)[0] == np.float32(s + np.float32(w * np.float32(q - s)))


def test_fixture_power_sees_a_contraction():
    # the bit test of tests/test_ema_gpu.py can tell the un-fused update from fma(w, p - s, s) on its own vectors
    s0, ps = er.kernel_vectors()
    for decay, warmup in ((0.999, True), (0.999, False)):
        w = er.ema_weight(decay, warmup, 1)
        differ = sum(int((er.ema_update(p, s, w).view(np.int32) != er.ema_update_fused(p, s, w).view(np.int32)).sum())
                     for p, s in zip(ps[0], s0))
        assert differ >= 1, (decay, warmup)
    big = er.KERNEL_SIZES.index(131079)
    w = er.ema_weight(0.999, False, 1)
    assert (er.ema_update(ps[0][big], s0[big], w).view(np.int32) != er.ema_update_fused(ps[0][big], s0[big], w).view(np.int32)).any()


def test_header_declares_the_ema_exports_and_python_binds_them():
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.trainer import _EmaEntry
    protos = header_prototypes()
    for name, arity in NEW_EXPORTS.items():
        assert name in protos, name
        ret, params = protos[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(params) == len(argtypes) == arity, name
        assert (restype, list(argtypes)) == (ctype_of(ret), [ctype_of(p) for p in params]), name
    assert [t for _, t in layout(_EmaEntry._fields_)] == [t for _, t in layout(header_struct('reid_ema_entry'))]
    assert ctypes.sizeof(_EmaEntry) == 24
    assert _lib.ABI_VERSION == 201                          # exports were only added


def test_library_exports_and_refuses_bad_arguments():
    from prcv2025reid_amd import build, _lib
    from prcv2025reid_amd.trainer import _EmaEntry
    build.build(verbose=False)
    for path in _lib.LIB_PATHS.values():
        h = _lib.bind(ctypes.CDLL(path))
        assert h.reid_ema_entry_bytes() == ctypes.sizeof(_EmaEntry)
        t = 0x1000                                           # never dereferenced: every call below is refused before a launch
        for decay in (0.0, 1.0, -0.5, 1.5, float('nan')):
            assert h.reid_ema_update(t, 1, decay, 1, 1, None, None) == -1
            assert b'decay' in h.reid_last_error()
        assert h.reid_ema_update(None, 1, 0.9, 1, 1, None, None) == -1
        assert h.reid_ema_update(t, 0, 0.9, 1, 1, None, None) == -1
        assert h.reid_ema_update(t, 1, 0.9, 1, 0, None, None) == -1      # device counter without the state
        assert b'device counter' in h.reid_last_error()
        assert h.reid_ema_update(t, 1, 0.9, 1, -1, t, None) == -1
        assert h.reid_ema_swap(None, 1, None) == -1
        assert h.reid_ema_swap(t, 0, None) == -1


def test_fused_adamw_accepts_the_ema_keywords():
    from prcv2025reid_amd.trainer import FusedAdamW
    sig = inspect.signature(FusedAdamW.__init__).parameters
    assert sig['ema_decay'].default is None and sig['ema_warmup'].default is True and tuple(sig['ema_buffers'].default) == ()
    for name in ('swap_ema', 'ema_weights', 'ema_state', 'load_ema_state', 'reset_ema', 'ema_num_updates'):
        assert hasattr(FusedAdamW, name), name
    assert 'device_counters' in inspect.signature(FusedAdamW.step).parameters


# ---------------------------------------------------------------------------------------------------------- checkpoint
class _Model:
    """state_dict / arch carrier (the real model needs the HIP device)."""
    def __init__(self, arch, sd, C):
        self.arch, self._sd, self.num_classes = arch, sd, C

    def state_dict(self):
        return self._sd

    def load_state_dict(self, sd, strict=True):
        self._sd = {k: sd[k].clone() for k in self._sd}


class _EmaOpt:
    """Duck-typed stand-in for FusedAdamW's EMA interface over some keys of a _Model's state dict."""
    def __init__(self, model, keys, decay=0.9):
        self.model, self.keys, self.ema_decay, self.ema_warmup, self.num_updates = model, keys, decay, True, 0
        self.shadow = [model._sd[k].clone() for k in keys]
        self.resets = 0

    def state_dict(self):
        return {'state': {}, 'param_groups': []}

    def ema_state(self):
        return dict(decay=self.ema_decay, warmup=self.ema_warmup, num_updates=self.num_updates, shadows=[s.clone() for s in self.shadow])

    def load_ema_state(self, st):
        self.ema_decay, self.ema_warmup, self.num_updates = st['decay'], st['warmup'], st['num_updates']
        self.shadow = [s.clone() for s in st['shadows']]

    def reset_ema(self):
        self.shadow = [self.model._sd[k].clone() for k in self.keys]
        self.num_updates = 0
        self.resets += 1

    def _swap(self):
        for i, k in enumerate(self.keys):
            self.model._sd[k], self.shadow[i] = self.shadow[i], self.model._sd[k]

    @contextlib.contextmanager
    def ema_weights(self):
        self._swap()
        try:
            yield self
        finally:
            self._swap()


OLD_KEYS = {'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'best_map', 'num_classes', 'config'}
EMA_KEYS = ['bn_neck.classifier.weight', 'bn_neck.bn.weight', 'bn_neck.bn.running_mean']


def _tiny():
    from prcv2025reid_amd.config import TrainingConfig, arch_of
    from prcv2025reid_amd.weights import seeded_state
    cfg = TrainingConfig(device='cpu', mer_lora_rank=4, vision_hidden_dim=128, vision_layers=2, vision_heads=2, vision_mlp_dim=256,
                         text_layers=2, text_mlp_dim=1024, text_vocab=1024, text_eos_id=1023, text_bos_id=1022)
    arch = arch_of(cfg)
    return cfg, arch, seeded_state(arch, 5, 3)


def test_checkpoint_round_trips_ema_state(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    opt = _EmaOpt(m, EMA_KEYS, decay=0.97)
    opt.shadow = [s + 0.25 for s in opt.shadow]; opt.num_updates = 7; opt.ema_warmup = False
    path = str(tmp_path / 'c' / 'ema.pth')
    ck.save_checkpoint(m, opt, None, 2, 0.5, cfg, path)
    back = torch.load(path, map_location='cpu', weights_only=False)
    assert set(back) == OLD_KEYS | {'ema_state_dict'}
    e = back['ema_state_dict']
    assert set(e) == {'decay', 'warmup', 'num_updates', 'shadows'}
    assert e['decay'] == 0.97 and e['warmup'] is False and e['num_updates'] == 7
    assert all(s.device.type == 'cpu' and torch.equal(s, w) for s, w in zip(e['shadows'], opt.shadow))
    for k in EMA_KEYS:                                        # the live weights were written, not the average
        assert torch.equal(back['model_state_dict'][k], sd[k])

    m2 = _Model(arch, {k: v + 1.0 for k, v in sd.items()}, 5)
    opt2 = _EmaOpt(m2, EMA_KEYS, decay=0.5)
    info = ck.load_checkpoint(path, m2, opt2)
    assert info['epoch'] == 2 and 'ema_state_dict' not in info
    assert opt2.ema_decay == 0.97 and opt2.ema_warmup is False and opt2.num_updates == 7 and opt2.resets == 0
    assert all(torch.equal(a, b) for a, b in zip(opt2.shadow, opt.shadow))


def test_checkpoint_without_ema_keeps_the_old_keys_and_resets_on_load(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    plain = _EmaOpt(m, EMA_KEYS); plain.ema_decay = None       # an optimizer without an average
    path = str(tmp_path / 'c' / 'plain.pth')
    ck.save_checkpoint(m, plain, None, 1, 0.1, cfg, path)
    ck.save_checkpoint(m, None, None, 1, 0.1, cfg, str(tmp_path / 'c' / 'none.pth'))
    for f in ('plain.pth', 'none.pth'):
        assert set(torch.load(str(tmp_path / 'c' / f), map_location='cpu', weights_only=False)) == OLD_KEYS
    with pytest.raises(ValueError, match='use_ema'):
        ck.save_checkpoint(m, plain, None, 1, 0.1, cfg, path, use_ema=True)
    # loaded into an optimizer WITH an average: the shadows restart from the loaded weights, not from the construction-time ones
    m2 = _Model(arch, {k: v + 1.0 for k, v in sd.items()}, 5)
    opt2 = _EmaOpt(m2, EMA_KEYS)
    opt2.num_updates = 3
    ck.load_checkpoint(path, m2, opt2)
    assert opt2.resets == 1 and opt2.num_updates == 0
    assert all(torch.equal(s, sd[k]) for s, k in zip(opt2.shadow, EMA_KEYS))


def test_checkpoint_use_ema_writes_the_average(tmp_path):
    from prcv2025reid_amd import checkpoint as ck
    cfg, arch, sd = _tiny()
    m = _Model(arch, {k: v.clone() for k, v in sd.items()}, 5)
    opt = _EmaOpt(m, EMA_KEYS)
    opt.shadow = [s * 0.5 + 0.125 for s in opt.shadow]
    want = [s.clone() for s in opt.shadow]
    path = str(tmp_path / 'c' / 'avg.pth')
    ck.save_checkpoint(m, opt, None, 1, 0.1, cfg, path, use_ema=True)
    back = torch.load(path, map_location='cpu', weights_only=False)
    plain = ck.full_state_dict(m)
    assert set(back['model_state_dict']) == set(plain)
    for k, v in back['model_state_dict'].items():
        assert torch.equal(v, want[EMA_KEYS.index(k)] if k in EMA_KEYS else plain[k]), k
    assert all(torch.equal(a, b) for a, b in zip(back['ema_state_dict']['shadows'], want))
    assert all(torch.equal(m._sd[k], sd[k]) for k in EMA_KEYS)          # swapped back
