"""CPU: the C-ABI libraries build, load and export every symbol include/reid_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'reid_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    names = re.findall(r'^\s*(?:const\s+char\s*\*|int64_t|int32_t|int)\s+(reid_\w+)\s*\(', src, flags=re.M)
    return sorted(set(names))


@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    return {f: ctypes.CDLL(p) for f, p in _lib.LIB_PATHS.items()}


def test_header_declares_what_python_binds():
    from prcv2025reid_amd import _lib
    assert set(_lib.EXPORTS) == set(header_functions())


@pytest.mark.parametrize('flavor', ['bf16', 'f16'])
def test_library_exports_every_declared_symbol_abi_201(libs, flavor):
    h = libs[flavor]
    missing = [n for n in header_functions() if not hasattr(h, n)]
    assert not missing, missing
    # ABI 201: reid_layernorm_bwd's overflow flag (200 was the round 2 ABI: reid_set_knob, fused SDM); the header says the same
    src = open(os.path.join(ROOT, 'include', 'reid_hip.h')).read()
    assert h.reid_version() == int(re.search(r'#define\s+REID_ABI_VERSION\s+(\d+)', src).group(1)) == 201
    assert h.reid_flavor() == (1 if flavor == 'f16' else 0)


def test_header_abi_version_is_the_bound_one():
    from prcv2025reid_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'reid_hip.h')).read()
    assert int(re.search(r'#define\s+REID_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.ABI_VERSION == 201


def _stub_library(version, flavor):
    # a stand-in for a loaded CDLL: every export present, reid_version / reid_flavor answering as given, no device code
    import types
    from prcv2025reid_amd import _lib
    h = types.SimpleNamespace(**{n: (lambda *a: 0) for n in _lib.EXPORTS})
    h.reid_version = lambda: version
    h.reid_flavor = lambda: flavor
    return h


@pytest.mark.parametrize('version', [200, 202])
def test_binding_refuses_other_abi_version(version):
    from prcv2025reid_amd import _lib
    with pytest.raises(_lib.ReidHipError, match=rf'ABI version {version}, this package binds 201: stale build, run `python -m prcv2025reid_amd.build --force`'):
        _lib._checked(_stub_library(version, 1 if _lib.flavor() == 'f16' else 0), 'stub.so')


def test_binding_accepts_current_abi_version():
    from prcv2025reid_amd import _lib
    h = _stub_library(201, 1 if _lib.flavor() == 'f16' else 0)
    assert _lib._checked(h, 'stub.so') is h
    with pytest.raises(_lib.ReidHipError, match='other 16-bit flavor'):
        _lib._checked(_stub_library(201, 0 if _lib.flavor() == 'f16' else 1), 'stub.so')


def test_argument_validation_needs_no_gpu(libs):
    # bad arguments are rejected on the host before any launch
    from prcv2025reid_amd._lib import GemmArgs
    h = libs['bf16']
    h.reid_last_error.restype = ctypes.c_char_p
    a = GemmArgs()
    assert h.reid_mer_gemm(ctypes.byref(a), None) == -1
    assert b'non-null' in h.reid_last_error()
    assert h.reid_attn_fwd(None, 0, None, None, 0, None, 1, 500, 12, 0, None) == -1
    assert h.reid_gemm_tn(None, None, None, 1, 8, 8, 8, 8, 8, ctypes.c_float(1), ctypes.c_float(0), None) == -1


def test_model_refuses_cpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from prcv2025reid_amd import _lib
    from prcv2025reid_amd.config import TrainingConfig
    from prcv2025reid_amd.model import CLIPBasedMultiModalReIDModel
    with pytest.raises(_lib.ReidHipError):
        CLIPBasedMultiModalReIDModel(TrainingConfig(device='cpu'))
