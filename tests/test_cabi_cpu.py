"""CPU: the C-ABI libraries build, load and export every symbol include/reid_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_code():
    src = open(os.path.join(ROOT, 'include', 'reid_hip.h')).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', src, flags=re.S))


def header_prototypes():
    """name -> (return type, [parameter types]) of every function include/reid_hip.h declares, in header order."""
    code = header_code()
    protos = {}
    for ret, name, params in re.findall(r'^\s*([A-Za-z_][\w ]*?[\s*]+)(reid_\w+)\s*\(([^)]*)\)\s*;', code, flags=re.M):
        params = [] if params.strip() in ('', 'void') else [re.sub(r'\w+\s*$', '', p) for p in params.split(',')]
        protos[name] = (ret, params)
    assert set(re.findall(r'\b(reid_\w+)\s*\(', code)) == set(protos), 'a declaration the parser above does not read'
    return protos


def header_macro(name):
    return int(re.search(rf'#define\s+{name}\s+(\d+)', header_code()).group(1))


def ctype_of(c_type):
    """The ctypes type _lib.SIGNATURES uses for a C type of the header."""
    from prcv2025reid_amd._lib import GemmArgs, GemmPlan
    t = ' '.join(c_type.replace('*', ' * ').replace('const ', ' ').split())
    if t.endswith('*'):
        return {'char *': ctypes.c_char_p, 'reid_gemm_args *': ctypes.POINTER(GemmArgs),
                'reid_gemm_plan *': ctypes.POINTER(GemmPlan)}.get(t, ctypes.c_void_p)
    enums = re.findall(r'typedef\s+enum\s*\{[^}]*\}\s*(\w+)\s*;', header_code())
    return {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
            **{e: ctypes.c_int32 for e in enums}}[t]


def header_struct(name):
    """[(field, ctypes type)] of ``typedef struct ... {...} name;``, arrays as ctypes arrays of the macro's length."""
    body = re.search(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*' + name + r'\s*;', header_code()).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        first, *more = [d.strip() for d in decl.split(',')]
        c_type, first = re.fullmatch(r'(.*?)(\w+(?:\s*\[\s*\w+\s*\])?)', first, flags=re.S).groups()
        for declarator in [first] + more:
            field, n = re.fullmatch(r'(\w+)(?:\s*\[\s*(\w+)\s*\])?', declarator).groups()
            t = ctype_of(c_type)
            fields.append((field, t * (int(n) if n.isdigit() else header_macro(n)) if n else t))
    return fields


def layout(fields):
    # ctypes array types compare by element type and length
    return [(n, (t._type_, t._length_) if issubclass(t, ctypes.Array) else t) for n, t in fields]


@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import build, _lib
    build.build(verbose=False)
    return {f: _lib.bind(ctypes.CDLL(p)) for f, p in _lib.LIB_PATHS.items()}


def test_header_declares_what_python_binds():
    # every prototype, mapped through the table's type vocabulary, is the table's entry: same names in header order,
    # same return type, same parameter types in order
    from prcv2025reid_amd import _lib
    protos = header_prototypes()
    assert list(_lib.SIGNATURES) == list(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert (restype, list(argtypes)) == (ctype_of(ret), [ctype_of(p) for p in params]), name


def test_structs_match_their_ctypes_mirrors():
    from prcv2025reid_amd._lib import GemmArgs, GemmPlan
    from prcv2025reid_amd.trainer import _Entry
    gemm = header_struct('reid_gemm_args')
    assert ('row_group_end', ctypes.c_int32 * header_macro('REID_GEMM_MAX_GROUPS')) in gemm
    assert layout(GemmArgs._fields_) == layout(gemm)
    assert layout(GemmPlan._fields_) == layout(header_struct('reid_gemm_plan'))
    # the optimizer entry's Python field names are shorter than the header's: types and order only
    assert [t for _, t in layout(_Entry._fields_)] == [t for _, t in layout(header_struct('reid_opt_entry'))]


def test_package_calls_pass_every_declared_argument():
    # ctypes raises for too few arguments but passes extra ones on silently: every call of an entry point in the package
    # passes exactly the declared number of positional arguments
    import ast
    import glob
    from prcv2025reid_amd import _lib
    calls, wrong = 0, []
    for path in sorted(glob.glob(os.path.join(ROOT, 'prcv2025reid_amd', '*.py'))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in _lib.SIGNATURES:
                calls += 1
                if (node.keywords or any(isinstance(a, ast.Starred) for a in node.args)
                        or len(node.args) != len(_lib.SIGNATURES[node.func.attr][1])):
                    wrong.append(f'{os.path.basename(path)}:{node.lineno} {node.func.attr}')
    assert calls and not wrong, wrong


def test_bound_library_refuses_malformed_calls(libs):
    # ctypes rejects these before the call: the last error is still the one gemm_tn set
    h = libs['bf16']
    assert h.reid_gemm_tn(None, None, None, 1, 8, 8, 8, 8, 8, 1.0, 0.0, None) == -1
    before = h.reid_last_error()
    with pytest.raises(TypeError):
        h.reid_attn_fwd(None, 0, None, None, 0, None, 1, 500, 12, 0, 0)             # no stream
    with pytest.raises(ctypes.ArgumentError):
        h.reid_attn_fwd(None, 0.5, None, None, 0, None, 1, 500, 12, 0, 0, None)     # a float for int32_t ld
    assert h.reid_last_error() == before


@pytest.mark.parametrize('flavor', ['bf16', 'f16'])
def test_library_exports_every_declared_symbol_abi_201(libs, flavor):
    h = libs[flavor]
    missing = [n for n in header_prototypes() if not hasattr(h, n)]
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
    a = GemmArgs()
    assert h.reid_mer_gemm(ctypes.byref(a), None) == -1
    assert b'non-null' in h.reid_last_error()
    assert h.reid_attn_fwd(None, 0, None, None, 0, None, 1, 500, 12, 0, 0, None) == -1
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
