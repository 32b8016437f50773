"""CPU: reid_mer_gemm's dispatch, asked of the library itself (reid_mer_gemm_plan launches nothing and touches no device), in both flavors.

Frozen routes: tests/golden/gemm_plan_routes.json was written by the hand-kept Python description of the dispatch that
test_gemm_exact_gpu.py carried before the plan existed -- an independent statement of the policy, not output of the code under test.
Invariants: what any plan must satisfy so that the kernels cover the problem and only get shapes they were built for."""
import ctypes
import itertools
import json
import os
import re

import pytest
import torch

from gemm_cases import CASES, S, STEP_CASES, case_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_plan_routes.json')
TILED, PP, PPS = range(3)
GENERIC, PLAIN16, RES32, PLAIN16H = 0, 1, 2, 7
BY_NAME = {c['name']: c for c in CASES + STEP_CASES}


@pytest.fixture(scope='module', params=['bf16', 'f16'])
def ops(request):
    from prcv2025reid_amd import build, ops as o, _lib
    build.build(verbose=False)
    _lib.set_flavor(request.param)
    yield o
    _lib.set_flavor('bf16')


def golden_rows(flavor):
    return [r for r in json.load(open(GOLDEN)) if r['flavor'] == flavor]


def route(plan):
    from prcv2025reid_amd import _lib
    return dict(kernel=_lib.GEMM_KERNELS[plan.kernel], bm=plan.bm, bn=plan.bn, epilogue=_lib.GEMM_EPILOGUES[plan.epilogue])


def test_names_follow_the_header():
    from prcv2025reid_amd import _lib
    src = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'include', 'reid_hip.h')).read()
    for prefix, names in (('REID_GEMM_', _lib.GEMM_KERNELS), ('REID_EPI_', _lib.GEMM_EPILOGUES)):
        found = {n.lower(): int(v) for n, v in re.findall(prefix + r'(\w+) = (\d+)', src)}
        assert found == {n: i for i, n in enumerate(names)}


def test_frozen_routes(ops):
    """Every case of CASES and STEP_CASES x cus in {4, 8, 64, 256, 304}: kernel, tile and epilogue are the recorded ones."""
    from prcv2025reid_amd import _lib
    rows = golden_rows(_lib.flavor())
    assert {(r['case'], r['cus']) for r in rows} == {(c['name'], cus) for c in CASES + STEP_CASES for cus in (4, 8, 64, 256, 304)}
    wrong = []
    for r in rows:
        c = BY_NAME[r['case']]
        assert r['tile'] == c.get('tile', 0)
        got = route(case_plan(ops, c, r['cus']))
        want = {k: r[k] for k in ('kernel', 'bm', 'bn', 'epilogue')}
        if got != want:
            wrong.append((r['case'], r['cus'], got, want))
    assert not wrong, wrong


def test_training_step_routes(ops):
    """The policy for the seven GEMMs of a vision block at the training step's size (256 x 197 rows in four row groups) on 256 CUs,
    spelled out -- and equal to the recorded rows."""
    from prcv2025reid_amd import _lib
    half = 'plain16h' if _lib.flavor() == 'bf16' else 'plain16'       # IEEE half is the f16 flavor's own 16-bit format
    expected = {
        'step_qkv': ('pps', 256, 'plain16'),                  # 224 rows would need a ninth round of 256 tiles (2052 against 1800)
        'step_out_proj_f16': ('pps', 224, half),              # 228 x 3 tiles: three rounds either way, each 7/8 as long
        'step_fc1_gelu_dsave': ('pp', 256, 'gelu2d'),         # the GELU epilogues are slower persistent
        'step_fc2_f16': ('pps', 224, half),
        'step_fc2_bwd_mul_aux': ('pp', 256, 'mulaux'),        # aux tile staged by the K loop's last steps (256 rows only)
        'step_fc1_bwd_plain': ('pps', 224, 'plain16'),
        'step_qkv_bwd_plain': ('pps', 224, 'plain16'),
    }
    assert set(expected) == {c['name'] for c in STEP_CASES}
    recorded = {r['case']: (r['kernel'], r['bm'], r['epilogue']) for r in golden_rows(_lib.flavor()) if r['cus'] == 256}
    for c in STEP_CASES:
        assert c['groups'] == [64, 64, 64, 64] and c['M'] == 256 * S
        plan = case_plan(ops, c, 256)
        got = route(plan)
        assert (got['kernel'], got['bm'], got['epilogue']) == expected[c['name']] == recorded[c['name']], c['name']
        assert got['bn'] == 256
        assert plan.grid == (256 if got['kernel'] == 'pps' else plan.tiles_m * plan.tiles_n)


def sweep_args(M, N, K, grouped, out32):
    """Plain call (16-bit or fp32 + residual output) with made-up non-null pointers: nothing dereferences them."""
    from prcv2025reid_amd._lib import GemmArgs, F32
    a = GemmArgs()
    a.A, a.B, a.C = 4096, 8192, 12288
    a.M, a.N, a.K = M, N, K
    a.lda = a.ldb = K
    a.ldc = N
    if out32:
        a.c_dtype = a.r_dtype = F32
        a.R, a.ldr = 16384, N
    if grouped:
        ends = sorted({max(1, M // 3), max(1, (2 * M) // 3), M})
        a.n_row_groups = len(ends)
        for i, e in enumerate(ends):
            a.row_group_end[i], a.row_group_b[i] = e, i
        a.b_group_stride = N * K
    return a


def group_rows(a):
    if a.n_row_groups == 0:
        return [a.M]
    ends = [0] + list(a.row_group_end[:a.n_row_groups])
    return [hi - lo for lo, hi in zip(ends, ends[1:])]


def test_plan_invariants(ops):
    from prcv2025reid_amd._lib import GemmPlan, lib
    h = lib()
    seen = set()
    for M, N, K, grouped, out32 in itertools.product((1, 63, 197, 1000, 12600, 50432, 65601), (32, 64, 96, 128, 640, 768, 772, 2304, 3072),
                                                     (64, 768, 3072), (False, True), (False, True)):
        a = sweep_args(M, N, K, grouped, out32)
        rows = group_rows(a)
        for cus, tile in itertools.product((1, 7, 8, 256), (0, 3, 12, 14)):
            p = GemmPlan()
            assert h.reid_mer_gemm_plan(ctypes.byref(a), cus, tile, ctypes.byref(p)) == 0, h.reid_last_error()
            what = (M, N, K, grouped, out32, cus, tile, route(p))
            tiles = p.tiles_m * p.tiles_n
            assert p.tiles_m == sum((r + p.bm - 1) // p.bm for r in rows), what      # tiles_m * bm covers M group by group
            assert p.tiles_n * p.bn >= N > (p.tiles_n - 1) * p.bn, what
            assert 1 <= p.grid <= tiles, what
            assert p.bm != 224 or p.epilogue != GENERIC, what
            assert p.epilogue in (GENERIC, PLAIN16, RES32), what
            if p.kernel == PPS:
                assert p.epilogue in (PLAIN16, PLAIN16H, RES32) and a.K2 == 0 and K >= 192, what
                assert p.grid % 8 == 0 or p.grid == tiles, what
            else:
                assert p.grid == tiles, what
            if p.kernel != TILED:
                assert N % 256 == 0 and p.bn == 256 and p.bm in (224, 256), what
            else:
                assert (p.bm, p.bn) in ((64, 32), (256, 32), (64, 64), (256, 64), (128, 32), (128, 128)), what
            seen.add((p.kernel, p.bm, p.bn, p.epilogue))
    assert len(seen) >= 12, seen                                                     # the sweep is not stuck on one route


REFUSED = [
    (dict(K=96), b'multiple of 64'),
    (dict(N=130), b'multiple of 4'),
    (dict(M=0), b'empty problem'),
    (dict(A=None), b'non-null'),
    (dict(lda=760), b'lda/ldb'),
    (dict(ldc=100), b'ldc='),
    (dict(M=3000000), b'beyond 4 GiB'),
    (dict(A2=64, B2=0, K2=32), b'K2='),
    (dict(A2=64, B2=128, K2=32, lda2=32, ldb2=32, k2_group_n=64), b'lda2='),
    (dict(act=9), b'act='),
    (dict(act=7), b'needs aux'),
    (dict(act=8), b'needs C2'),
    (dict(R=64, ldr=8), b'ldr'),
    (dict(C2=64, ldc2=8), b'ldc2'),
    (dict(mask_r=8), b'modality mask'),
    (dict(c_group=196, c_group_stride=100), b'c_group_stride'),
    (dict(row_scale=64), b'row_scale needs rows_per_img'),
    (dict(n_row_groups=9), b'n_row_groups='),
    (dict(n_row_groups=1, b_group_stride=768 * 768), b'strictly increasing'),
    (dict(c_dtype=2, R=64, ldr=768, r_dtype=1), b'REID_F16'),          # half output with a residual (bf16 flavor; the f16 flavor: below)
    (dict(C2=64, ldc2=768, c2_dtype=2), b'REID_F16 is supported for C only'),
]


def test_refused_arguments_are_refused_by_the_plan(ops):
    """Every refused argument set: REID_ERR_ARG and reid_mer_gemm's own message, from the plan as from the launcher (which stops at the
    same check, before any launch: no GPU needed)."""
    from prcv2025reid_amd._lib import GemmPlan, flavor, lib
    h = lib()
    p = GemmPlan()
    assert h.reid_mer_gemm_plan(None, 256, 0, ctypes.byref(p)) == -1 and b'null args' in h.reid_last_error()
    ok = sweep_args(1000, 768, 768, False, False)
    assert h.reid_mer_gemm_plan(ctypes.byref(ok), 256, 0, None) == -1 and b'null plan' in h.reid_last_error()
    assert h.reid_mer_gemm_plan(ctypes.byref(ok), 256, 0, ctypes.byref(p)) == 0
    for change, message in REFUSED:
        a = sweep_args(1000, 768, 768, False, False)
        for k, v in change.items():
            setattr(a, k, v)
        if flavor() == 'f16' and message.startswith(b'REID_F16'):
            continue                                                   # REID_F16 is that flavor's own format: nothing to refuse
        assert h.reid_mer_gemm_plan(ctypes.byref(a), 256, 0, ctypes.byref(p)) == -1, change
        said = h.reid_last_error()
        assert said.startswith(b'reid_mer_gemm: ') and message in said, (change, said)
        assert h.reid_mer_gemm(ctypes.byref(a), None) == -1 and h.reid_last_error() == said, change
    if flavor() == 'bf16':                                             # a half output under a forced tile
        a = sweep_args(1000, 768, 768, False, False)
        a.c_dtype = 2
        assert h.reid_mer_gemm_plan(ctypes.byref(a), 256, 0, ctypes.byref(p)) == 0 and p.epilogue == PLAIN16H
        assert h.reid_mer_gemm_plan(ctypes.byref(a), 256, 12, ctypes.byref(p)) == -1 and b'REID_F16 output' in h.reid_last_error()


def test_plan_takes_cpu_tensors(ops):
    from prcv2025reid_amd import _lib
    t16 = _lib.t16()
    plan = ops.gemm_plan(torch.empty(1000, 768, dtype=t16), torch.empty(768, 768, dtype=t16), torch.empty(1000, 768, dtype=t16), cus=256)
    assert route(plan) == dict(kernel='tiled', bm=128, bn=128, epilogue='plain16')
    with pytest.raises(_lib.ReidHipError, match='multiple of 64'):
        ops.gemm_plan(torch.empty(1000, 96, dtype=t16), torch.empty(768, 96, dtype=t16), torch.empty(1000, 768, dtype=t16), cus=256)
