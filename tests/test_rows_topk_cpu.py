"""reid_rows_topk without a GPU: the numpy restatement of its order (rows_topk_ref.py) against torch's stable descending sort, the
host-side refusals of the bound library, and the device-only stance of the Python layers."""
import ctypes

import numpy as np
import pytest
import torch

import rows_topk_ref as T


@pytest.fixture(scope='module')
def libs():
    from prcv2025reid_amd import _lib, build
    build.build(verbose=False)
    return {f: _lib.bind(ctypes.CDLL(p)) for f, p in _lib.LIB_PATHS.items()}


def special_rows(rng, nq, n):
    """Rows of few distinct values (long tie runs) with -0, +0, +-inf, NaNs of both signs, denormals and negatives sprinkled in."""
    S = (rng.integers(-6, 7, (nq, n)) * 0.25).astype(np.float32)
    normal = rng.random((nq, n)) < 0.3
    S[normal] = rng.standard_normal(int(normal.sum())).astype(np.float32)
    specials = np.array([0x80000000, 0x00000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001, 0x00000001, 0x80000001,
                         0x007fffff, 0x807fffff, 0x00800000, 0x80800000], np.uint32).view(np.float32)
    where = rng.random((nq, n)) < 0.25
    S[where] = specials[rng.integers(0, len(specials), int(where.sum()))]
    return S


def test_restatement_is_torchs_stable_descending_sort():
    rng = np.random.default_rng(11)
    S = special_rows(rng, 200, 301)
    S[0] = 0.0                                                        # one all-equal row
    S[1] = np.where(rng.random(301) < 0.5, np.float32(-0.0), np.float32(0.0))   # -0 and +0 only: one tie block
    assert np.isnan(S).any() and (T.bits(S) == 0x80000000).any() and np.isinf(S).any()
    order = torch.sort(torch.from_numpy(S), dim=1, descending=True, stable=True)[1].numpy()
    for k in (1, 7, 301, 320):
        idx, score = T.rows_topk_ref(S, 301, k)
        m = min(k, 301)
        assert np.array_equal(idx[:, :m], order[:, :m])
        assert np.array_equal(T.bits(score[:, :m]), T.bits(np.take_along_axis(S, order[:, :m], 1)))
        assert (idx[:, m:] == -1).all() and (T.bits(score[:, m:]) == 0xff800000).all()


def test_key_order_and_exclusion_of_the_restatement():
    f = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], np.float32)
    key = T.order_key(f)
    assert key[3] == key[4] == 0x80000000 and key[0] == 0x007fffff and key[-1] == 0xffffffff
    assert (np.diff(key[[0, 1, 2, 3, 5, 6, 7, 8]].astype(np.int64)) > 0).all()
    assert T.order_key(np.array([0xffc00001], np.uint32).view(np.float32))[0] == 0xffffffff       # a negative NaN too
    S = np.array([[5, 4, 3, 2, 1]], np.float32)
    g_img = np.array([7, -1, 3, 7, -1], np.int32)
    idx, score = T.rows_topk_ref(S, 5, 4, g_img, np.array([[7, -1, -1, -1]], np.int32))
    assert idx.tolist() == [[1, 2, 4, -1]] and score[0, :3].tolist() == [4, 3, 1] and score[0, 3] == -np.inf   # -1 never matches a hole


def test_bound_library_refuses_bad_arguments_without_a_gpu(libs):
    # fake non-null pointers: every call is refused on the host before anything is read or launched
    P, I, O = 1 << 20, (1 << 20) + 4096, (1 << 20) + 8192
    for h in libs.values():
        def refused(*args):
            assert h.reid_rows_topk(*args) == -1
            return h.reid_last_error()
        assert b'k=0 outside 1..1024' in refused(P, 16, 2, 10, 0, None, None, I, O, None)
        assert b'k=1025 outside 1..1024' in refused(P, 16, 2, 10, 1025, None, None, I, O, None)
        assert b'ld=8' in refused(P, 8, 2, 10, 3, None, None, I, O, None)                       # ld < n
        assert b'ld=14' in refused(P, 14, 2, 10, 3, None, None, I, O, None)                     # ld % 4 != 0
        assert b'16-byte aligned' in refused(P + 4, 16, 2, 10, 3, None, None, I, O, None)
        assert b'null pointer' in refused(P, 16, 2, 10, 3, None, None, None, O, None)
        assert b'null pointer' in refused(P, 16, 2, 10, 3, None, None, I, None, None)
        assert b'null pointer' in refused(None, 16, 2, 10, 3, None, None, I, O, None)
        assert b'nq=0' in refused(P, 16, 0, 10, 3, None, None, I, O, None)
        assert b'n=0' in refused(P, 16, 2, 0, 3, None, None, I, O, None)


def test_python_layers_refuse_cpu_tensors():
    from prcv2025reid_amd import _lib, ops
    from prcv2025reid_amd.evaluate import ProtocolEvaluator
    from prcv2025reid_amd.rerank import RerankParams, rerank_topk
    Q, G = torch.randn(4, 8), torch.randn(30, 8)
    with pytest.raises(_lib.ReidHipError, match='device tensors'):
        rerank_topk(Q, G, RerankParams(8, 3, 0.3), k=10)
    with pytest.raises(_lib.ReidHipError, match=r'k=1025 outside 1\.\.1024'):
        rerank_topk(Q, G, RerankParams(8, 3, 0.3), k=1025)
    with pytest.raises(_lib.ReidHipError, match='device tensors'):
        ProtocolEvaluator.ranked_lists(object.__new__(ProtocolEvaluator), Q, k=10)          # refused before any state is touched
    with pytest.raises(_lib.ReidHipError, match='CUDA'):
        ops.rows_topk(torch.zeros(2, 8), 8, 3)
