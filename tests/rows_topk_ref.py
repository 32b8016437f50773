"""numpy restatement of reid_rows_topk's contract (include/reid_hip.h): key, order, exclusion, -1 / -inf fill.  Shared by
test_rows_topk_cpu.py (which checks it against torch's stable descending sort) and test_rows_topk_gpu.py."""
import numpy as np


def order_key(x):
    """u32 key of float32 ``x``: the order-preserving image of x + 0.0f, every NaN -> 0xFFFFFFFF."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0                                   # -0 -> +0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(x)] = np.uint32(0xFFFFFFFF)
    return key


def excluded(g_img, q_excl_row):
    """Bool [n]: rank_metrics_kernel's ``excluded`` for one query."""
    g = np.asarray(g_img)
    return (g >= 0) & np.isin(g, np.asarray(q_excl_row))


def rows_topk_ref(scores, n, k, g_img=None, q_excl=None):
    """(idx i32 [nq, k], score f32 [nq, k]) of float32 ``scores`` [nq, ld >= n]."""
    scores = np.asarray(scores, dtype=np.float32)
    nq = scores.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), -np.inf, np.float32)
    cols = np.arange(n)
    for q in range(nq):
        row = scores[q, :n]
        key = order_key(row)
        order = np.lexsort((cols, -key.astype(np.int64)))             # key descending, then column ascending
        if g_img is not None and q_excl is not None:
            order = order[~excluded(np.asarray(g_img)[:n], q_excl[q])[order]]
        m = min(k, len(order))
        idx[q, :m] = order[:m]
        out[q, :m] = row[order[:m]]
    return idx, out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
