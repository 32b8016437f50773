"""k-reciprocal re-ranking (Zhong et al., CVPR 2017) of one evaluation on the HIP path; definition: DESIGN.md "k-reciprocal
re-ranking".  The reference has no re-ranking; this is the post-processing step a submission is usually written with.

All queries and the gallery are pooled.  The default form: N = Nq + Ng <= 65 536 rows, dense from start to finish:
  1. pooled kNN lists           GalleryIndex(X).topk(X, k1 + 1): exact fp32 order, the package's tie rule
  2. weights V [N, N]           reid_rerank_weights: reciprocal sets, their expansion, exp(-d) normalised over R*(i)
  3. local expansion V2 [N, N]  reid_rerank_expand: mean of V over the first k2 neighbours
  4. s* rows per query chunk    reid_rerank_jaccard on V2 and the evaluator's fp32-grade cosine rows
The result depends on the whole query set (queries are neighbours of each other), so all queries of one evaluation go into one
call.  V and V2 take N^2 * 4 bytes each (17 GB at the limit); V is released once V2 exists.  Nothing falls back to the CPU.

``RerankParams(sparse=True)`` asks for the sparse form (``SparseReranker``): the same definition and the same values, the
non-zeros only (layout: include/reid_hip.h), no limit on N other than int32 row indices:
  2. weights as padded rows     reid_rerank_weights_sparse: (column, value) lists of at most W = (k1 + 1)(kh + 2) entries, and vcnt
  3. V2 as CSR                  reid_rerank_expand_count, a cumsum, reid_rerank_expand_sparse; then the gallery rows transposed
                                to CSC with torch ops (bincount, cumsum, one stable sort): a cold step
  4. s* rows per query chunk    reid_rerank_jaccard_sparse: one workgroup per s* row, m accumulated in the row itself

The pooled-only form (``Reranker.for_pool(X, params)``, ``SparseReranker.for_pool``): the pool is X alone (Nq = 0, Ng = N), every row is
both query and gallery column, ``rows(a, b)`` = s* of pool rows a..b-1 against all N columns.  Same steps, same kernels; it is what
``cluster.jaccard_dbscan`` draws its Jaccard rows from.

Ranked lists of either form (``topk``, ``rerank_topk``): reid_rows_topk on the s* rows, an exact top-k select in the order of a stable
descending sort, without the sort.
"""
from dataclasses import dataclass
from typing import Iterator, Optional, Tuple

import torch

from . import _lib, ops
from .evaluate import split_gallery, split_scores
from .retrieval import GalleryIndex, l2_normalize

MAX_ROWS = 65536          # pooled rows: V and V2 are dense [N, N] fp32
MAX_K1 = 64               # reid_rerank_weights holds a kNN list of k1 + 1 entries per wave
SPARSE_MERGE_MAX = 8192   # REID_RERANK_MERGE_MAX: entries of one row's merge k2 (k1 + 1)(kh + 2) that reid_rerank_expand_sparse holds in LDS


@dataclass(frozen=True)
class RerankParams:
    k1: int = 20
    k2: int = 6
    lambda_value: float = 0.3
    sparse: bool = False      # the sparse form: no row limit (SparseReranker)


def list_width(k1: int) -> int:
    """W = (k1 + 1)(kh + 2) >= |R*(i)|, kh = round-half-to-even(k1 / 2): the width of a padded row of V."""
    kh = k1 // 2 + ((k1 // 2) & 1 if k1 & 1 else 0)
    return (k1 + 1) * (kh + 2)


def check_shapes(Nq: int, Ng: int, params: RerankParams):
    """Refuses, before anything touches the device, what the kernels would refuse or what would not fit."""
    if Nq < 1 or Ng < 1:
        raise _lib.ReidHipError(f're-ranking needs at least one query and one gallery row (Nq={Nq}, Ng={Ng})')
    _check_pooled(Nq + Ng, f'{Nq} + {Ng} = {Nq + Ng}', params)


def check_pool(N: int, params: RerankParams):
    """``check_shapes`` for the pooled-only form (``for_pool``): one set of N rows, every row both query and gallery column."""
    if N < 1:
        raise _lib.ReidHipError(f're-ranking needs at least one pooled row (N={N})')
    _check_pooled(N, f'{N}', params)


def _check_pooled(N: int, shown: str, params: RerankParams):
    if N > MAX_ROWS and not params.sparse:
        raise _lib.ReidHipError(f're-ranking pools queries and gallery into dense [N, N] fp32 matrices: N = {shown} exceeds '
                                f'{MAX_ROWS} rows (RerankParams(sparse=True) has no row limit)')
    if N > 2 ** 31 - 1:
        raise _lib.ReidHipError(f're-ranking: N = {shown} pooled rows do not fit int32 row indices')
    if not 1 <= params.k1 <= MAX_K1:
        raise _lib.ReidHipError(f're-ranking: k1={params.k1} outside 1..{MAX_K1}')
    if params.k1 + 1 > N:
        raise _lib.ReidHipError(f're-ranking: k1 + 1 = {params.k1 + 1} neighbours asked of N = {N} pooled rows')
    if not 1 <= params.k2 <= params.k1 + 1:
        raise _lib.ReidHipError(f're-ranking: k2={params.k2} outside 1..k1 + 1 = {params.k1 + 1}')
    if not 0.0 <= params.lambda_value <= 1.0:
        raise _lib.ReidHipError(f're-ranking: lambda={params.lambda_value} outside [0, 1]')
    if params.sparse and params.k2 * list_width(params.k1) > SPARSE_MERGE_MAX:
        raise _lib.ReidHipError(f're-ranking, sparse form: k1={params.k1} k2={params.k2} merge k2 (k1 + 1)(kh + 2) = '
                                f'{params.k2 * list_width(params.k1)} entries per row, more than SPARSE_MERGE_MAX = {SPARSE_MERGE_MAX}')


class _RankedRows:
    """What both forms share: the two constructors in front of ``_build`` (steps 1-3), and the lists once ``rows(a, b)`` exists."""

    def __init__(self, Qf: torch.Tensor, Gf: torch.Tensor, params: RerankParams, Gcat: Optional[torch.Tensor] = None):
        """Qf, Gf: L2-normalised fp32 device rows; Gcat: the gallery's split operand (``split_gallery(Gf)``) if the caller has it."""
        check_shapes(Qf.shape[0], Gf.shape[0], params)
        if not (Qf.is_cuda and Gf.is_cuda):
            raise _lib.ReidHipError('re-ranking needs device tensors (there is no CPU path)')
        self._build(torch.cat([Qf, Gf], 0).contiguous(), Qf.shape[0], params, split_gallery(Gf) if Gcat is None else Gcat)

    @classmethod
    def for_pool(cls, X: torch.Tensor, params: RerankParams):
        """The pooled-only form: the pool is X alone (L2-normalised fp32 device rows; Nq = 0, Ng = N), every row both query and gallery
        column; ``rows(a, b)`` returns the s* rows of pool rows a..b-1 against all N columns."""
        check_pool(X.shape[0], params)
        if not X.is_cuda:
            raise _lib.ReidHipError('re-ranking needs device tensors (there is no CPU path)')
        self = cls.__new__(cls)
        X = X.contiguous()
        self._build(X, 0, params, split_gallery(X))
        return self

    def topk(self, a: int, b: int, k: int, g_img: Optional[torch.Tensor] = None, q_excl: Optional[torch.Tensor] = None):
        """(idx i32 [b - a, k], s* f32 [b - a, k]): the first k gallery rows of queries a..b-1 by s* descending, gallery index ascending
        on ties (``ops.rows_topk`` on ``rows(a, b)``); ``g_img`` [Ng] and ``q_excl`` [b - a, 4] drop images as ``ops.rank_metrics`` does."""
        return ops.rows_topk(self.rows(a, b), self.Ng, k, g_img, q_excl)


class Reranker(_RankedRows):
    """Steps 1-3 for one (query set, gallery) pair, built once; ``rows(a, b)`` then returns the s* rows of queries a..b-1."""

    def _build(self, X: torch.Tensor, Nq: int, params: RerankParams, Gcat: torch.Tensor):
        self.params = params
        self.Nq, self.Ng = Nq, X.shape[0] - Nq
        self.N = X.shape[0]
        self.X, self.Gcat = X, Gcat
        self.nbr, _ = GalleryIndex(self.X, normalized=True).topk(self.X, k=params.k1 + 1, normalized=True)
        ld = (self.N + 3) // 4 * 4
        V = torch.empty(self.N, ld, device=self.X.device)
        ops.rerank_weights(self.nbr, self.X, V, params.k1)
        self.V2 = torch.empty(self.N, ld, device=self.X.device)
        ops.rerank_expand(V, self.nbr, self.V2, params.k1, params.k2)

    def rows(self, a: int, b: int) -> torch.Tensor:
        """s* [b - a, ld >= Ng] of queries a..b-1 (ld a multiple of 4; columns >= Ng are padding, not written)."""
        cos = split_scores(self.X[a:b], self.Gcat)
        out = torch.empty_like(cos)
        ops.rerank_jaccard(self.V2[a:b], self.V2[self.Nq:], cos, out, self.Ng, self.N, self.params.lambda_value)
        return out


class SparseReranker(_RankedRows):
    """``Reranker`` on the sparse form: the same ``rows(a, b)``, V2 as CSR (``rowptr``, ``cols``, ``vals``) and its gallery rows as
    CSC (``colptr``, ``grows``, ``cvals``).  Building it synchronises once, to size the arrays of non-zeros."""

    def _build(self, X: torch.Tensor, Nq: int, params: RerankParams, Gcat: torch.Tensor):
        self.params = params
        self.Nq, self.Ng = Nq, X.shape[0] - Nq
        self.N = N = X.shape[0]
        dev = X.device
        self.X, self.Gcat = X, Gcat
        index = GalleryIndex(self.X, normalized=True)
        index.exact_scratch_bytes = 2 << 30       # the pooled call is drawn in query chunks: no [N, N] scratch is kept
        self.nbr, _ = index.topk(self.X, k=params.k1 + 1, normalized=True)
        del index
        W = list_width(params.k1)
        vcols = torch.empty(N, W, dtype=torch.int32, device=dev)
        vvals = torch.empty(N, W, device=dev)
        vcnt = torch.empty(N, dtype=torch.int32, device=dev)
        ops.rerank_weights_sparse(self.nbr, self.X, vcols, vvals, vcnt, params.k1)
        cnt = torch.empty(N, dtype=torch.int32, device=dev)
        ops.rerank_expand_count(vcols, vvals, vcnt, self.nbr, cnt, params.k1, params.k2)
        self.rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, dtype=torch.int64, out=self.rowptr[1:])
        nnz, first = (int(v) for v in self.rowptr[[N, self.Nq]].tolist())       # the one synchronisation
        self.cols = torch.empty(nnz, dtype=torch.int32, device=dev)
        self.vals = torch.empty(nnz, device=dev)
        ops.rerank_expand_sparse(vcols, vvals, vcnt, self.nbr, self.rowptr, self.cols, self.vals, params.k1, params.k2)
        del vcols, vvals, vcnt
        self.colptr, self.grows, self.cvals = csc_of_rows(self.cols[first:], self.vals[first:], cnt[self.Nq:], N)

    def rows(self, a: int, b: int) -> torch.Tensor:
        """s* [b - a, ld >= Ng] of queries a..b-1 (ld a multiple of 4; columns >= Ng are padding, not written)."""
        cos = split_scores(self.X[a:b], self.Gcat)
        out = torch.empty_like(cos)
        ops.rerank_jaccard_sparse(self.rowptr[a:b + 1], self.cols, self.vals, self.colptr, self.grows, self.cvals, cos, out, self.Ng,
                                  self.params.lambda_value)
        return out


def csc_of_rows(cols: torch.Tensor, vals: torch.Tensor, cnt: torch.Tensor, N: int):
    """(colptr i64 [N + 1], rows i32, cvals f32): the transpose of CSR rows given by their lengths ``cnt`` and their concatenated
    ``cols`` (ascending inside a row, < N) and ``vals``; rows come out ascending inside a column (a stable sort)."""
    row_of = torch.repeat_interleave(torch.arange(cnt.shape[0], dtype=torch.int32, device=cols.device), cnt.long(), output_size=cols.shape[0])
    colptr = torch.zeros(N + 1, dtype=torch.int64, device=cols.device)
    torch.cumsum(torch.bincount(cols, minlength=N), 0, out=colptr[1:])
    order = torch.sort(cols, stable=True)[1]
    return colptr, row_of[order].contiguous(), vals[order].contiguous()


def _pooled(q_feats: torch.Tensor, g_feats: torch.Tensor, params: RerankParams, normalized: bool):
    """The checks of the public calls, then steps 1-3."""
    check_shapes(q_feats.shape[0], g_feats.shape[0], params)
    if not (q_feats.is_cuda and g_feats.is_cuda):
        raise _lib.ReidHipError('re-ranking needs device tensors (there is no CPU path)')
    Qf, Gf = q_feats.contiguous().float(), g_feats.contiguous().float()
    if not normalized:
        Qf, Gf = l2_normalize(Qf), l2_normalize(Gf)
    return (SparseReranker if params.sparse else Reranker)(Qf, Gf, params)


def rerank_scores(q_feats: torch.Tensor, g_feats: torch.Tensor, params: RerankParams = RerankParams(), normalized: bool = False,
                  chunk: int = 1024) -> Iterator[Tuple[int, torch.Tensor]]:
    """Yields ``(a, S)`` chunk by chunk: S [<= chunk, ld >= Ng] holds the re-ranked similarities s* of queries a, a + 1, ...
    against the gallery (re-ranked distance = 1 - s*; rank by s* descending, gallery index ascending on ties).  Arguments are
    checked and steps 1-3 run at the call, the Jaccard step as the chunks are drawn."""
    rr = _pooled(q_feats, g_feats, params, normalized)

    def chunks():
        for a in range(0, rr.Nq, chunk):
            yield a, rr.rows(a, min(rr.Nq, a + chunk))
    return chunks()


def rerank_topk(q_feats: torch.Tensor, g_feats: torch.Tensor, params: RerankParams = RerankParams(), k: int = 100,
                normalized: bool = False, chunk: int = 1024) -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx i32 [Nq, k], s* f32 [Nq, k]): every query's first k gallery rows by the re-ranked similarity, the order of a stable
    descending sort of the rows ``rerank_scores`` yields for the same call (positions past Ng hold -1 / -inf).  1 <= k <= 1024."""
    if not 1 <= k <= ops.ROWS_TOPK_MAX_K:
        raise _lib.ReidHipError(f're-ranking: k={k} outside 1..{ops.ROWS_TOPK_MAX_K} (the limit of ops.rows_topk)')
    rr = _pooled(q_feats, g_feats, params, normalized)
    parts = [rr.topk(a, min(rr.Nq, a + chunk), k) for a in range(0, rr.Nq, chunk)]
    return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)
