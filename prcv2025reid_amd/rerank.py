"""k-reciprocal re-ranking (Zhong et al., CVPR 2017) of one evaluation on the HIP path; definition: DESIGN.md "k-reciprocal
re-ranking".  The reference has no re-ranking; this is the post-processing step a submission is usually written with.

All queries and the gallery are pooled, N = Nq + Ng <= 65 536 rows, dense from start to finish:
  1. pooled kNN lists           GalleryIndex(X).topk(X, k1 + 1): exact fp32 order, the package's tie rule
  2. weights V [N, N]           reid_rerank_weights: reciprocal sets, their expansion, exp(-d) normalised over R*(i)
  3. local expansion V2 [N, N]  reid_rerank_expand: mean of V over the first k2 neighbours
  4. s* rows per query chunk    reid_rerank_jaccard on V2 and the evaluator's fp32-grade cosine rows
The result depends on the whole query set (queries are neighbours of each other), so all queries of one evaluation go into one
call.  V and V2 take N^2 * 4 bytes each (17 GB at the limit); V is released once V2 exists.  Nothing falls back to the CPU.
"""
from dataclasses import dataclass
from typing import Iterator, Optional, Tuple

import torch

from . import _lib, ops
from .evaluate import split_gallery, split_scores
from .retrieval import GalleryIndex, l2_normalize

MAX_ROWS = 65536          # pooled rows: V and V2 are dense [N, N] fp32
MAX_K1 = 64               # reid_rerank_weights holds a kNN list of k1 + 1 entries per wave


@dataclass(frozen=True)
class RerankParams:
    k1: int = 20
    k2: int = 6
    lambda_value: float = 0.3


def check_shapes(Nq: int, Ng: int, params: RerankParams):
    """Refuses, before anything touches the device, what the kernels would refuse or what would not fit."""
    N = Nq + Ng
    if Nq < 1 or Ng < 1:
        raise _lib.ReidHipError(f're-ranking needs at least one query and one gallery row (Nq={Nq}, Ng={Ng})')
    if N > MAX_ROWS:
        raise _lib.ReidHipError(f're-ranking pools queries and gallery into dense [N, N] fp32 matrices: N = {Nq} + {Ng} = {N} exceeds '
                                f'{MAX_ROWS} rows (the sparse large-gallery form is not built)')
    if not 1 <= params.k1 <= MAX_K1:
        raise _lib.ReidHipError(f're-ranking: k1={params.k1} outside 1..{MAX_K1}')
    if params.k1 + 1 > N:
        raise _lib.ReidHipError(f're-ranking: k1 + 1 = {params.k1 + 1} neighbours asked of N = {N} pooled rows')
    if not 1 <= params.k2 <= params.k1 + 1:
        raise _lib.ReidHipError(f're-ranking: k2={params.k2} outside 1..k1 + 1 = {params.k1 + 1}')
    if not 0.0 <= params.lambda_value <= 1.0:
        raise _lib.ReidHipError(f're-ranking: lambda={params.lambda_value} outside [0, 1]')


class Reranker:
    """Steps 1-3 for one (query set, gallery) pair, built once; ``rows(a, b)`` then returns the s* rows of queries a..b-1."""

    def __init__(self, Qf: torch.Tensor, Gf: torch.Tensor, params: RerankParams, Gcat: Optional[torch.Tensor] = None):
        """Qf, Gf: L2-normalised fp32 device rows; Gcat: the gallery's split operand (``split_gallery(Gf)``) if the caller has it."""
        check_shapes(Qf.shape[0], Gf.shape[0], params)
        if not (Qf.is_cuda and Gf.is_cuda):
            raise _lib.ReidHipError('re-ranking needs device tensors (there is no CPU path)')
        self.params = params
        self.Nq, self.Ng = Qf.shape[0], Gf.shape[0]
        self.N = self.Nq + self.Ng
        self.X = torch.cat([Qf, Gf], 0).contiguous()
        self.Gcat = split_gallery(Gf) if Gcat is None else Gcat
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


def rerank_scores(q_feats: torch.Tensor, g_feats: torch.Tensor, params: RerankParams = RerankParams(), normalized: bool = False,
                  chunk: int = 1024) -> Iterator[Tuple[int, torch.Tensor]]:
    """Yields ``(a, S)`` chunk by chunk: S [<= chunk, ld >= Ng] holds the re-ranked similarities s* of queries a, a + 1, ...
    against the gallery (re-ranked distance = 1 - s*; rank by s* descending, gallery index ascending on ties).  Arguments are
    checked and steps 1-3 run at the call, the Jaccard step as the chunks are drawn."""
    check_shapes(q_feats.shape[0], g_feats.shape[0], params)
    if not (q_feats.is_cuda and g_feats.is_cuda):
        raise _lib.ReidHipError('re-ranking needs device tensors (there is no CPU path)')
    Qf, Gf = q_feats.contiguous().float(), g_feats.contiguous().float()
    if not normalized:
        Qf, Gf = l2_normalize(Qf), l2_normalize(Gf)
    rr = Reranker(Qf, Gf, params)

    def chunks():
        for a in range(0, rr.Nq, chunk):
            yield a, rr.rows(a, min(rr.Nq, a + chunk))
    return chunks()
