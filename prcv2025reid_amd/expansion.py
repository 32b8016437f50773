"""Query expansion and database-side augmentation on the HIP path; definition: DESIGN.md "Query expansion and database-side
augmentation" and reid_expand_rows in include/reid_hip.h.  The reference has neither; with re-ranking this is the usual
post-processing of a ReID evaluation.

Every feature is replaced by the L2-normalised sum of itself and its k nearest gallery rows, each weighted by cosine ** alpha
(alpha = 0: plain average query expansion, Chum et al. ICCV 2007; alpha > 0: alpha-QE, Radenovic et al. TPAMI 2018).
  * ``expand_queries``   the lists are the queries' gallery top-k (``GalleryIndex.topk``): query -> gallery cosines;
  * ``augment_gallery``  database-side augmentation (Arandjelovic & Zisserman 2012, Gordo et al. 2017): the lists are the
                         gallery's own top-(k + 1), the row itself dropped by index: gallery <-> gallery cosines only;
  * ``ProtocolEvaluator(..., augment=)`` and its ``expand=`` arguments (evaluate.py) do both inside an evaluation, the query lists
    under the evaluator's same-image exclusion.
One kernel does the gather, the weights, the sum and the normalisation (``ops.expand_rows``); nothing falls back to the CPU.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, ops
from .retrieval import GalleryIndex, l2_normalize


@dataclass(frozen=True)
class ExpansionParams:
    k: int = 10           # neighbours averaged in (the row itself comes on top)
    alpha: int = 3        # weight = max(cosine, 0) ** alpha; 0 = unweighted (AQE)

    def __post_init__(self):
        if not (isinstance(self.k, int) and isinstance(self.alpha, int)):
            raise _lib.ReidHipError(f'expansion: k={self.k!r} and alpha={self.alpha!r} must be integers')
        if not 1 <= self.k <= ops.EXPAND_MAX_LIST:
            raise _lib.ReidHipError(f'expansion: k={self.k} outside 1..{ops.EXPAND_MAX_LIST} (the longest list reid_expand_rows walks)')
        if not 0 <= self.alpha <= ops.EXPAND_MAX_ALPHA:
            raise _lib.ReidHipError(f'expansion: alpha={self.alpha} outside 0..{ops.EXPAND_MAX_ALPHA}')


def _device_rows(t: torch.Tensor, what: str, normalized: bool) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.ReidHipError(f'{what} needs device tensors (there is no CPU path)')
    t = t.contiguous().float()
    return t if normalized else l2_normalize(t)


def expand_queries(q_feats: torch.Tensor, index: GalleryIndex, params: ExpansionParams = ExpansionParams(), normalized: bool = False,
                   query_img_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """L2-normalised [Nq, D]: every query plus its first ``params.k`` rows of ``index`` (``index.topk``, which drops gallery rows of
    the query's own image id when both id vectors exist), weighted by cosine ** alpha."""
    Qf = _device_rows(q_feats, 'expand_queries', normalized)
    kl = min(params.k, index.Gf.shape[0])                      # (a gallery of fewer than k rows: all of them)
    nbr, score = index.topk(Qf, k=kl, normalized=True, query_img_ids=query_img_ids)
    return ops.expand_rows(Qf, index.Gf, nbr, score, kl, params.alpha)


def augment_gallery(gallery: torch.Tensor, params: ExpansionParams = ExpansionParams(), normalized: bool = False,
                    chunk: int = 16384) -> torch.Tensor:
    """L2-normalised [Ng, D]: every gallery row plus its ``params.k`` nearest OTHER gallery rows, weighted by cosine ** alpha.  Lists and
    neighbour rows come from the gallery as given, so the result does not depend on ``chunk`` (rows whose lists are drawn at once)."""
    if chunk < 1:
        raise ValueError(f'augment_gallery: chunk={chunk}')
    if params.k + 1 > ops.EXPAND_MAX_LIST:
        raise _lib.ReidHipError(f'augment_gallery: k={params.k} needs lists of k + 1 entries (the row itself is one), more than '
                                f'{ops.EXPAND_MAX_LIST}')
    Gf = _device_rows(gallery, 'augment_gallery', normalized)
    index = GalleryIndex(Gf, normalized=True)
    out = torch.empty_like(Gf)
    kl = min(params.k + 1, Gf.shape[0])                        # k + 1: the row itself is one of them; a smaller gallery: all of it
    for a in range(0, Gf.shape[0], chunk):
        b = min(Gf.shape[0], a + chunk)
        nbr, score = index.topk(Gf[a:b], k=kl, normalized=True)
        ops.expand_rows(Gf[a:b], Gf, nbr, score, min(params.k, kl), params.alpha, self_base=a, out=out[a:b])
    return out
