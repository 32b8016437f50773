"""Batched MM-protocol evaluator on the HIP path.

Reference: ``rank_and_metrics`` (tools/eval_mm_protocol.py:369-469), ``_reid_map`` (train.py:450-479), the aggregation of
``validate_competition_style`` (train.py:591-602) and ``export_submission_csv`` (tools/eval_mm_protocol.py:595-649).

The reference scores one query at a time, argsorts the whole gallery row and walks it in Python.  Here
  * scores come from the MFMA GEMM of the hot path with SPLIT operands: every fp32 feature is written as a sum of 16-bit
    pieces (2 for the f16 flavor, 3 for bf16) and the significant cross products are laid side by side along K, so one
    ``reid_mer_gemm`` call returns fp32-grade similarities (error <= ~2e-7 for unit vectors, i.e. fp32 rounding level)
    at matrix-core speed;
  * AP / CMC come from ``reid_rank_metrics`` (csrc/metrics.hip): ranks of the positives only, no sort of the gallery.
Nothing here falls back to the CPU; the pure-Python oracle lives in oracle/reid_oracle.py and is used by tests only.
"""
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence

import torch

from . import _lib, ops
from .retrieval import GalleryIndex, l2_normalize

if TYPE_CHECKING:          # (rerank.py imports this module: the classes are only named in annotations here)
    from .expansion import ExpansionParams
    from .rerank import RerankParams

_SCALE = 16.0        # features are scaled into the 16-bit formats' comfortable range before splitting (undone by alpha)


def _split(x: torch.Tensor, pieces: int) -> List[torch.Tensor]:
    out, r = [], x
    for _ in range(pieces):
        h = ops.to_t16(r)
        out.append(h)
        r = r - h.float()
    return out


def _split_operands(Qf: torch.Tensor, Gf: torch.Tensor):
    """[Q pieces laid along K], [G pieces laid along K] such that Qcat @ Gcat.T ~= (Q @ G.T) * SCALE^2 to fp32 accuracy."""
    f16 = _lib.flavor() == 'f16'
    n = 2 if f16 else 3
    pairs = [(0, 0), (0, 1), (1, 0)] if f16 else [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]
    q = _split(Qf * _SCALE, n); g = _split(Gf * _SCALE, n)
    return torch.cat([q[i] for i, _ in pairs], 1).contiguous(), torch.cat([g[j] for _, j in pairs], 1).contiguous()


def split_gallery(Gf: torch.Tensor) -> torch.Tensor:
    """The gallery half of the split operands (rows padded with zeros to a multiple of 4), built once per gallery."""
    pad = (-Gf.shape[0]) % 4
    Gp = torch.cat([Gf, torch.zeros(pad, Gf.shape[1], device=Gf.device)], 0) if pad else Gf
    return _split_operands(Gp[:1], Gp)[1]


def split_scores(Qf: torch.Tensor, Gcat: torch.Tensor) -> torch.Tensor:
    """fp32-grade cosine rows [nq, Gcat rows] of normalised queries against ``split_gallery``'s operand."""
    Qcat = _split_operands(Qf, Qf[:1])[0]
    S = torch.empty(Qf.shape[0], Gcat.shape[0], device=Qf.device)
    ops.gemm(Qcat, Gcat, S, alpha=1.0 / (_SCALE * _SCALE))
    return S


class ProtocolEvaluator:
    """Gallery-side state built once: normalised features, split 16-bit operand, pid CSR, image ids."""

    def __init__(self, gallery_feats: torch.Tensor, gallery_pids: torch.Tensor, gallery_img_ids: Optional[Sequence] = None,
                 normalized: bool = False, augment: Optional['ExpansionParams'] = None):
        """``augment``: an ``ExpansionParams`` replaces the gallery features by ``expansion.augment_gallery`` of them (database-side
        augmentation) before anything else is built from them."""
        g = gallery_feats.contiguous().float()
        if not g.is_cuda:
            raise _lib.ReidHipError('ProtocolEvaluator needs device tensors (there is no CPU path)')
        self.dev = g.device
        self.Gf = g if normalized else l2_normalize(g)
        if augment is not None:
            from .expansion import augment_gallery
            self.Gf = augment_gallery(self.Gf, augment, normalized=True)
        self.Ng, self.D = self.Gf.shape
        self._Gcat = split_gallery(self.Gf)                   # only the gallery half is kept
        pids = gallery_pids.to(self.dev).long()
        self.g_pid = pids.to(torch.int32).contiguous()
        uniq, inv = torch.unique(pids, return_inverse=True)
        order = torch.argsort(inv, stable=True)               # gallery rows grouped by pid, ascending row inside a group
        counts = torch.bincount(inv, minlength=uniq.numel())
        self.csr_off = torch.cat([torch.zeros(1, dtype=torch.long, device=self.dev), counts.cumsum(0)]).to(torch.int32).contiguous()
        self.csr_idx = order.to(torch.int32).contiguous()
        self.max_pos = int(counts.max())
        self._uniq = uniq
        self._img_map: Dict = {}
        self.g_img = None
        if gallery_img_ids is not None:
            ids = [self._img_id(x) for x in gallery_img_ids]
            self.g_img = torch.tensor(ids, dtype=torch.int32, device=self.dev)
        self.index = None

    def _img_id(self, x) -> int:
        if x is None:
            return -1
        return self._img_map.setdefault(x, len(self._img_map))

    # ---------------------------------------------------------------------------------------------------------
    def scores(self, q_feats: torch.Tensor, normalized: bool = False) -> torch.Tensor:
        """fp32-grade cosine similarities [nq, ld >= Ng] (ld a multiple of 4; columns >= Ng are padding)."""
        Qf = q_feats.contiguous().float().to(self.dev)
        if not normalized:
            Qf = l2_normalize(Qf)
        return split_scores(Qf, self._Gcat)

    def _reranker(self, q_feats: torch.Tensor, rerank: 'RerankParams', normalized: bool = False):
        """Pooled state of one re-ranked evaluation (rerank.py): every query of the call at once."""
        from .rerank import Reranker, SparseReranker
        Qf = q_feats.contiguous().float().to(self.dev)
        return (SparseReranker if rerank.sparse else Reranker)(Qf if normalized else l2_normalize(Qf), self.Gf, rerank, self._Gcat)

    def _exclusions(self, q_img_ids: Optional[Sequence], ignore_same_img: bool) -> Optional[torch.Tensor]:
        """i32 [Nq, 4] gallery image ids each query ignores (-1 = unused), or None when nothing is masked."""
        if not (ignore_same_img and q_img_ids is not None and self.g_img is not None):
            return None
        rows = []
        for ids in q_img_ids:
            ids = ids if isinstance(ids, (set, list, tuple)) else [ids]
            known = [self._img_map[x] for x in ids if x is not None and x in self._img_map]   # unknown ids mask nothing
            if len(known) > 4:
                raise ValueError('at most 4 image ids per query (one per modality sample)')
            rows.append(known + [-1] * (4 - len(known)))
        return torch.tensor(rows, dtype=torch.int32, device=self.dev)

    def _expanded(self, q_feats: torch.Tensor, expand: 'ExpansionParams', q_img_ids: Optional[Sequence], ignore_same_img: bool,
                  chunk: int, normalized: bool) -> torch.Tensor:
        """Query expansion inside an evaluation: the L2-normalised queries plus their first ``expand.k`` gallery rows of this
        evaluator's own ``ranked_lists`` -- the ranking ``per_query`` scores, under the same same-image exclusion, so an excluded
        gallery image is never averaged into its own query."""
        if not q_feats.is_cuda:
            raise _lib.ReidHipError('query expansion needs device tensors (there is no CPU path)')
        Qf = q_feats.contiguous().float().to(self.dev)
        if not normalized:
            Qf = l2_normalize(Qf)
        nbr, score = self.ranked_lists(Qf, k=expand.k, q_img_ids=q_img_ids, ignore_same_img=ignore_same_img, chunk=chunk, normalized=True)
        return ops.expand_rows(Qf, self.Gf, nbr, score, expand.k, expand.alpha)

    def per_query(self, q_feats: torch.Tensor, q_pids: torch.Tensor, q_img_ids: Optional[Sequence] = None,
                  ignore_same_img: bool = True, chunk: int = 1024, normalized: bool = False, rerank: Optional['RerankParams'] = None,
                  expand: Optional['ExpansionParams'] = None):
        """(ap f64 [Nq], rank1 i32 [Nq], npos i32 [Nq]) on the device.  ``rerank``: a ``RerankParams`` ranks by the k-reciprocal
        re-ranked similarity s* (rerank.py) instead of the cosine; the same-image exclusion is the same.  ``expand``: an
        ``ExpansionParams`` first replaces the queries by their expansion (``_expanded``); with ``rerank`` as well, the expanded queries
        are what the re-ranker receives."""
        if expand is not None:
            q_feats, normalized = self._expanded(q_feats, expand, q_img_ids, ignore_same_img, chunk, normalized), True
        Nq = q_feats.shape[0]
        qp = q_pids.to(self.dev).long()
        pos = torch.searchsorted(self._uniq, qp).clamp(max=self._uniq.numel() - 1)
        slot = torch.where(self._uniq[pos] == qp, pos, torch.full_like(pos, -1)).to(torch.int32).contiguous()
        qp32 = qp.to(torch.int32).contiguous()
        excl = self._exclusions(q_img_ids, ignore_same_img)
        ap = torch.zeros(Nq, dtype=torch.float64, device=self.dev)
        rank1 = torch.zeros(Nq, dtype=torch.int32, device=self.dev)
        npos = torch.zeros(Nq, dtype=torch.int32, device=self.dev)
        rr = None if rerank is None else self._reranker(q_feats, rerank, normalized)
        for a in range(0, Nq, chunk):
            b = min(Nq, a + chunk)
            S = self.scores(q_feats[a:b], normalized) if rr is None else rr.rows(a, b)
            ops.rank_metrics(S, self.g_pid, self.g_img, qp32[a:b], slot[a:b], None if excl is None else excl[a:b].contiguous(),
                             self.csr_off, self.csr_idx, self.Ng, self.max_pos, ap[a:b], rank1[a:b], npos[a:b])
        return ap, rank1, npos

    def ranked_lists(self, q_feats: torch.Tensor, k: int = 100, q_img_ids: Optional[Sequence] = None, ignore_same_img: bool = True,
                     chunk: int = 1024, normalized: bool = False, rerank: Optional['RerankParams'] = None,
                     expand: Optional['ExpansionParams'] = None):
        """(idx i32 [Nq, k], score f32 [Nq, k]) on the device: every query's first k gallery rows, score descending and gallery index
        ascending on ties, of the very rows ``per_query`` ranks (``scores``, or s* with ``rerank``; of the expanded queries with
        ``expand``) under the same same-image exclusion; positions past the eligible gallery rows hold -1 / -inf.
        1 <= k <= 1024 (``ops.rows_topk``)."""
        if not q_feats.is_cuda:
            raise _lib.ReidHipError('ranked_lists needs device tensors (there is no CPU path)')
        if not 1 <= k <= ops.ROWS_TOPK_MAX_K:
            raise _lib.ReidHipError(f'ranked_lists: k={k} outside 1..{ops.ROWS_TOPK_MAX_K} (the limit of ops.rows_topk)')
        if expand is not None:
            q_feats, normalized = self._expanded(q_feats, expand, q_img_ids, ignore_same_img, chunk, normalized), True
        Nq = q_feats.shape[0]
        excl = self._exclusions(q_img_ids, ignore_same_img)
        idx = torch.empty(Nq, k, dtype=torch.int32, device=self.dev)
        score = torch.empty(Nq, k, dtype=torch.float32, device=self.dev)
        rr = None if rerank is None else self._reranker(q_feats, rerank, normalized)
        for a in range(0, Nq, chunk):
            b = min(Nq, a + chunk)
            S = self.scores(q_feats[a:b], normalized) if rr is None else rr.rows(a, b)
            ops.rows_topk(S, self.Ng, k, self.g_img, None if excl is None else excl[a:b].contiguous(), out=(idx[a:b], score[a:b]))
        return idx, score

    def rank_and_metrics(self, q_feats, q_pids, q_img_ids=None, ignore_same_img: bool = True, chunk: int = 1024,
                         rerank: Optional['RerankParams'] = None, expand: Optional['ExpansionParams'] = None) -> Dict[str, float]:
        """Same dictionary as eval_mm_protocol.py:455-469: queries without an (unmasked) positive are skipped."""
        ap, rank1, npos = self.per_query(q_feats, q_pids, q_img_ids, ignore_same_img, chunk, rerank=rerank, expand=expand)
        if bool((npos < 0).any()):
            raise _lib.ReidHipError('a query has more than 8192 positives in the gallery: not supported by reid_rank_metrics')
        valid = npos > 0
        n = int(valid.sum())
        if n == 0:
            return {'mAP': 0.0, 'R@1': 0.0, 'R@5': 0.0, 'R@10': 0.0, 'num_queries': 0}
        r = rank1[valid]
        return {'mAP': float(ap[valid].mean()), 'R@1': float((r <= 1).double().mean()), 'R@5': float((r <= 5).double().mean()),
                'R@10': float((r <= 10).double().mean()), 'num_queries': n}

    def reid_map(self, q_feats, q_pids):
        """(mAP, top-1) of _reid_map (train.py:450-479): mAP over queries with a positive, top-1 over ALL queries."""
        ap, rank1, npos = self.per_query(q_feats, q_pids, None, False)
        valid = npos > 0
        n = max(1, int(valid.sum()))
        return float(ap[valid].sum() / n), float(((rank1 == 1) & valid).double().sum() / q_feats.shape[0])

    # ---------------------------------------------------------------------------------------------------------
    def export_submission_csv(self, q_feats, query_keys: Sequence[str], gallery_img_names: Sequence, output_path: str,
                              top_k: int = 100, rerank: Optional['RerankParams'] = None, chunk: int = 1024,
                              expand: Optional['ExpansionParams'] = None):
        """eval_mm_protocol.py:595-649: one row per query, the top_k gallery image ids of the unmasked ranking.  ``rerank``: a
        ``RerankParams`` lists by the re-ranked similarity s* in the order of a stable descending sort of the s* rows (``ranked_lists``
        without exclusion; the sort itself only for a top_k outside 1..1024, the list lengths of ``ops.rows_topk``).  ``expand``: an
        ``ExpansionParams`` first replaces the queries by their expansion from ``ranked_lists(q, k=expand.k)``, unmasked like the export
        itself (no query image ids reach this call)."""
        import csv
        if expand is not None:
            q_feats = self._expanded(q_feats.to(self.dev), expand, None, True, chunk, False)
        if rerank is None:
            if self.index is None:
                self.index = GalleryIndex(self.Gf, normalized=True)
            idx, _ = self.index.topk(q_feats.to(self.dev), k=min(top_k, self.Ng))
        elif 1 <= top_k <= ops.ROWS_TOPK_MAX_K:                    # (host features are moved here, as the other branches do)
            idx, _ = self.ranked_lists(q_feats.to(self.dev), k=top_k, chunk=chunk, rerank=rerank)   # -1 past the gallery's end (top_k > Ng)
        else:                                                      # outside ops.rows_topk's list lengths (top_k <= 0 included): the sort
            rr = self._reranker(q_feats, rerank)
            idx = torch.cat([torch.sort(rr.rows(a, min(rr.Nq, a + chunk))[:, :self.Ng], dim=1, descending=True, stable=True)[1][:, :top_k]
                             for a in range(0, rr.Nq, chunk)], 0)
        idx = idx.cpu().tolist()
        with open(output_path, 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(['query_key', 'ranked_gallery_ids'])
            for key, row in zip(query_keys, idx):
                w.writerow([key, ' '.join(str(gallery_img_names[i]) for i in row if i >= 0 and gallery_img_names[i] is not None)])


def competition_metrics(all_metrics: Dict[str, Dict[str, float]]) -> Dict[str, float]:
    """train.py:578-602: mean of the four single-modality mAPs, the four-modality mAP and their average."""
    def _get_map(m):
        if isinstance(m, dict):
            for k in ('mAP', 'map', 'mAP_mean', 'map_mean'):
                if k in m:
                    return float(m[k])
        if isinstance(m, (int, float)):
            return float(m)
        return 0.0
    singles = [_get_map(all_metrics.get(k, {})) for k in ('single/nir', 'single/sk', 'single/cp', 'single/text')]
    map_single = sum(singles) / max(1, len([x for x in singles if x == x]))
    map_quad = _get_map(all_metrics.get('quad/nir+sk+cp+text', {}))
    return {'map_single': map_single, 'map_quad': map_quad, 'map_avg2': (map_single + map_quad) / 2.0}
