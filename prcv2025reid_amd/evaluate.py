"""Batched MM-protocol evaluator on the HIP path.

Reference: ``rank_and_metrics`` (tools/eval_mm_protocol.py:369-469), ``_reid_map`` (train.py:450-479), the aggregation of
``validate_competition_style`` (train.py:591-602) and ``export_submission_csv`` (tools/eval_mm_protocol.py:595-649).

The reference scores one query at a time, argsorts the whole gallery row and walks it in Python.  Here
  * scores come from the MFMA GEMM of the hot path with SPLIT operands: every fp32 feature is written as a sum of 16-bit
    pieces (2 for the f16 flavor, 3 for bf16) and the significant cross products are laid side by side along K, so one
    ``reid_mer_gemm`` call returns fp32-grade similarities (error <= ~2e-7 for unit vectors, i.e. fp32 rounding level)
    at matrix-core speed;
  * AP / CMC come from ``reid_rank_metrics`` (csrc/metrics.hip): ranks of the positives only, no sort of the gallery;
  * mAP@K / CMC@K / mINP (``compute_map(k=100)`` / ``compute_cmc``, train.py:101-138: the competition's metric) come from the same pass
    with cutoffs, ``reid_rank_metrics_at``, or from ranked lists, ``reid_list_metrics`` (csrc/list_metrics.hip); ``cutoff_summary``
    forms the means.
Nothing here falls back to the CPU; the pure-Python oracle lives in oracle/reid_oracle.py and is used by tests only.
"""
from typing import TYPE_CHECKING, Dict, List, Mapping, Optional, Sequence, Tuple

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
        Nq, qp32, slot, blocks = self._scored_blocks(q_feats, q_pids, q_img_ids, ignore_same_img, chunk, normalized, rerank, expand)
        ap = torch.zeros(Nq, dtype=torch.float64, device=self.dev)
        rank1 = torch.zeros(Nq, dtype=torch.int32, device=self.dev)
        npos = torch.zeros(Nq, dtype=torch.int32, device=self.dev)
        for a, b, S, excl in blocks():
            ops.rank_metrics(S, self.g_pid, self.g_img, qp32[a:b], slot[a:b], excl,
                             self.csr_off, self.csr_idx, self.Ng, self.max_pos, ap[a:b], rank1[a:b], npos[a:b])
        return ap, rank1, npos

    def _query_ids(self, q_pids: torch.Tensor):
        """(q_pid i32 [Nq], q_slot i32 [Nq]) on the device: the CSR row of every query's pid, -1 for a pid without a gallery row."""
        qp = q_pids.to(self.dev).long()
        pos = torch.searchsorted(self._uniq, qp).clamp(max=self._uniq.numel() - 1)
        slot = torch.where(self._uniq[pos] == qp, pos, torch.full_like(pos, -1)).to(torch.int32).contiguous()
        return qp.to(torch.int32).contiguous(), slot

    def _scored_blocks(self, q_feats, q_pids, q_img_ids, ignore_same_img, chunk, normalized, rerank, expand):
        """The prologue ``per_query`` and ``per_query_at`` share: (Nq, q_pid, q_slot, blocks), where ``blocks()`` yields, per chunk of
        queries, (a, b, score rows of queries a..b, their exclusion rows or None) -- cosine rows, or s* rows with ``rerank``, of the
        expanded queries with ``expand``."""
        if expand is not None:
            q_feats, normalized = self._expanded(q_feats, expand, q_img_ids, ignore_same_img, chunk, normalized), True
        Nq = q_feats.shape[0]
        qp32, slot = self._query_ids(q_pids)
        excl = self._exclusions(q_img_ids, ignore_same_img)
        rr = None if rerank is None else self._reranker(q_feats, rerank, normalized)

        def blocks():
            for a in range(0, Nq, chunk):
                b = min(Nq, a + chunk)
                S = self.scores(q_feats[a:b], normalized) if rr is None else rr.rows(a, b)
                yield a, b, S, None if excl is None else excl[a:b].contiguous()
        return Nq, qp32, slot, blocks

    def per_query_at(self, q_feats: torch.Tensor, q_pids: torch.Tensor, ks: Sequence[int] = (100,), q_img_ids: Optional[Sequence] = None,
                     ignore_same_img: bool = True, chunk: int = 1024, normalized: bool = False, rerank: Optional['RerankParams'] = None,
                     expand: Optional['ExpansionParams'] = None) -> Dict[str, torch.Tensor]:
        """``per_query`` with cutoffs ``ks`` (ascending, at most 8): a dictionary of device tensors -- 'ap' f64, 'rank1', 'npos',
        'rank_last' i32 [Nq], 'hits' i32 and 'sum_at' f64 [Nq, len(ks)] (include/reid_hip.h, reid_rank_metrics_at; the definitions are
        DESIGN.md section 21) -- of the same rows, re-ranker and expansion; 'ap', 'rank1' and 'npos' are ``per_query``'s bit for bit.
        ``cutoff_summary`` turns them into mAP@K / R@K / mINP."""
        ops.check_cutoffs(ks)
        Nq, qp32, slot, blocks = self._scored_blocks(q_feats, q_pids, q_img_ids, ignore_same_img, chunk, normalized, rerank, expand)
        i32 = dict(dtype=torch.int32, device=self.dev)
        out = {'ap': torch.zeros(Nq, dtype=torch.float64, device=self.dev), 'rank1': torch.zeros(Nq, **i32), 'npos': torch.zeros(Nq, **i32),
               'rank_last': torch.zeros(Nq, **i32), 'hits': torch.zeros(Nq, len(ks), **i32),
               'sum_at': torch.zeros(Nq, len(ks), dtype=torch.float64, device=self.dev)}
        for a, b, S, excl in blocks():
            ops.rank_metrics_at(S, self.g_pid, self.g_img, qp32[a:b], slot[a:b], excl, self.csr_off, self.csr_idx, self.Ng, self.max_pos,
                                ks, *(out[n][a:b] for n in ('ap', 'rank1', 'npos', 'rank_last', 'hits', 'sum_at')))
        return out

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
                         rerank: Optional['RerankParams'] = None, expand: Optional['ExpansionParams'] = None,
                         ks: Optional[Sequence[int]] = None, norm: str = 'hits') -> Dict[str, float]:
        """Same dictionary as eval_mm_protocol.py:455-469: queries without an (unmasked) positive are skipped.  ``ks``: cutoffs add the
        keys of ``cutoff_summary`` (mAP@K, R@K, num_queries@K, mINP) from the same pass; None returns the dictionary above alone."""
        at = None
        if ks is None:
            ap, rank1, npos = self.per_query(q_feats, q_pids, q_img_ids, ignore_same_img, chunk, rerank=rerank, expand=expand)
        else:
            at = self.per_query_at(q_feats, q_pids, ks, q_img_ids, ignore_same_img, chunk, rerank=rerank, expand=expand)
            ap, rank1, npos = at['ap'], at['rank1'], at['npos']
        if bool((npos < 0).any()):
            raise _lib.ReidHipError('a query has more than 8192 positives in the gallery: not supported by reid_rank_metrics')
        valid = npos > 0
        n = int(valid.sum())
        if n == 0:
            res = {'mAP': 0.0, 'R@1': 0.0, 'R@5': 0.0, 'R@10': 0.0, 'num_queries': 0}
        else:
            r = rank1[valid]
            res = {'mAP': float(ap[valid].mean()), 'R@1': float((r <= 1).double().mean()), 'R@5': float((r <= 5).double().mean()),
                   'R@10': float((r <= 10).double().mean()), 'num_queries': n}
        if at is not None:
            res.update(cutoff_summary(at['sum_at'], at['hits'], rank1, at['rank_last'], npos, ks, norm))
        return res

    def reid_map(self, q_feats, q_pids, k: Optional[int] = None):
        """(mAP, top-1) of _reid_map (train.py:450-479): mAP over queries with a positive, top-1 over ALL queries.  ``k``: a cutoff
        returns (mAP@k in the 'hits' form -- compute_map(k), train.py:101-126 --, the same top-1)."""
        if k is None:
            ap, rank1, npos = self.per_query(q_feats, q_pids, None, False)
        else:
            at = self.per_query_at(q_feats, q_pids, (k,), None, False)
            ap, rank1, npos = at['ap'], at['rank1'], at['npos']
        valid = npos > 0
        n = max(1, int(valid.sum()))
        top1 = float(((rank1 == 1) & valid).double().sum() / q_feats.shape[0])
        if k is None:
            return float(ap[valid].sum() / n), top1
        return cutoff_summary(at['sum_at'], at['hits'], rank1, None, npos, (k,), 'hits')[f'mAP@{k}'], top1

    # ---------------------------------------------------------------------------------------------------------
    def per_query_lists(self, idx: torch.Tensor, q_pids: torch.Tensor, ks: Sequence[int] = (100,), q_img_ids: Optional[Sequence] = None,
                        ignore_same_img: bool = True, check_duplicates: bool = True) -> Dict[str, torch.Tensor]:
        """The per-query tensors of ``score_lists``: 'npos', 'rank1' i32 [Nq], 'hits' i32 and 'sum_at' f64 [Nq, len(ks)] of ranked
        lists ``idx`` [Nq, k] (gallery rows, best first, -1 = no entry, trailing only; reid_list_metrics, include/reid_hip.h).  'npos'
        counts the positives of the GALLERY, not of the list.  Raises ValueError for a cutoff above k (before any launch), for a
        gallery row listed twice (``check_duplicates``: a sort of the lists on the device) and for an index outside -1 .. Ng - 1."""
        idx = idx.to(self.dev)
        if idx.dim() != 2 or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f'idx: expected an integer tensor [Nq, k], got {idx.dtype} {tuple(idx.shape)}')
        if idx.shape[0] != len(q_pids):
            raise ValueError(f'idx: {idx.shape[0]} lists for {len(q_pids)} query pids')
        ops.check_cutoffs(ks, limit=idx.shape[1])
        if idx.dtype != torch.int32:                      # (an int64 index beyond int32 is out of range whatever Ng is)
            idx = idx.clamp(min=-2, max=2 ** 31 - 1)
        idx = idx.to(torch.int32).contiguous()
        if check_duplicates and idx.shape[1] > 1:
            srt = torch.sort(idx, dim=1)[0]
            twice = ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any(1)
            if bool(twice.any()):
                raise ValueError(f'ranked lists: a gallery row occurs twice in the list of query {int(twice.nonzero()[0])}')
        qp32, slot = self._query_ids(q_pids)
        npos, rank1, hits, sum_at, status = ops.list_metrics(idx, self.g_pid, self.g_img, qp32, slot, self._exclusions(q_img_ids, ignore_same_img),
                                                             self.csr_off, self.csr_idx, self.Ng, ks)
        if bool(status.any()):
            q = int(status.nonzero()[0])
            raise ValueError(f'ranked lists: query {q} holds an index outside -1 .. {self.Ng - 1} or an entry behind a -1 '
                             f'(reid_list_metrics status {int(status[q])})')
        return {'npos': npos, 'rank1': rank1, 'hits': hits, 'sum_at': sum_at}

    def score_lists(self, idx: torch.Tensor, q_pids: torch.Tensor, ks: Sequence[int] = (100,), q_img_ids: Optional[Sequence] = None,
                    ignore_same_img: bool = True, norm: str = 'hits', check_duplicates: bool = True) -> Dict[str, float]:
        """mAP@K / R@K / num_queries@K (``cutoff_summary``; no mINP: a list does not hold the last positive) of ranked lists, e.g. of
        ``ranked_lists`` or ``GalleryIndex.topk``: see ``per_query_lists``.  A gallery row the query excludes is skipped and the
        positions behind it move up, so a list is scored as the ranking without the same-image rows."""
        t = self.per_query_lists(idx, q_pids, ks, q_img_ids, ignore_same_img, check_duplicates)
        return cutoff_summary(t['sum_at'], t['hits'], t['rank1'], None, t['npos'], ks, norm)

    def score_submission_csv(self, path: str, query_pids: Mapping[str, int], gallery_img_names: Sequence, ks: Sequence[int] = (100,),
                             norm: str = 'hits') -> Dict[str, float]:
        """``score_lists`` of the file ``export_submission_csv`` writes: one row per query, ``query_key,ranked_gallery_ids`` with the
        gallery image names separated by blanks.  ``query_pids`` maps every query key to its pid; ``gallery_img_names`` are the names
        the export was given (row i of the gallery <-> name i).  Unmasked, like the export's ranking.  A list shorter than the
        largest cutoff counts as holding nothing further.  ValueError with the file's line number for an unknown query key or
        gallery name."""
        ops.check_cutoffs(ks)
        rows, pids = parse_submission_csv(path, query_pids, gallery_img_names)
        k = max(max(len(r) for r in rows), max(int(x) for x in ks))
        if k > ops.ROWS_TOPK_MAX_K:
            raise ValueError(f'{path}: lists of up to {k} entries, at most {ops.ROWS_TOPK_MAX_K} can be scored')
        idx = torch.tensor([r + [-1] * (k - len(r)) for r in rows], dtype=torch.int32)
        return self.score_lists(idx, torch.tensor(pids, dtype=torch.long), ks, None, False, norm)

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


def cutoff_summary(sum_at: torch.Tensor, hits: torch.Tensor, rank1: torch.Tensor, rank_last: Optional[torch.Tensor], npos: torch.Tensor,
                   ks: Sequence[int], norm: str = 'hits') -> Dict[str, float]:
    """mAP@K, R@K and num_queries@K for every K of ``ks`` (and mINP when ``rank_last`` is given) from the per-query tensors of
    ``per_query_at`` / ``per_query_lists``: sum_at f64 and hits [Nq, len(ks)], rank1, rank_last, npos [Nq].  Plain torch on the
    tensors' device, CPU included.  Definitions: include/reid_hip.h, DESIGN.md section 21.
      norm 'hits': AP@K = sum_K / hits_K over the queries with hits_K > 0 -- compute_map(k) of the reference (train.py:101-126);
      norm 'min':  AP@K = sum_K / min(K, npos) over the queries with npos > 0 -- the usual truncated AP.
    R@K (CMC@K) is the share of the queries with npos > 0 whose first positive ranks <= K (rank1 = 0: no positive in the list);
    num_queries@K is the number of queries in the mAP@K mean; mINP is the mean of npos / rank_last over the queries with npos > 0.
    A mean over no query is 0."""
    if norm not in ('hits', 'min'):
        raise ValueError(f"norm: expected 'hits' or 'min', got {norm!r}")
    ks = list(ops.check_cutoffs(ks))
    if tuple(sum_at.shape) != (npos.shape[0], len(ks)) or tuple(hits.shape) != tuple(sum_at.shape):
        raise ValueError(f'sum_at, hits: expected [{npos.shape[0]}, {len(ks)}], got {tuple(sum_at.shape)}, {tuple(hits.shape)}')
    has_pos = npos > 0
    n_pos = has_pos.sum().double()

    def mean(x, use, n):                                  # of x over the queries of `use`, n of them; 0 for none
        return torch.where(use, x, torch.zeros_like(x)).sum() / n.clamp(min=1.0)
    vals = [(npos < 0).any().double()]
    for c, K in enumerate(ks):
        if norm == 'hits':
            use, den = hits[:, c] > 0, hits[:, c]
        else:
            use, den = has_pos, npos.clamp(max=K)
        n = use.sum().double()
        vals += [mean(sum_at[:, c].double() / den.clamp(min=1).double(), use, n),
                 mean(((rank1 >= 1) & (rank1 <= K)).double(), has_pos, n_pos), n]
    if rank_last is not None:
        vals.append(mean(npos.double() / rank_last.clamp(min=1).double(), has_pos, n_pos))
    vals = torch.stack(vals).tolist()                     # one read-back for the whole dictionary
    if vals[0]:
        raise _lib.ReidHipError('a query has more than 8192 positives in the gallery: not evaluated by reid_rank_metrics_at')
    out: Dict[str, float] = {}
    for c, K in enumerate(ks):
        out[f'mAP@{K}'], out[f'R@{K}'], out[f'num_queries@{K}'] = vals[1 + 3 * c], vals[2 + 3 * c], int(vals[3 + 3 * c])
    if rank_last is not None:
        out['mINP'] = vals[-1]
    return out


def parse_submission_csv(path: str, query_pids: Mapping[str, int], gallery_img_names: Sequence) -> Tuple[List[List[int]], List[int]]:
    """(gallery rows per query, pid per query) of a file ``export_submission_csv`` wrote, in the file's order.  ValueError naming the
    file's line for a query key ``query_pids`` lacks or a gallery name that is not one of ``gallery_img_names`` (compared as str,
    the form the export writes; of rows that share a name the first one is meant)."""
    import csv
    row_of: Dict[str, int] = {}
    for i, name in enumerate(gallery_img_names):
        if name is not None:
            row_of.setdefault(str(name), i)
    rows, pids = [], []
    with open(path, newline='') as f:
        reader = csv.reader(f)
        if next(reader, None) != ['query_key', 'ranked_gallery_ids']:
            raise ValueError(f'{path}:1: expected the header query_key,ranked_gallery_ids')
        for rec in reader:
            line = reader.line_num
            if not rec:
                continue
            if len(rec) != 2:
                raise ValueError(f'{path}:{line}: expected 2 fields, got {len(rec)}')
            key, names = rec[0], rec[1].split()
            if key not in query_pids:
                raise ValueError(f'{path}:{line}: unknown query key {key!r}')
            unknown = [x for x in names if x not in row_of]
            if unknown:
                raise ValueError(f'{path}:{line}: unknown gallery image {unknown[0]!r}')
            rows.append([row_of[x] for x in names])
            pids.append(int(query_pids[key]))
    if not rows:
        raise ValueError(f'{path}: no query rows')
    return rows, pids


def competition_metrics(all_metrics: Dict[str, Dict[str, float]], key: Optional[str] = None) -> Dict[str, float]:
    """train.py:578-602: mean of the four single-modality mAPs, the four-modality mAP and their average.  ``key``: the entry of every
    metrics dictionary to average instead of the first of mAP / map / mAP_mean / map_mean -- 'mAP@100' for the competition's metric."""
    def _get_map(m):
        if isinstance(m, dict):
            for k in ('mAP', 'map', 'mAP_mean', 'map_mean') if key is None else (key,):
                if k in m:
                    return float(m[k])
        if isinstance(m, (int, float)):
            return float(m)
        return 0.0
    singles = [_get_map(all_metrics.get(k, {})) for k in ('single/nir', 'single/sk', 'single/cp', 'single/text')]
    map_single = sum(singles) / max(1, len([x for x in singles if x == x]))
    map_quad = _get_map(all_metrics.get('quad/nir+sk+cp+text', {}))
    return {'map_single': map_single, 'map_quad': map_quad, 'map_avg2': (map_single + map_quad) / 2.0}
