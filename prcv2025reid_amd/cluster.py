"""DBSCAN on the k-reciprocal Jaccard distance, on the HIP path: the pseudo-label step of SpCL / Cluster-Contrast style training on
unlabelled rows, and a way to find identities in, or deduplicate, a gallery.  Definition: DESIGN.md §22; kernels: csrc/cluster.hip
(contract in include/reid_hip.h).  The reference has no clustering.

The N x N distance matrix never exists.  Similarity rows arrive chunk by chunk (``jaccard_dbscan``: the s* rows of the pooled
re-ranker, ``Reranker.for_pool``) and each chunk is turned into its slice of the eps-neighbour CSR and dropped:
  1. per chunk               reid_dbscan_count (|N(i)| and the core flag), a chunk-local cumsum, reid_dbscan_fill (the neighbour
                             columns, ascending) from the same resident rows; one host read per chunk sizes the chunk's columns
  2. components of the cores reid_dbscan_hook / reid_dbscan_compress rounds over ``parent`` until a hook pass changes nothing; the
                             host reads one counter per round
  3. border rows             reid_dbscan_border: a non-core row takes the smallest root among the cores that reach it
  4. numbering               clusters 0, 1, .. in ascending order of their root (their smallest core row): a cumsum of root flags
Labels, core flags and the CSR are the same bits in every run (integer atomicMin / atomicAdd only).  Nothing falls back to the CPU.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Iterable, Optional, Tuple

import torch

from . import _lib, ops, rerank
from .retrieval import l2_normalize

NOISE = -1
_UNREACHED = 2 ** 31 - 1          # label of a row no core has reached yet (INT32_MAX)


@dataclass(frozen=True)
class ClusterParams:
    k1: int = 30
    k2: int = 6
    eps: float = 0.6                  # neighbours: Jaccard distance 1 - s* <= eps, i.e. s* >= float32(1 - eps)
    min_samples: int = 4              # a row counts itself, as in sklearn
    lambda_value: float = 0.0         # pure Jaccard, as SpCL uses
    sparse: Optional[bool] = None     # None: dense up to rerank.MAX_ROWS pooled rows, sparse beyond

    def __post_init__(self):
        if not 0.0 <= self.eps <= 1.0:                                     # (NaN fails both comparisons)
            raise _lib.ReidHipError(f'clustering: eps={self.eps} outside [0, 1] (a Jaccard distance)')
        if int(self.min_samples) != self.min_samples or self.min_samples < 1:
            raise _lib.ReidHipError(f'clustering: min_samples={self.min_samples} (an integer >= 1: a row counts itself)')

    def rerank_params(self, N: int) -> rerank.RerankParams:
        sparse = N > rerank.MAX_ROWS if self.sparse is None else bool(self.sparse)
        return rerank.RerankParams(k1=self.k1, k2=self.k2, lambda_value=self.lambda_value, sparse=sparse)

    @property
    def threshold(self) -> float:
        """float32(1 - eps): formed in double, rounded once."""
        return ctypes.c_float(1.0 - self.eps).value


@dataclass
class Clustering:
    labels: torch.Tensor              # i64 [N]: cluster 0 .. n_clusters - 1, -1 = noise
    core: torch.Tensor                # bool [N]
    n_clusters: int
    rounds: int                       # hook passes run, the last (which changed nothing) included
    rowptr: torch.Tensor              # i64 [N + 1], cols i32 [rowptr[N]]: the eps-neighbour lists N(i), ascending, i itself among them
    cols: torch.Tensor

    def kept(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(index i64 [M] ascending, labels i64 [M]) of the rows that are not noise: the rows and identities of a pseudo-labelled
        training set of ``n_clusters`` classes."""
        index = torch.nonzero(self.labels >= 0).flatten()
        return index, self.labels[index]

    def hybrid_labels(self) -> Tuple[torch.Tensor, int]:
        """(labels i64 [N], num_classes) for a hybrid memory (losses.HybridMemory, SpCL): the cluster numbers as they are, and every
        noise row a class of its own -- ``n_clusters`` + its rank among the noise rows in ascending row order."""
        noise = self.labels < 0
        rank = torch.cumsum(noise.to(torch.int64), 0) - 1
        return torch.where(noise, self.n_clusters + rank, self.labels), self.n_clusters + int(noise.sum())


def round_cap(N: int) -> int:
    """Hook passes allowed before ``dbscan_rows`` gives up: 4 ceil(log2(N + 1)) + 8 (a permuted chain of 65 536 rows needs 12)."""
    return 4 * math.ceil(math.log2(N + 1)) + 8


def dbscan_rows(chunks: Iterable[Tuple[int, torch.Tensor]], N: int, threshold: float, min_samples: int) -> Clustering:
    """DBSCAN of N rows from their similarity rows (larger = closer), the precomputed form.  ``chunks`` yields ``(a, S)``: S f32
    [nr, ld >= N] on the device holds rows a .. a + nr - 1 (ld % 4 == 0, 16-byte aligned; columns >= N are ignored), in ascending a,
    covering 0 .. N - 1 exactly once.  j is a neighbour of i when S[i, j] >= float32(threshold) (NaN never, +inf always) or j == i;
    a row with at least ``min_samples`` neighbours is a core.  A symmetric S gives sklearn's DBSCAN(metric='precomputed') of -S."""
    if not 1 <= N <= 2 ** 31 - 1:
        raise _lib.ReidHipError(f'clustering: N={N} outside 1..2^31 - 1 (int32 row indices)')
    if threshold != threshold:
        raise _lib.ReidHipError('clustering: the threshold is NaN')
    if int(min_samples) != min_samples or min_samples < 1:
        raise _lib.ReidHipError(f'clustering: min_samples={min_samples} (an integer >= 1: a row counts itself)')
    threshold, min_samples = ctypes.c_float(threshold).value, int(min_samples)
    dev = count = core = None
    parts, done = [], 0
    for a, S in chunks:
        if a != done or not isinstance(S, torch.Tensor) or S.dim() != 2 or S.shape[0] < 1 or a + S.shape[0] > N:
            raise _lib.ReidHipError(f'clustering: chunk at row {a} of shape {tuple(getattr(S, "shape", ()))} where rows {done}.. of {N} '
                                    'were expected (chunks ascend and cover every row once)')
        if not S.is_cuda:
            raise _lib.ReidHipError('clustering needs device tensors (there is no CPU path)')
        if count is None:
            dev = S.device
            count = torch.empty(N, dtype=torch.int32, device=dev)
            core = torch.empty(N, dtype=torch.uint8, device=dev)
        nr = S.shape[0]
        ops.dbscan_count(S, N, a, threshold, min_samples, count[a:a + nr], core[a:a + nr])
        ptr = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        torch.cumsum(count[a:a + nr], 0, dtype=torch.int64, out=ptr[1:])
        part = torch.empty(int(ptr[nr]), dtype=torch.int32, device=dev)      # the chunk's one host read
        ops.dbscan_fill(S, N, a, threshold, ptr, part)
        parts.append(part)
        done += nr
    if done != N:
        raise _lib.ReidHipError(f'clustering: the chunks end at row {done} of {N}')
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, dtype=torch.int64, out=rowptr[1:])
    cols = parts[0] if len(parts) == 1 else torch.cat(parts)
    del parts

    # components of the cores: hook + compress rounds; parent[x] <= x and parents only decrease, so every chase ends
    parent = torch.arange(N, dtype=torch.int32, device=dev)
    cap = round_cap(N)
    changed = torch.zeros(cap, dtype=torch.int32, device=dev)              # one counter per round: nothing is reset in between
    for r in range(cap):
        ops.dbscan_hook(rowptr, cols, core, parent, changed[r:r + 1])
        if int(changed[r]) == 0:                                           # the round's one host read
            rounds = r + 1
            break
        ops.dbscan_compress(parent)
    else:
        raise _lib.ReidHipError(f'clustering: the components did not settle in {cap} rounds at N={N}')

    is_core = core.bool()
    label = torch.where(is_core, parent, torch.full_like(parent, _UNREACHED))
    ops.dbscan_border(rowptr, cols, core, parent, label)
    root = is_core & (parent == torch.arange(N, dtype=torch.int32, device=dev))
    number = torch.cumsum(root, 0) - 1                                     # monotone in the root: smallest root = smallest number
    reached = label != _UNREACHED
    labels = torch.where(reached, number[label.clamp(max=N - 1).long()], torch.full_like(number, NOISE))
    return Clustering(labels=labels, core=is_core, n_clusters=int(root.sum()), rounds=rounds, rowptr=rowptr, cols=cols)


def jaccard_dbscan(feats: torch.Tensor, params: ClusterParams = ClusterParams(), normalized: bool = False, chunk: int = 1024) -> Clustering:
    """DBSCAN of the rows of ``feats`` [N, D] on the k-reciprocal Jaccard distance 1 - s*, s* from the re-ranker over the pool of these
    rows alone (``Reranker.for_pool`` / ``SparseReranker.for_pool``), ``chunk`` rows of s* at a time; the rows are L2-normalised
    unless ``normalized``.  Rows within ``params.eps`` of each other are neighbours."""
    if feats.dim() != 2:
        raise ValueError(f'feats: expected [N, D], got {tuple(feats.shape)}')
    N = feats.shape[0]
    rp = params.rerank_params(N)
    rerank.check_pool(N, rp)
    if chunk < 1:
        raise ValueError(f'chunk={chunk}: at least one row at a time')
    if not feats.is_cuda:
        raise _lib.ReidHipError('clustering needs device tensors (there is no CPU path)')
    X = feats.contiguous().float()
    if not normalized:
        X = l2_normalize(X)
    rr = (rerank.SparseReranker if rp.sparse else rerank.Reranker).for_pool(X, rp)
    return dbscan_rows(((a, rr.rows(a, min(N, a + chunk))) for a in range(0, N, chunk)), N, params.threshold, params.min_samples)


def cluster_scores(labels: torch.Tensor, pids: torch.Tensor) -> Tuple[float, float, float]:
    """(precision, recall, F1) over pairs of rows of a clustering against known identities: a pair is predicted when both rows
    share a label >= 0 (a noise row, label < 0, is a cluster of its own), true when both share a pid.  A side without a pair scores
    1.0 (nothing claimed, nothing missed); F1 is 0 when precision + recall is.  Exact int64 pair counts from the contingency table."""
    labels, pids = labels.flatten().long(), pids.flatten().long().to(labels.device)
    if labels.shape != pids.shape:
        raise ValueError(f'labels and pids: {tuple(labels.shape)} against {tuple(pids.shape)}')
    n = labels.shape[0]
    if n == 0:
        return 1.0, 1.0, 1.0
    own = labels.clamp(min=0).max() + 1 + torch.arange(n, device=labels.device)
    lab = torch.unique(torch.where(labels < 0, own, labels), return_inverse=True)[1]
    pid = torch.unique(pids, return_inverse=True)[1]

    def pairs(key):                   # pairs of rows that share a key: sum of c (c - 1) / 2 over the key's counts
        c = torch.unique(key, return_counts=True)[1]
        return int((c * (c - 1) // 2).sum())
    both, predicted, true = pairs(lab * (int(pid.max()) + 1) + pid), pairs(lab), pairs(pid)
    precision = both / predicted if predicted else 1.0
    recall = both / true if true else 1.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return precision, recall, f1
