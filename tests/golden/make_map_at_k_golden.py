#!/usr/bin/env python3
"""Generate tests/golden/map_at_k.npz from the reference itself.  BUILD CONTAINER ONLY.

``compute_map`` (train.py:101-126, mAP@k) and ``compute_cmc`` (train.py:128-138, CMC@k) are pulled out of the reference's
``train.py`` by ``ast`` at generation time, as make_golden.py does for ``_reid_map`` (the module itself cannot be imported), and
executed on a small seeded retrieval case.  Only data is stored: Q, G, the pids and the reference's values.

The reference ranks with an UNSTABLE ``torch.sort`` of a plain fp32 ``mm``; the evaluator ranks fp32-grade scores (error < 4e-7,
tests/test_evaluate_gpu.py::test_scores_are_fp32_grade) with a defined tie rule.  So that neither ties nor rounding can change a
rank, seeds are tried until every query's adjacent sorted similarities differ by at least MIN_GAP = 1e-5, and that is asserted.

The case: Nq = 16, Ng = 64, D = 64; 8 gallery identities of unequal sizes (1 .. 20 rows) and three query pids without a gallery row,
so k = 100 > Ng and k = 20 < Ng both occur and some queries have no positive among their first 1 or 5.

Usage:  python tests/golden/make_map_at_k_golden.py
"""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
PATH = os.path.join(HERE, 'map_at_k.npz')
MAP_KS = (1, 5, 20, 100)
CMC_KS = (1, 5, 10, 20)
MIN_GAP = 1e-5
NQ, NG, D = 16, 64, 64
SIZES = (1, 2, 3, 5, 8, 11, 14, 20)              # rows per gallery identity 0..7: sum = NG
ABSENT = (100, 101, 102)                         # query pids without a gallery row


def reference_functions():
    """{'compute_map', 'compute_cmc'} compiled from the reference's train.py."""
    path = os.path.join(REF, 'train.py')
    src = open(path, encoding='utf-8').read()
    ns = {'torch': torch, 'np': np, 'F': F}
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name in ('compute_map', 'compute_cmc'):
            node.decorator_list = []
            exec(compile('def ' + ast.get_source_segment(src, node).split('def ', 1)[1], 'train.py', 'exec'), ns)
    return ns['compute_map'], ns['compute_cmc']


def case(seed):
    """(Q, G, q_pid, g_pid) of one seed: clustered features, so positives rank early but not always first."""
    assert sum(SIZES) == NG
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(len(SIZES) + len(ABSENT), D, generator=g)
    g_pid = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(SIZES)])[torch.randperm(NG, generator=g)]
    q_pid = torch.cat([torch.arange(len(SIZES)), torch.randint(0, len(SIZES), (NQ - len(SIZES) - len(ABSENT),), generator=g),
                       torch.tensor(ABSENT)])[torch.randperm(NQ, generator=g)]
    row = torch.where(q_pid >= ABSENT[0], q_pid - ABSENT[0] + len(SIZES), q_pid)
    G = centers[g_pid] * 0.35 + torch.randn(NG, D, generator=g)
    Q = centers[row] * 0.35 + torch.randn(NQ, D, generator=g)
    return Q, G, q_pid, g_pid


def min_gap(Q, G):
    """The smallest difference of adjacent sorted similarities over all queries, of the reference's own fp32 product."""
    sim = torch.mm(F.normalize(Q, p=2, dim=1), F.normalize(G, p=2, dim=1).t())
    s = torch.sort(sim, dim=1, descending=True)[0].double()
    return float((s[:, :-1] - s[:, 1:]).min())


def generate():
    """The fixture's contents as a dictionary of numpy values."""
    compute_map, compute_cmc = reference_functions()
    for seed in range(1000):
        Q, G, q_pid, g_pid = case(seed)
        if min_gap(Q, G) >= MIN_GAP:
            break
    assert min_gap(Q, G) >= MIN_GAP, 'no seed separates every pair of adjacent similarities'
    return dict(Q=Q.numpy(), G=G.numpy(), q_pid=q_pid.numpy(), g_pid=g_pid.numpy(), seed=np.int64(seed),
                map_ks=np.array(MAP_KS, dtype=np.int64), cmc_ks=np.array(CMC_KS, dtype=np.int64),
                map_at=np.array([compute_map(Q, G, q_pid, g_pid, k=k) for k in MAP_KS], dtype=np.float64),
                cmc_at=np.array([compute_cmc(Q, G, q_pid, g_pid, k=k) for k in CMC_KS], dtype=np.float64))


if __name__ == '__main__':
    out = generate()
    np.savez_compressed(PATH, **out)
    print(f"[map_at_k] seed {int(out['seed'])}, min gap {min_gap(torch.tensor(out['Q']), torch.tensor(out['G'])):.3g}: mAP@{MAP_KS} = {out['map_at']}, "
          f"CMC@{CMC_KS} = {out['cmc_at']} -> {PATH} ({os.path.getsize(PATH)} bytes)")
