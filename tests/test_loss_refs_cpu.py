"""CPU: the references, scales and the gate of test_loss_kernels_gpu.py checked on their own (loss_refs.py).

  * the numpy rank-metric walk agrees with oracle.reid_oracle.rank_and_metrics on tie-free data and with a brute-force count on
    small, heavily tied cases;
  * the plain SDM / CE / BN-neck references agree with the oracle's and with torch's own;
  * the gate bites: a numpy emulation of the one-pass fp32 batch variance (sqsum / n - mu^2) fails the BN gate from |mean|/std = 30
    on, a two-pass fp32 emulation -- and the shifted fp64 pass reid_bnneck_fwd runs -- pass at every ratio up to 1000."""
import itertools

import numpy as np
import pytest
import torch

import loss_refs as R
from oracle import reid_oracle as O


def test_rank_ref_matches_oracle_on_tie_free_data():
    g = torch.Generator().manual_seed(3)
    Nq, Ng, npid = 24, 500, 9
    Q = O.l2n(torch.randn(Nq, 64, generator=g)); G = O.l2n(torch.randn(Ng, 64, generator=g))
    gp = torch.randint(0, npid, (Ng,), generator=g); qp = torch.randint(0, npid + 2, (Nq,), generator=g)
    g_img = [f'g{i}' for i in range(Ng)]
    q_img = [[g_img[j] for j in torch.randint(0, Ng, (i % 5,), generator=g).tolist()][:4] for i in range(Nq)]
    for i in range(0, Nq, 3):                                   # some queries exclude one of their own positives
        p = (gp == qp[i]).nonzero().flatten().tolist()
        if p:
            q_img[i] = q_img[i][:3] + [g_img[p[0]]]
    want = O.rank_and_metrics(Q, qp, G, gp, q_img, g_img)
    S = np.stack([O.cosine_sim(Q[i:i + 1], G).squeeze(0).numpy() for i in range(Nq)])     # the oracle's own score rows
    assert all(len(np.unique(S[i])) == Ng for i in range(Nq))   # tie-free
    ids = np.arange(Ng)
    aps, r1 = [], []
    for i in range(Nq):
        ap, rank1, npos = R.rank_metrics_ref(S[i], gp.numpy(), int(qp[i]), ids, [int(x[1:]) for x in q_img[i]])
        if npos > 0:
            aps.append(ap); r1.append(rank1)
    assert len(aps) == want['num_queries']
    assert abs(np.mean(aps) - want['mAP']) < 1e-6               # the oracle's precision column is fp32
    for k in (1, 5, 10):
        assert abs(np.mean([r <= k for r in r1]) - want[f'R@{k}']) < 1e-12


def _brute(s, g_pid, q_pid, g_img, excl):
    """rank of a positive = 1 + #kept entries that precede it under (score desc, index asc), counted pair by pair."""
    n = len(s)
    dropped = [g_img is not None and g_img[j] >= 0 and g_img[j] in excl for j in range(n)]
    pos = [j for j in range(n) if g_pid[j] == q_pid and not dropped[j]]
    if not pos:
        return 0.0, 0, 0
    ranks = sorted(1 + sum(1 for i in range(n) if not dropped[i] and (s[i] > s[j] or (s[i] == s[j] and i < j))) for j in pos)
    return sum((k + 1) / r for k, r in enumerate(ranks)) / len(pos), ranks[0], len(pos)


def test_rank_ref_matches_brute_force_on_ties():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(1, 9))
        s = (rng.integers(0, 3, n) / 8.0).astype(np.float32)    # three score levels: almost everything ties
        g_pid = rng.integers(0, 2, n); g_img = rng.integers(-1, 4, n)
        excl = [int(v) for v in rng.integers(-1, 4, int(rng.integers(0, 5)))]
        got = R.rank_metrics_ref(s, g_pid, 1, g_img, excl)
        want = _brute(s.tolist(), g_pid.tolist(), 1, g_img.tolist(), [e for e in excl if e >= 0])
        assert got[1:] == want[1:] and abs(got[0] - want[0]) < 1e-15, (trial, s, g_pid, g_img, excl, got, want)
    # every arrangement of 2 positives among 5 entries with ALL scores equal: the ranks are the indices
    for pos in itertools.combinations(range(5), 2):
        g_pid = np.array([1 if j in pos else 0 for j in range(5)])
        ap, r1, npos = R.rank_metrics_ref(np.full(5, 0.25, np.float32), g_pid, 1)
        assert (r1, npos) == (pos[0] + 1, 2) and abs(ap - 0.5 * (1 / (pos[0] + 1) + 2 / (pos[1] + 1))) < 1e-15
    assert R.rank_metrics_ref(np.zeros(3, np.float32), np.ones(3, int), 1, has_slot=False) == (0.0, 0, 0)
    assert R.rank_metrics_ref(np.zeros(R.MAX_POS + 1, np.float32), np.ones(R.MAX_POS + 1, int), 1) == (0.0, 0, -1)


def test_scales_and_gate():
    ref = torch.tensor([[1.0, 1e-6], [1e-6, 1e-9]], dtype=torch.float64)
    out = ref.clone(); out[1, 0] += 1e-9                         # 1e-3 of its own row, 1e-9 of the tensor's maximum
    assert abs(R.err_rows(out, ref) - 1e-3) < 1e-9 and abs(R.err_elems(out, ref) - 1e-3) < 1e-9
    z = torch.zeros(2, 2, dtype=torch.float64)
    assert R.err_rows(z, z) == 0.0 and R.err_rows(z + 1e-30, z) == float('inf') and R.err_elems(z + 1e-30, z) == float('inf')
    assert R.err_rows(torch.full((1, 2), float('nan')), torch.ones(1, 2)) == float('inf')
    assert abs(R.err_sums(np.array([1.0 + 1e-6]), np.array([1.0]), np.array([100.0])) - 1e-8) < 1e-12
    assert R.gate_ok(4 * R.U24, 0.0) and not R.gate_ok(4.01 * R.U24, 0.0)
    assert R.gate_ok(3.9e-6, 1e-6) and not R.gate_ok(4.1e-6, 1e-6)


def test_plain_references_agree_with_the_oracle():
    g = torch.Generator().manual_seed(5)
    q = torch.randn(9, 32, generator=g); gal = torch.randn(7, 32, generator=g)
    y = (torch.randint(0, 3, (9, 1), generator=g) == torch.randint(0, 3, (1, 7), generator=g)).float()
    for tau in (0.05, 0.2, 0.9):
        a, _ = R.sdm_plain(q, gal, y, tau); b = O.sdm_loss(q, gal, y, tau=tau)
        assert abs(float(a) - float(b)) < 2e-6
        a64, s64 = R.sdm_plain(q.double(), gal.double(), y, tau)
        assert a64.dtype == torch.float64 and abs(float(a64) - float(b)) < 2e-6 and float(s64) >= float(a64)
    z = torch.randn(11, 13, generator=g) * 3; lab = torch.randint(0, 13, (11,), generator=g)
    lab[2] = -1; lab[4] = 13
    valid = torch.ones(11, dtype=torch.uint8); valid[6] = 0
    loss, scale, d, ok = R.ce_plain(z.double(), lab, valid, 0.1, 0.7)
    assert int(ok.sum()) == 8 and float(loss[~ok].abs().max()) == 0.0 and float(d[~ok].abs().max()) == 0.0
    assert abs(float(loss[ok].mean()) - float(O.cross_entropy_ls(z[ok].double(), lab[ok], 0.1))) < 1e-12
    fl, fd = R.ce_floor(z, lab, valid, 0.1, 0.7)
    assert R.err_sums(fl, loss, scale) < 8 * R.U24 and R.err_rows(fd, d) < 8 * R.U24
    x, gamma, beta, rm, rv, dy = R.bn_inputs(16, 32, [0, 1, 10], seed=2)
    for training in (True, False):
        ref = R.bn_neck_plain(*(t.double() for t in (x, gamma, beta, rm, rv, dy)), training)
        st = {'bn_neck.bn.weight': gamma.double(), 'bn_neck.bn.bias': beta.double(), 'bn_neck.bn.running_mean': rm.double(),
              'bn_neck.bn.running_var': rv.double(), 'bn_neck.classifier.weight': torch.zeros(2, 32, dtype=torch.float64)}
        f = O.bn_neck(x.double(), st, training)[0]
        assert float((f - ref['y']).abs().max()) < 1e-12
        xr = x.double().requires_grad_(True)                     # the closed-form backward against autograd of the forward
        bn = torch.nn.functional.batch_norm(xr, rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), training, 0.1, 1e-5)
        (torch.nn.functional.normalize(bn, dim=1) * 8.0).backward(dy.double())
        assert float((xr.grad - ref['dx']).abs().max()) < 1e-12
        e = R.bn_errors(R.bn_neck_floor(x, gamma, beta, rm, rv, dy, training), ref)
        assert set(e) == set(R.BN_SCALES) and max(e[k] for k in ('y', 'mean', 'running_var', 'dz')) < 1e-5


RATIOS = (0, 1, 10, 30, 100, 300, 1000)


@pytest.mark.parametrize('rows', [8, 64])
def test_bn_gate_fails_one_pass_variance_and_passes_two_pass(rows):
    """The gate of the GPU test, applied to numpy emulations of the statistics: invstd = 1 / sqrt(var + 1e-5) per column against
    fp64, next to the floor (torch's fp32 batch norm on the CPU), each normalised by the element's own reference."""
    print()
    for ratio in RATIOS:
        x, gamma, beta, rm, rv, dy = R.bn_inputs(rows, 512, [ratio], seed=100 + rows)
        ref = R.bn_neck_plain(*(t.double() for t in (x, gamma, beta, rm, rv, dy)), True)
        floor = R.err_elems(R.bn_neck_floor(x, gamma, beta, rm, rv, dy, True)['invstd'], ref['invstd'])
        errs = {}
        for name, fn in (('one-pass', R.bn_stats_one_pass_f32), ('two-pass', R.bn_stats_two_pass_f32), ('shifted', R.bn_stats_shifted_f64)):
            mu, var = fn(x.numpy())
            inv = (np.float32(1) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
            errs[name] = R.err_elems(torch.from_numpy(inv), ref['invstd'])
            if name == 'shifted':                                # its mean is the correctly rounded one, small means included
                assert R.err_elems(torch.from_numpy(mu), ref['mean']) <= R.U24
        print(f'  rows {rows:3d} |mean|/std {ratio:5d}: invstd error one-pass {errs["one-pass"]:.2e}  two-pass {errs["two-pass"]:.2e}  '
              f'shifted-fp64 {errs["shifted"]:.2e}  floor {floor:.2e}  gate {R.gate_limit(floor):.2e}')
        assert R.gate_ok(errs['two-pass'], floor) and R.gate_ok(errs['shifted'], floor), (ratio, errs, floor)
        if ratio >= 30:
            assert not R.gate_ok(errs['one-pass'], floor), (ratio, errs, floor)
