"""CPU: the fp64 reference of the cross-batch memory loss (xbm_ref.py) against its own loop form, the shadow ring's order, the config
defaults, the CPU-tensor error, and the condition that makes the GPU test's stream worth running: the ring's older rows ARE chosen."""
import pytest
import torch

import cross_triplet_ref as R
import xbm_ref as X


def _stream(P, N, D, M, ratio, normalize, margin=0.3):
    """[(step, slots of the batch, vectorised reference, loop reference)] along the stream, both rings fed alike."""
    ring, loop = X.Ring(P, M, D), X.LoopRing(P, M, D)
    out = []
    for s in range(1, X.STEPS + 1):
        q, g, lab = X.stream_step(P, N, D, ratio, s)
        slots = ring.enqueue(q, g, lab)
        loop.enqueue(q, g, lab)
        out.append((s, slots, ring.clone(), X.reference(ring, q, g, lab, None, None, margin, normalize),
                    X.loop_reference(loop, q, g, lab, None, None, margin, normalize)))
    return out


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('margin', [0.3, None])
def test_vectorised_reference_equals_the_loop_form(margin, normalize):
    P, N, D, M = 2, 8, 12, 20
    for s, slots, ring, ref, loop in _stream(P, N, D, M, 30.0, normalize, margin):
        for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
            assert ref[k].tolist() == loop[k], (s, k)
        for k in ('q_d_ap', 'q_d_an', 'q_row_loss', 'g_d_ap', 'g_d_an', 'g_row_loss'):
            assert torch.allclose(ref[k], torch.tensor(loop[k], dtype=torch.float64), rtol=1e-12, atol=1e-13), (s, k)
        assert ref['n_q'] == loop['n_q'] and ref['n_g'] == loop['n_g'] and ref['flag'] == loop['flag']
        assert all(abs(a - b) <= 1e-12 * (1 + abs(b)) for a, b in zip(ref['L'], loop['L']))
        assert max(ref['L']) > 0


def test_validity_in_the_reference_equals_the_loop_form():
    P, N, D, M = 2, 8, 12, 12
    ring, loop = X.Ring(P, M, D), X.LoopRing(P, M, D)
    for s in (1, 2, 3):
        q, g, lab = X.stream_step(P, N, D, 0.0, s)
        qv = torch.ones(P, N, dtype=torch.uint8); gv = torch.ones(N, dtype=torch.uint8)
        qv[0, s] = 0; gv[7 - s] = 0
        ring.enqueue(q, g, lab, qv, gv); loop.enqueue(q, g, lab, qv, gv)
        ref, lp = X.reference(ring, q, g, lab, qv, gv, 0.3, True), X.loop_reference(loop, q, g, lab, qv, gv, 0.3, True)
        for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n'):
            assert ref[k].tolist() == lp[k], (s, k)
        assert int(ref['q_idx_p'][0, s]) == -1 and bool((ref['g_idx_p'][:, 7 - s] == -1).all())
        assert ring.valid.tolist() == loop.valid and ring.labels.tolist() == loop.labels


def test_shadow_ring_wraps_and_overwrites_the_oldest_rows():
    P, N, D, M = 1, 3, 4, 7
    ring = X.Ring(P, M, D)
    where = {}                                                   # slot -> (step, row) it should hold
    for s in range(1, 6):
        q = torch.full((P, N, D), float(s)) + torch.arange(N)[None, :, None] / 10
        slots = ring.enqueue(q, -q[0], torch.arange(N) + 10 * s)
        assert slots.tolist() == [((s - 1) * N + i) % M for i in range(N)]
        for i, sl in enumerate(slots.tolist()):
            where[sl] = (s, i)
        assert (ring.cursor, ring.written) == ((s * N) % M, s * N)
        for sl in range(M):
            if sl in where:
                ws, wi = where[sl]
                assert float(ring.rows[1, sl, 0]) == pytest.approx(ws + wi / 10) and float(ring.rows[0, sl, 0]) == pytest.approx(-(ws + wi / 10))
                assert int(ring.labels[sl]) == wi + 10 * ws and bool(ring.valid[:, sl].all())
            else:
                assert not bool(ring.valid[:, sl].any())
    assert ring.written > M and len(where) == M                  # wrapped: every slot written, the first batches gone


def test_config_defaults():
    from prcv2025reid_amd.config import TrainingConfig
    c = TrainingConfig()
    assert (c.xbm_weight, c.xbm_size, c.xbm_margin, c.xbm_normalize, c.xbm_start_epoch) == (0.0, 4096, 0.3, True, 1)


def test_cpu_tensors_are_refused():
    from prcv2025reid_amd import losses, _lib
    q, g, lab = X.stream_step(2, 8, 12, 0.0, 1)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.xbm_cross_triplet(q, g, lab, None)
    with pytest.raises(_lib.ReidHipError, match='no CPU path'):
        losses.CrossBatchMemory(32, 3, 12, 'cpu')


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('ratio', [0.0, 30.0])
def test_the_stream_picks_rows_of_older_batches(ratio, normalize):
    """The non-vacuity condition of the GPU test: on the stream P = 2, N = 16, D = 96, M = 48, from the second step on at least one fifth
    of the kept candidates of the active anchors lie in slots of OLDER batches, and from the fourth step on the ring has wrapped."""
    P, N, D, M = 2, 16, 96, 48
    for s, slots, ring, ref in _stream_fast(P, N, D, M, ratio, normalize):
        cur = set(slots.tolist())
        picks = [int(j) for k in ('q_idx_p', 'q_idx_n', 'g_idx_p', 'g_idx_n') for j in ref[k].flatten().tolist() if j >= 0]
        older = sum(1 for j in picks if j not in cur)
        print(f'  ratio={ratio:g} normalize={normalize} step {s}: {older} of {len(picks)} picks from older batches')
        assert len(picks) == 2 * 2 * P * N                       # every anchor is active on this stream
        if s >= 2:
            assert older >= len(picks) / 5, (s, older, len(picks))
        assert (ring.written > M) == (s >= 4)


def _stream_fast(P, N, D, M, ratio, normalize):
    """_stream without the loop form (slow at this size)."""
    ring = X.Ring(P, M, D)
    for s in range(1, X.STEPS + 1):
        q, g, lab = X.stream_step(P, N, D, ratio, s)
        slots = ring.enqueue(q, g, lab)
        yield s, slots, ring.clone(), X.reference(ring, q, g, lab, None, None, 0.3, normalize)
