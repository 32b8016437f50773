"""GPU: the device image transforms (reid_augment_images) against the restatement (image_transform_ref.py) bit for bit, and the
transforming DeviceFeeder driving training steps."""
import random

import numpy as np
import pytest
import torch

import image_transform_ref as R
from prcv2025reid_amd import _lib
from prcv2025reid_amd import data as D
from prcv2025reid_amd import transforms as T

pytestmark = pytest.mark.gpu

S = 224


def _ragged_batch(n=300, seed=0):
    rng = np.random.default_rng(seed)
    fixed = [(1, 1), (1500, 900), (128, 384), (384, 128), (1, 700), (700, 1), (600, 5), (16, 40), (224, 224), (3000, 20),
             (8192, 40), (2500, 3)]
    images = []
    for k in range(n):
        if k % 17 == 5:
            images.append(None)                                  # empty slot
            continue
        H, W = fixed[k] if k < len(fixed) else (128, 384) if k % 4 == 0 else \
            (int(rng.integers(1, 1501)), int(rng.integers(1, 901)))
        images.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return images


def _varied_params(t, images, seed):
    """Drawn parameters with every flag and jitter order on and off (all combinations cycle through the batch)."""
    p = t.draw_params([None if a is None else a.shape[:2] for a in images])
    n = len(images)
    k = np.arange(n)
    p.flip = (k % 2) == 1
    p.contrast_first = (k // 2 % 2) == 1
    p.brightness[k // 4 % 3 == 0] = 1.0
    p.contrast[k // 4 % 3 == 1] = 1.0
    p.erase[k // 12 % 2 == 0] = 0
    # crops more than 100 times taller than wide that shrink vertically (the kernel's vertical-first branch), with flip and
    # jitter varying across them: the random crops of the tall images fall back to near-square ones, so they are pinned
    tall = ((6, (1, 0, 3, 540)), (9, (2, 100, 15, 2800)), (10, (0, 0, 40, 8192)), (11, (0, 37, 2, 2400)))
    for (i, box), (flip, contrast_first) in zip(tall, ((False, False), (True, False), (False, True), (True, True))):
        assert images[i] is not None and box[3] > 100 * box[2] and box[3] > t.S
        p.crop[i], p.flip[i], p.contrast_first[i] = box, flip, contrast_first
    return p


@pytest.mark.parametrize('flavor', ['bf16', 'f16'])
def test_kernel_equals_restatement_ragged(flavor):
    before = _lib.flavor()
    _lib.set_flavor(flavor)
    try:
        images = _ragged_batch()
        t = T.TrainTransform(S, random_erase=0.5, seed=3)
        packed = T.Packed(images)
        p = _varied_params(t, images, 3)
        got = t.apply(packed, p).cpu()
        torch.cuda.synchronize()
    finally:
        _lib.set_flavor(before)
    tall = [i for i in range(len(images)) if p.crop[i, 3] > 100 * p.crop[i, 2] and p.crop[i, 3] > S]
    assert len(tall) == 4 and len({(bool(p.flip[i]), bool(p.contrast_first[i])) for i in tall}) == 4
    want = R.transform_batch(images, p, S)
    bad = [i for i in range(len(images)) if not torch.equal(got[i], want[i])]
    assert not bad, [(i, None if images[i] is None else images[i].shape, p.crop[i].tolist(), int((got[i] != want[i]).sum()))
                     for i in bad[:8]]
    for i in range(len(images)):                                 # erase boxes and empty slots are exactly 0.0 (+0.0 bits)
        if images[i] is None:
            assert (got[i].view(torch.int32) == 0).all()
        x, y, w, h = p.erase[i]
        if w > 0:
            assert (got[i][:, y:y + h, x:x + w].view(torch.int32) == 0).all()


def test_eval_transform_equals_restatement_and_pil():
    rng = np.random.default_rng(1)
    # (3000, 20), (8192, 40): more than 100 times taller than wide and shrinking -- Image.resize's vertical-first path
    sizes = [(128, 384), (1, 1), (900, 1500), (224, 224), (50, 7000), (3000, 20), (8192, 40)]
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
    images.insert(2, None)
    t = T.EvalTransform(S)
    got = t(images).cpu()
    p = T.identity_params([None if a is None else a.shape[:2] for a in images])
    assert torch.equal(got, R.transform_batch(images, p, S))
    # a pinned tall crop through apply: (600, 5) cropped to 3 x 540
    tall = [rng.integers(0, 256, (600, 5, 3), dtype=np.uint8)]
    q = T.identity_params([(600, 5)])
    q.crop[0] = (1, 0, 3, 540)
    got_tall = t.apply(T.Packed(tall), q).cpu()
    assert torch.equal(got_tall, R.transform_batch(tall, q, S))
    try:
        from PIL import Image
    except ImportError:
        return
    for i, a in enumerate(images):
        if a is not None:
            pil = R.normalize(np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR)))
            assert torch.equal(got[i], pil)
    pil = R.normalize(np.asarray(Image.fromarray(tall[0]).crop((1, 0, 4, 540)).resize((S, S), Image.BILINEAR)))
    assert torch.equal(got_tall[0], pil)


def test_same_seed_same_bytes():
    images = _ragged_batch(64, seed=4)
    outs = [T.TrainTransform(S, random_erase=0.5, seed=9)(images).cpu() for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_train_transform_call_equals_restatement_with_out():
    images = _ragged_batch(40, seed=6)
    t = T.TrainTransform(S, random_erase=0.5, seed=2)
    p = T.TrainTransform(S, random_erase=0.5, seed=2).draw_params([None if a is None else a.shape[:2] for a in images])
    out = torch.full((len(images), 3, S, S), 7.0, device='cuda')
    r = t(images, out=out)
    assert r.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), R.transform_batch(images, p, S))


def test_packed_applied_twice_without_sync():
    # two augmented views of one batch: the second call rewrites the pinned table only after the first copy has read it
    images = _ragged_batch(40, seed=7)
    t = T.TrainTransform(S, random_erase=0.5, seed=4)
    packed = T.Packed(images)
    sizes = [None if a is None else a.shape[:2] for a in images]
    p1, p2 = t.draw_params(sizes), t.draw_params(sizes)
    torch.cuda._sleep(100_000_000)                               # the stream is busy: the first copy is queued behind this
    a = t.apply(packed, p1)
    b = t.apply(packed, p2)
    assert torch.equal(a.cpu(), R.transform_batch(images, p1, S))
    assert torch.equal(b.cpu(), R.transform_batch(images, p2, S))


def test_bad_sizes_and_buffers_raise_before_launch():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    t = T.EvalTransform(S)
    packed = T.Packed([img])
    p = T.identity_params([(20, 30)])
    out = torch.full((1, 3, S, S), 5.0, device='cuda')
    for field, value in [('crop', [0, 0, 31, 20]), ('crop', [-1, 0, 30, 20]), ('erase', [200, 0, 30, 10])]:
        q = T.identity_params([(20, 30)])
        getattr(q, field)[0] = value
        with pytest.raises(_lib.ReidHipError, match='outside'):
            t.apply(packed, q, out=out)
    q = T.identity_params([(20, 30)])
    q.brightness[0] = np.nan
    with pytest.raises(_lib.ReidHipError, match='jitter'):
        t.apply(packed, q, out=out)
    big = T.Packed([np.zeros((1, 9000, 3), np.uint8)])
    with pytest.raises(_lib.ReidHipError, match='8192'):
        t.apply(big, T.identity_params([(1, 9000)]), out=out)
    packed.src_bytes -= 1                                        # the image no longer fits the source buffer
    with pytest.raises(_lib.ReidHipError, match='src_bytes'):
        t.apply(packed, p, out=out)
    with pytest.raises(_lib.ReidHipError, match='S=6'):
        T.EvalTransform(6).apply(T.Packed([img]), p, out=torch.empty(1, 3, 6, 6, device='cuda'))
    with pytest.raises(_lib.ReidHipError):
        t.apply(T.Packed([img]), p, out=torch.empty(1, 3, S, S))
    torch.cuda.synchronize()
    assert (out == 5.0).all()                                    # nothing was launched


def test_feeder_with_transform_drives_training_steps():
    from helpers import load_case, case_inputs
    from test_data_cpu import make_samples
    from test_model_gpu import build_model
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    z, meta = load_case('tiny_train_frozen')
    cfg, arch, state, batch, tokens = case_inputs(meta)
    model = build_model(meta, state, True)
    rng = np.random.default_rng(8)
    samples = make_samples(4, n_pid=5, image_size=4)
    for s in samples:                                           # raw uint8 images; a zero placeholder becomes an absent image
        s['person_id'] = torch.tensor(int(s['person_id']) - 1)
        for m, v in list(s['images'].items()):
            s['images'][m] = np.zeros((0, 0, 3), np.uint8) if float(v.abs().sum()) == 0 else \
                rng.integers(0, 256, (int(rng.integers(20, 200)), int(rng.integers(20, 200)), 3), dtype=np.uint8)
    sm = D.StrictPKBatchSampler(samples, 3, 2, rng=random.Random(7))
    picked = []

    def limited(n=4):
        for i, b in enumerate(sm):
            if i == n:
                return
            picked.append(b)
            yield b
    size = arch['image_size']
    transform = T.TrainTransform(size, random_erase=0.5, seed=1)
    feeder = D.DeviceFeeder(samples, limited(), model.tokenizer, 'cuda', depth=2, transform=transform)
    gs = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in model.get_learnable_params()]
    drv = StepDriver(model, FusedAdamW(gs, weight_decay=1e-4))
    drv.start_epoch(2)
    losses = []
    for k, b in enumerate(feeder):
        assert b['images']['vis'].is_cuda and b['images']['vis'].dtype == torch.float32 and not b['modality_mask']['vis'].is_cuda
        raw = D.collate_raw([samples[i] for i in picked[k]])
        flat = [img for m in D.MODALITIES for img in raw['images'][m]]
        want = R.transform_batch(flat, b['transform_params'], size)
        got = torch.cat([b['images'][m] for m in D.MODALITIES]).cpu()
        assert torch.equal(got, want)
        for m in D.MODALITIES:
            assert torch.equal(b['modality_mask'][m], raw['modality_mask'][m])
        L = drv.step(b['images'], b['tokens'], b['modality_mask'], b['person_id'])
        losses.append(float(L['total_loss'].detach()))
    assert len(losses) == 4 and all(x == x and abs(x) < 1e4 for x in losses)
    assert drv.opt.step_count == 4
