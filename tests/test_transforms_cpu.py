"""CPU: the restatement of the device image transforms (image_transform_ref.py) against PIL, the normalisation table against
torch, the parameter draws, and the raw-image collate's masks."""
import random

import numpy as np
import pytest
import torch

import image_transform_ref as R
from prcv2025reid_amd import data as D
from prcv2025reid_amd import transforms as T
from prcv2025reid_amd.config import TrainingConfig
from test_data_cpu import make_samples

S = 224


def _cases():
    """(H, W, crop box, flip, brightness, contrast, contrast first) -- >= 200 cases with the named corners."""
    rng = np.random.default_rng(2025)
    fixed = [((1, 1), (0, 0, 1, 1)), ((40, 16), (0, 0, 16, 40)), ((300, 500), (7, 9, 1, 1)), ((224, 224), (0, 0, 224, 224)),
             ((300, 4000), (0, 0, 4000, 300)), ((4000, 300), (0, 0, 300, 4000)), ((4000, 300), (13, 100, 287, 3500)),
             ((128, 384), (0, 0, 384, 128)), ((900, 900), (0, 0, 900, 900)), ((300, 300), (76, 76, 224, 224)),
             ((600, 5), (1, 0, 3, 540)), ((3000, 20), (0, 0, 20, 3000))]     # (> 100 x taller than wide: vertical pass first)
    out = []
    for k in range(220):
        if k < len(fixed):
            (H, W), box = fixed[k]
        else:
            H, W = int(rng.integers(1, 901)), int(rng.integers(1, 901))
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            box = (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h)
        exact = k % 5 == 0
        fb = np.float32(1.0 if exact or k % 7 == 1 else rng.uniform(0.8, 1.2))
        fc = np.float32(1.0 if exact or k % 7 == 2 else rng.uniform(0.8, 1.2))
        if k % 11 == 3:
            fb, fc = np.float32(0.8), np.float32(1.2)
        out.append((H, W, box, bool(k % 3 == 0), fb, fc, bool(k % 2)))
    return out


def _pil_chain(img, box, flip, fb, fc, contrast_first):
    from PIL import Image, ImageEnhance
    x, y, w, h = box
    p = Image.fromarray(img).crop((x, y, x + w, y + h)).resize((S, S), Image.BILINEAR)
    if flip:
        p = p.transpose(Image.FLIP_LEFT_RIGHT)
    steps = [(ImageEnhance.Brightness, fb), (ImageEnhance.Contrast, fc)]
    for enhancer, f in (steps[::-1] if contrast_first else steps):
        p = enhancer(p).enhance(float(f))
    return np.asarray(p)


def test_restatement_equals_pil():
    pytest.importorskip('PIL')
    rng = np.random.default_rng(7)
    cases = _cases()
    assert len(cases) >= 200
    for H, W, box, flip, fb, fc, cf in cases:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if H * W > 10000 and rng.random() < 0.5:                # smooth content too: gradients exercise the rounding paths
            img = (np.add.outer(np.arange(H), np.arange(W))[..., None] * np.array([1, 3, 7]) % 256).astype(np.uint8)
        want = _pil_chain(img, box, flip, fb, fc, cf)
        got = R.transform_uint8(img, S, box, flip, float(fb), float(fc), cf)
        assert np.array_equal(got, want), (H, W, box, flip, fb, fc, cf, int((got != want).sum()))


def test_eval_resize_equals_pil():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(3)
    for H, W in [(128, 384), (1, 1), (500, 37), (224, 224)]:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))
        assert np.array_equal(R.resize_bilinear(img, S), want)


def test_normalize_table_is_torch_bit_for_bit():
    lut = T.normalize_table()
    v = torch.arange(256, dtype=torch.uint8)
    img = v.view(1, 256, 1).expand(3, 256, 1).permute(1, 2, 0).numpy()      # [256, 1, 3]: every value in every channel
    ref = R.normalize(img)[:, :, 0]                                            # [3, 256]
    assert lut.dtype == torch.float32 and lut.shape == (3, 256)
    assert torch.equal(lut.view(torch.int32), ref.view(torch.int32))
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)
    for c in range(3):
        for x in range(256):
            assert lut[c, x].item() == ((torch.tensor(x, dtype=torch.float32) / 255 - mean[c]) / std[c]).item()


def _train(**kw):
    kw.setdefault('random_erase', 0.3)
    return T.TrainTransform(image_size=S, seed=kw.pop('seed', 1), **kw)


def test_crop_draws_stay_in_bounds():
    t = _train()
    rng = np.random.default_rng(0)
    sizes = [(int(rng.integers(1, 2000)), int(rng.integers(1, 2000))) for _ in range(2000)]
    p = t.draw_params(sizes)
    x, y, w, h = p.crop.T
    H, W = p.size.T
    assert (x >= 0).all() and (y >= 0).all() and (w >= 1).all() and (h >= 1).all()
    assert (x + w <= W).all() and (y + h <= H).all()
    # near-square images of >= 100 px: attempt or fallback, area and aspect stay in range (up to the rounding of w and h)
    sizes = [(int(s), int(s * rng.uniform(0.9, 1.1))) for s in rng.integers(100, 2000, 2000)]
    p = t.draw_params(sizes)
    x, y, w, h = p.crop.T
    H, W = p.size.T
    area, aspect = w * h / (H * W), w / h
    assert (area >= 0.8 * 0.97).all() and (area <= 1.0).all()
    assert (aspect >= 0.75 * 0.97).all() and (aspect <= 4 / 3 * 1.03).all()
    assert (x + w <= W).all() and (y + h <= H).all() and len(set(x.tolist())) > 100


def test_crop_fallback_is_the_clamped_centre_crop():
    p = _train().draw_params([(1, 500), (500, 1), (10, 1000)])
    assert p.crop[0].tolist() == [249, 0, 1, 1]          # W / H = 500 > 4/3: h = 1, w = round(4/3) = 1, centred
    assert p.crop[1].tolist() == [0, 249, 1, 1]          # W / H < 3/4: w = 1, h = round(1 / 0.75) = 1
    assert p.crop[2].tolist() == [(1000 - 13) // 2, 0, 13, 10]


def test_erase_draws():
    t = _train(random_erase=1.0)
    p = t.draw_params([(100, 100)] * 5000)
    x, y, w, h = p.erase.T
    on = w > 0
    assert on.all()                                      # p = 1 and S = 224: an attempt always fits
    assert (x + w <= S).all() and (y + h <= S).all() and (w < S).all() and (h < S).all()
    area = w * h / (S * S)
    assert (area >= 0.02 * 0.9).all() and (area <= 0.2 * 1.1).all()
    # no attempt kept -> no erase: on a 2 x 2 output the largest area at the widest ratio gives h = round(sqrt(0.8 * 3.3)) = 2
    u = np.ones((4, 3, T.ATTEMPTS)) * 0.999
    u[:, 1, 5] = 0.5                                     # image 1: attempt 6 (ratio 1: h = w = 1) fits
    e = T._random_erasing(2, np.array([True, True, False]), u)
    assert (e[0] == 0).all() and e[1, 2:].tolist() == [1, 1] and (e[2] == 0).all()


def test_flip_and_erase_rates():
    for p_erase in (0.3, 0.5):
        p = _train(random_erase=p_erase, seed=11).draw_params([(128, 384)] * 10000)
        assert abs(p.flip.mean() - 0.5) <= 0.02
        assert abs((p.erase[:, 2] > 0).mean() - p_erase) <= 0.02
        assert abs(p.contrast_first.mean() - 0.5) <= 0.02
        assert (p.brightness >= 0.8).all() and (p.brightness <= 1.2).all() and (p.contrast >= 0.8).all() and (p.contrast <= 1.2).all()


def test_same_seed_same_table():
    sizes = [(128, 384), None, (50, 70), (1, 1)] * 20
    a = _train(seed=5).draw_params(sizes).table(np.arange(len(sizes)) * 1000)
    b = _train(seed=5).draw_params(sizes).table(np.arange(len(sizes)) * 1000)
    c = _train(seed=6).draw_params(sizes).table(np.arange(len(sizes)) * 1000)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_config_switches():
    sizes = [(128, 384)] * 500
    cfg = TrainingConfig(color_jitter=False, random_erase=0.0)
    p = T.TrainTransform.from_config(cfg, seed=1).draw_params(sizes)
    assert (p.brightness == 1.0).all() and (p.contrast == 1.0).all() and not p.contrast_first.any()
    assert (p.erase == 0).all()
    assert p.flip.any() and (p.crop[:, 2] < 384).any()
    p = T.TrainTransform.from_config(TrainingConfig(random_flip=False, random_crop=False), seed=1).draw_params(sizes)
    assert not p.flip.any() and (p.crop == [0, 0, 384, 128]).all()
    assert (p.erase[:, 2] > 0).any() and (p.brightness != 1.0).all()
    d = T.TrainTransform.from_config(TrainingConfig(), seed=1)
    assert d.scale == (0.8, 1.0) and d.random_erase == 0.3 and d.S == 224
    d.set_scale((0.6, 1.0))
    p = d.draw_params([(1000, 1000)] * 3000)
    assert (p.crop[:, 2] * p.crop[:, 3] < 0.75 * 1e6).any()


def test_table_layout():
    p = T.identity_params([(5, 7), None])
    p.flip[0] = True
    p.contrast_first[0] = True
    p.brightness[0] = np.float32(0.9)
    p.erase[0] = (1, 2, 3, 4)
    t = p.table([3 * 2 ** 32 + 2 ** 31 + 5, 0])
    assert t.dtype == np.int32 and t.shape == (2, T.FIELDS)
    assert np.uint32(t[0, 0]) == 2 ** 31 + 5 and t[0, 1] == 3
    assert t[0, 2:8].tolist() == [5, 7, 0, 0, 7, 5] and t[0, 8] == T.FLIP | T.CONTRAST_FIRST
    assert t[0, 9:11].view(np.float32).tolist() == [np.float32(0.9), 1.0] and t[0, 11:15].tolist() == [1, 2, 3, 4]
    assert t[1, 8] == T.EMPTY


def test_transform_refuses_cpu():
    from prcv2025reid_amd._lib import ReidHipError
    with pytest.raises(ReidHipError):
        T.EvalTransform(224, device='cpu')
    with pytest.raises(ReidHipError):
        T.TrainTransform.from_config(TrainingConfig(device='cpu'), seed=0)


def _raw_samples(seed):
    """make_samples with uint8 HWC images: a zero placeholder there becomes an empty array (an absent modality)."""
    rng = np.random.default_rng(seed)
    samples = make_samples(seed, image_size=8)
    for s in samples:
        for m, v in list(s['images'].items()):
            if float(v.abs().sum()) == 0:
                s['images'][m] = np.zeros((0, 0, 3), np.uint8) if rng.random() < 0.5 else torch.zeros(0, dtype=torch.uint8)
            else:
                H, W = int(rng.integers(1, 60)), int(rng.integers(1, 60))
                s['images'][m] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return samples


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_raw_collate_masks_match_collate_of_transformed(seed):
    samples = _raw_samples(seed)
    t = T.TrainTransform(image_size=32, random_erase=0.5, seed=seed)
    sm = D.StrictPKBatchSampler(samples, 3, 2, rng=random.Random(seed))
    for n, idxs in enumerate(sm):
        if n == 3:
            break
        batch = [samples[i] for i in idxs]
        raw = D.collate_raw(batch)
        transformed = []
        for s in batch:
            imgs = {}
            for m, v in s['images'].items():
                a = np.asarray(v)
                p = t.draw_params([a.shape[:2] if a.size else None])
                imgs[m] = R.transform_batch([a], p, 32)[0]
            transformed.append({**s, 'images': imgs})
        ref = D.collate(transformed, image_size=32)
        for m in D.MODALITIES + ['text']:
            assert torch.equal(raw['modality_mask'][m], ref['modality_mask'][m]), m
        assert raw['modality'] == ref['modality'] and raw['text_description'] == ref['text_description']
        assert torch.equal(raw['person_id'], ref['person_id'])
        for m in D.MODALITIES:
            assert [x is None for x in raw['images'][m]] == [float(x.abs().sum()) == 0 for x in ref['images'][m]]


def test_raw_collate_accepts_pil_images_and_refuses_paths():
    Image = pytest.importorskip('PIL.Image')
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    batch = [{'person_id': torch.tensor(1), 'images': {'vis': Image.fromarray(rgb), 'nir': Image.fromarray(rgb[..., 0])},
              'modality_mask': {'vis': 1.0, 'nir': 1.0}, 'text_description': ['a']}]
    raw = D.collate_raw(batch)
    assert np.array_equal(raw['images']['vis'][0], rgb) and raw['modality_mask']['vis'].tolist() == [1.0]
    with pytest.raises(ValueError, match='uint8 RGB HWC'):                  # a grey image is refused where it is staged
        T._as_image(raw['images']['nir'][0])
    batch[0]['images']['sk'] = '/data/sk/0001.jpg'
    with pytest.raises(ValueError, match="images\\['sk'\\]: expected a decoded image"):
        D.collate_raw(batch)
