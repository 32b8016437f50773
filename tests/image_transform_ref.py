"""Restatement of the device image transforms in numpy / torch, given their parameters (test code; no PIL import).

What it restates (prcv2025reid_amd/transforms.py, csrc/augment.hip): PIL's ``Image.crop(box).resize((S, S), BILINEAR)``
(ImagingResample: separable, horizontal pass first -- vertical first for an image more than 100 times taller than wide that
shrinks vertically, as Image.resize does -- each pass rounded to uint8; precompute_coeffs in double, 22-bit fixed-point
coefficients int(0.5 + k * 2^22), accumulator 2^21 + sum v * k, >> 22, clamp), the mirror, ``ImageEnhance.Brightness`` /
``.Contrast`` (Image.blend: trunc(float32(d) + float32(f) * float32(v - d)), contrast's d = int(mean luma + 0.5) with PIL's
fixed-point luma), ToTensor + Normalize in torch fp32, RandomErasing with value 0, zeros for an empty slot.
"""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _tri(x: float) -> float:
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def coefficients(in_size: int, out_size: int) -> np.ndarray:
    """float64 [out_size, in_size] matrix of the integer coefficients of one pass (precompute_coeffs + normalize_coeffs_8bpc)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    K = np.zeros((out_size, in_size), np.float64)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [_tri((x + lo - center + 0.5) * ss) for x in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            K[xx, lo + x] = int(0.5 + k * (1 << 22)) if k >= 0 else int(-0.5 + k * (1 << 22))
    return K


def _pass(img: np.ndarray, K: np.ndarray, axis: int) -> np.ndarray:
    # integer products and sums stay below 2^31, so float64 matrix products are exact
    x = img.astype(np.float64)
    acc = np.tensordot(K, x, axes=([1], [axis]))               # the resampled axis comes first
    if axis == 1:
        acc = acc.transpose(1, 0, 2)
    acc = acc.astype(np.int64) + (1 << 21)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize_bilinear(img: np.ndarray, S: int) -> np.ndarray:
    """uint8 [H, W, 3] -> [S, S, 3] as PIL's resize((S, S), BILINEAR) of the whole image."""
    H, W = img.shape[:2]
    out = img
    if H > 100 * W and S < H:          # Image.resize: a very tall image is first resized vertically, then horizontally
        out = _pass(out, coefficients(H, S), axis=0)
        if W != S:
            out = _pass(out, coefficients(W, S), axis=1)
        return np.ascontiguousarray(out)
    if W != S:
        out = _pass(out, coefficients(W, S), axis=1)
    if H != S:
        out = _pass(out, coefficients(H, S), axis=0)
    return np.ascontiguousarray(out)


def blend(d, img: np.ndarray, f) -> np.ndarray:
    """Image.blend(degenerate d, img, f) on uint8 (ImagingBlend: float32 arithmetic, truncation, clamp)."""
    f32 = np.float32(f)
    dd = np.float32(d)
    t = dd + f32 * (img.astype(np.int32) - np.int32(d)).astype(np.float32)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def contrast_degenerate(img: np.ndarray) -> int:
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    L = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16
    return int(int(L.sum()) / L.size + 0.5)


def normalize(img: np.ndarray) -> torch.Tensor:
    """ToTensor + Normalize exactly as torchvision computes them on fp32."""
    t = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    return t.sub_(mean).div_(std)


def transform_uint8(img: np.ndarray, S: int, crop, flip: bool, brightness: float, contrast: float,
                    contrast_first: bool) -> np.ndarray:
    """Crop + resize, flip and jitter of one image: uint8 [S, S, 3] (the PIL image before ToTensor)."""
    x, y, w, h = (int(v) for v in crop)
    out = resize_bilinear(img[y:y + h, x:x + w], S)
    if flip:
        out = np.ascontiguousarray(out[:, ::-1])
    steps = [('b', brightness), ('c', contrast)]
    for kind, f in (steps[::-1] if contrast_first else steps):
        out = blend(0 if kind == 'b' else contrast_degenerate(out), out, f)
    return out


def transform_one(img, S: int, crop, flip, brightness, contrast, contrast_first, erase) -> torch.Tensor:
    """fp32 [3, S, S] of one image (None = empty slot: zeros)."""
    if img is None:
        return torch.zeros(3, S, S)
    t = normalize(transform_uint8(img, S, crop, flip, brightness, contrast, contrast_first))
    ex, ey, ew, eh = (int(v) for v in erase)
    if ew > 0 and eh > 0:
        t[:, ey:ey + eh, ex:ex + ew] = 0.0
    return t


def transform_batch(images, params, S: int) -> torch.Tensor:
    """fp32 [n, 3, S, S] for a list of uint8 HWC images (None = empty) and a TransformParams."""
    return torch.stack([transform_one(None if params.size[i, 0] == 0 else np.asarray(images[i]), S, params.crop[i],
                                      bool(params.flip[i]), float(params.brightness[i]), float(params.contrast[i]),
                                      bool(params.contrast_first[i]), params.erase[i]) for i in range(len(images))])
