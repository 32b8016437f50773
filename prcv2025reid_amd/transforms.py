"""Train and eval image transforms of the reference's input, run on the device (reid_augment_images, include/reid_hip.h).

Reference: datasets/dataset.py:284-297 (train), :300-307 and tools/eval_mm_protocol.py:171-173 (eval), train.py:1634-1641 (the
epoch-5 crop widening).  For given parameters the output equals PIL + torch bit for bit:

    RandomResizedCrop(S, scale) -> RandomHorizontalFlip(0.5) -> ColorJitter(brightness=0.2, contrast=0.2)
    -> ToTensor -> Normalize(ImageNet mean / std) -> RandomErasing(p, scale=(0.02, 0.2), value=0)

and ``Resize((S, S)) -> ToTensor -> Normalize`` for eval.  Input: a list of uint8 RGB HWC images (numpy arrays or CPU tensors,
e.g. ``np.asarray(Image.open(p).convert('RGB'))``), ``None`` for an absent modality (an all-zero output, the reference's
placeholder).  One call packs the images into one pinned buffer, makes one host-to-device copy and launches the kernels on the
current stream; it returns fp32 [n, 3, S, S] on the device.

The parameters are drawn from a ``torch.Generator`` the transform owns, by torchvision's procedures (torchvision itself is not a
dependency, so its exact random sequence is not reproduced -- DESIGN.md section 7), as whole-batch tensors: a constant number of
generator calls per batch.  There is no CPU path: a CPU device or output tensor raises ``ReidHipError``.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import ReidHipError

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FIELDS = 16                                # REID_AUG_FIELDS
FLIP, CONTRAST_FIRST, EMPTY = 1, 2, 4      # reid_aug_flag
ATTEMPTS = 10                              # RandomResizedCrop / RandomErasing tries per image
CROP_RATIO = (3.0 / 4.0, 4.0 / 3.0)
ERASE_SCALE, ERASE_RATIO = (0.02, 0.2), (0.3, 3.3)
JITTER = 0.2                               # ColorJitter(brightness=0.2, contrast=0.2): factors ~ U(0.8, 1.2)


def normalize_table() -> torch.Tensor:
    """[3, 256] fp32: ToTensor + Normalize of every uint8 value, by the very torch operations torchvision applies on fp32."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1)
    return v.expand(3, 256).clone().sub_(mean).div_(std)


@dataclass
class TransformParams:
    """Per-image parameters of one batch (n images).  ``size`` (H, W) = (0, 0) marks an empty slot."""
    size: np.ndarray              # int64 [n, 2]  (H, W)
    crop: np.ndarray              # int64 [n, 4]  (x, y, w, h) inside the image
    flip: np.ndarray              # bool  [n]
    contrast_first: np.ndarray    # bool  [n]     jitter order: contrast before brightness
    brightness: np.ndarray        # float32 [n]   1.0 = identity
    contrast: np.ndarray          # float32 [n]
    erase: np.ndarray             # int64 [n, 4]  (x, y, w, h) of the S x S output; w = 0: no erase

    def __len__(self):
        return len(self.size)

    @property
    def empty(self) -> np.ndarray:
        return self.size[:, 0] == 0

    def table(self, offsets: Sequence[int]) -> np.ndarray:
        """int32 [n, FIELDS] entries of reid_augment_images for images at byte ``offsets`` of the packed buffer."""
        n = len(self)
        t = np.zeros((n, FIELDS), np.int64)
        off = np.asarray(offsets, np.int64)
        t[:, 0], t[:, 1] = off & 0xFFFFFFFF, off >> 32
        t[:, 2], t[:, 3] = self.size[:, 0], self.size[:, 1]
        t[:, 4:8] = self.crop
        t[:, 8] = self.flip * FLIP + self.contrast_first * CONTRAST_FIRST + self.empty * EMPTY
        t[:, 9] = self.brightness.astype(np.float32).view(np.int32)
        t[:, 10] = self.contrast.astype(np.float32).view(np.int32)
        t[:, 11:15] = self.erase
        t[:, 0] = np.where(t[:, 0] >= 2 ** 31, t[:, 0] - 2 ** 32, t[:, 0])     # the low word as a signed int32 bit pattern
        return t.astype(np.int32)


def identity_params(sizes: Sequence[Optional[Tuple[int, int]]]) -> TransformParams:
    """Resize of the whole image, no flip, jitter or erase (the eval transform)."""
    n = len(sizes)
    size = np.array([s if s is not None else (0, 0) for s in sizes], np.int64).reshape(n, 2)
    crop = np.zeros((n, 4), np.int64)
    crop[:, 2], crop[:, 3] = size[:, 1], size[:, 0]
    return TransformParams(size, crop, np.zeros(n, bool), np.zeros(n, bool), np.ones(n, np.float32), np.ones(n, np.float32),
                           np.zeros((n, 4), np.int64))


class Packed:
    """Images packed for one call: a pinned host buffer [table | images] and the byte offset of every image after the table.
    ``apply`` writes the table into the buffer and copies the buffer to the device asynchronously; a Packed applied again (two
    views of one batch) first waits until its previous copy has read the buffer."""

    def __init__(self, images: Sequence):
        arrays = [_as_image(x) for x in images]
        self.sizes = [None if a is None else (a.shape[0], a.shape[1]) for a in arrays]
        n = len(arrays)
        self.head = (n * FIELDS * 4 + 255) // 256 * 256
        nbytes = [0 if a is None else a.size for a in arrays]
        self.offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
        self.src_bytes = int(sum(nbytes))
        self.host = torch.empty(self.head + max(self.src_bytes, 1), dtype=torch.uint8, pin_memory=True)
        flat = self.host.numpy()
        for a, o in zip(arrays, self.offsets):
            if a is not None:
                flat[self.head + o:self.head + o + a.size] = a.reshape(-1)
        self.copied: Optional[torch.cuda.Event] = None       # recorded after the last host-to-device copy of ``host``

    def __len__(self):
        return len(self.sizes)


def _as_image(x) -> Optional[np.ndarray]:
    """uint8 [H, W, 3] host array of one image; None (or an image without pixels) -> None."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.device.type != 'cpu':
            raise ValueError('images are host arrays (uint8 HWC); the transform stages them itself')
        x = x.numpy()
    a = np.asarray(x)
    if a.size == 0:
        return None
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f'expected a uint8 RGB HWC image, got {a.dtype} {tuple(a.shape)}')
    return np.ascontiguousarray(a)


class _DeviceTransform:
    def __init__(self, image_size: int = 224, device='cuda'):
        self.S = int(image_size)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ReidHipError(f'the image transforms run on the GPU only (device {self.device}): there is no CPU path')
        self._lut = {}

    def draw_params(self, sizes: Sequence[Optional[Tuple[int, int]]]) -> TransformParams:
        raise NotImplementedError

    def lut(self) -> torch.Tensor:
        dev = self.device if self.device.index is not None else torch.device('cuda', torch.cuda.current_device())
        t = self._lut.get(dev)
        if t is None:
            t = normalize_table().to(dev)
            torch.cuda.current_stream(dev).synchronize()     # (once: usable from any stream afterwards)
            self._lut[dev] = t
        return t

    def apply(self, packed: Packed, params: TransformParams, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Runs the kernels on the current stream for ``params`` (one entry per packed image); returns fp32 [n, 3, S, S]."""
        n, S = len(packed), self.S
        if len(params) != n:
            raise ValueError(f'{len(params)} parameter entries for {n} images')
        if n == 0:
            return torch.empty(0, 3, S, S, device=self.device) if out is None else out
        if list(map(tuple, params.size)) != [(0, 0) if s is None else tuple(s) for s in packed.sizes]:
            raise ValueError('parameters drawn for other image sizes')
        if out is None:
            out = torch.empty(n, 3, S, S, dtype=torch.float32, device=self.device)
        elif not out.is_cuda:
            raise ReidHipError('out must be a CUDA(HIP) tensor: there is no CPU path')
        elif out.dtype != torch.float32 or tuple(out.shape) != (n, 3, S, S) or not out.is_contiguous():
            raise ValueError(f'out: expected contiguous float32 {(n, 3, S, S)}, got {out.dtype} {tuple(out.shape)}')
        if packed.copied is not None:
            packed.copied.synchronize()                       # (reuse: the previous copy has read the table this call rewrites)
        host_table = packed.host[:packed.head].view(torch.int32)
        host_table[:n * FIELDS].copy_(torch.from_numpy(params.table(packed.offsets).reshape(-1)))
        dev = packed.host.to(out.device, non_blocking=True)                   # the one host-to-device copy: table + images
        packed.copied = torch.cuda.Event()
        packed.copied.record()
        ws = torch.empty(ops.augment_ws_bytes(n, S), dtype=torch.uint8, device=out.device)
        return ops.augment_images(dev[packed.head:], packed.src_bytes, dev[:packed.head].view(torch.int32), host_table, n, S,
                                  self.lut(), ws, out)

    def __call__(self, images: Sequence, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        packed = Packed(images)
        return self.apply(packed, self.draw_params(packed.sizes), out=out)


class EvalTransform(_DeviceTransform):
    """``Resize((S, S)) -> ToTensor -> Normalize`` (dataset.py:300-307, eval_mm_protocol.py:171-173)."""

    def draw_params(self, sizes):
        return identity_params(sizes)


class TrainTransform(_DeviceTransform):
    """The reference's training transform (dataset.py:284-297).  ``flip`` / ``crop`` False switch that step off (no crop =
    resize of the whole image); ``color_jitter`` False gives factors 1.0; ``random_erase`` is RandomErasing's p."""

    def __init__(self, image_size: int = 224, scale: Tuple[float, float] = (0.8, 1.0), flip: bool = True, crop: bool = True,
                 color_jitter: bool = True, random_erase: float = 0.0, seed: int = 0, device='cuda'):
        super().__init__(image_size, device)
        self.scale = tuple(float(s) for s in scale)
        self.flip, self.crop, self.color_jitter = bool(flip), bool(crop), bool(color_jitter)
        self.random_erase = float(random_erase)
        self.generator = torch.Generator().manual_seed(int(seed))

    @classmethod
    def from_config(cls, config, seed: int, device=None):
        """config.image_size, random_flip, random_crop, color_jitter, random_erase (configs/config.py fields)."""
        g = lambda name, default: getattr(config, name, default)
        return cls(image_size=g('image_size', 224), flip=g('random_flip', True), crop=g('random_crop', True),
                   color_jitter=g('color_jitter', True), random_erase=g('random_erase', 0.0), seed=seed,
                   device=device if device is not None else g('device', 'cuda'))

    def set_scale(self, scale: Tuple[float, float]):
        """RandomResizedCrop's area range, e.g. (0.6, 1.0) for the widening of train.py:1630-1645 (the caller decides when)."""
        self.scale = tuple(float(s) for s in scale)

    def draw_params(self, sizes: Sequence[Optional[Tuple[int, int]]]) -> TransformParams:
        p = identity_params(sizes)
        n, S, g = len(p), self.S, self.generator
        f64 = dict(dtype=torch.float64, generator=g)
        # the same six generator calls per batch whatever the switches and sizes
        crop_u = torch.rand(4, n, ATTEMPTS, **f64).numpy()      # area fraction, log ratio, row, column (of each attempt)
        flip_u = torch.rand(n, **f64).numpy()
        order = torch.rand(n, 2, **f64).argsort(dim=1).numpy()   # a permutation of (brightness, contrast) per image
        factors = torch.empty(n, 2, dtype=torch.float32).uniform_(1 - JITTER, 1 + JITTER, generator=g).numpy()
        erase_p = torch.rand(n, **f64).numpy()
        erase_u = torch.rand(4, n, ATTEMPTS, **f64).numpy()      # area fraction, log ratio, row, column
        if self.crop:
            p.crop = _random_resized_crop(p.size, self.scale, crop_u)
        if self.flip:
            p.flip = flip_u < 0.5
        if self.color_jitter:
            p.brightness, p.contrast = factors[:, 0].copy(), factors[:, 1].copy()
            p.contrast_first = order[:, 0] == 1
        if self.random_erase > 0:
            p.erase = _random_erasing(S, erase_p < self.random_erase, erase_u)
        p.crop[p.empty] = 0
        return p


def _random_resized_crop(size: np.ndarray, scale, u: np.ndarray) -> np.ndarray:
    """RandomResizedCrop.get_params for every image at once: the first of ten attempts that fits (area fraction ~ U(scale), log
    aspect ~ U(log 3/4, log 4/3), w = round(sqrt(A r)), h = round(sqrt(A / r)), corner uniform), else the centre crop clamped to
    the ratio range."""
    H, W = size[:, 0:1].astype(np.float64), size[:, 1:2].astype(np.float64)
    area = H * W * (scale[0] + (scale[1] - scale[0]) * u[0])
    lr0, lr1 = math.log(CROP_RATIO[0]), math.log(CROP_RATIO[1])
    ratio = np.exp(lr0 + (lr1 - lr0) * u[1])
    w = np.round(np.sqrt(area * ratio))
    h = np.round(np.sqrt(area / ratio))
    fits = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = fits.argmax(axis=1)
    rows = np.arange(len(size))
    w, h = w[rows, first], h[rows, first]
    y = np.floor(u[2][rows, first] * (H[:, 0] - h + 1))
    x = np.floor(u[3][rows, first] * (W[:, 0] - w + 1))
    out = np.stack([x, y, w, h], axis=1).astype(np.int64)
    for i in np.flatnonzero(~fits.any(axis=1)):               # fallback: whole image, clamped to the ratio range, centred
        Hi, Wi = int(size[i, 0]), int(size[i, 1])
        if Hi == 0:
            continue
        in_ratio = Wi / Hi
        if in_ratio < CROP_RATIO[0]:
            cw, chh = Wi, int(round(Wi / CROP_RATIO[0]))
        elif in_ratio > CROP_RATIO[1]:
            chh, cw = Hi, int(round(Hi * CROP_RATIO[1]))
        else:
            cw, chh = Wi, Hi
        out[i] = ((Wi - cw) // 2, (Hi - chh) // 2, cw, chh)
    return out


def _random_erasing(S: int, on: np.ndarray, u: np.ndarray) -> np.ndarray:
    """RandomErasing.get_params (value 0) of an S x S output for every image at once: ten attempts of area ~ U(0.02, 0.2) S^2 and
    ratio ~ logU(0.3, 3.3), h = round(sqrt(A r)), w = round(sqrt(A / r)), kept if h < S and w < S; none kept -> no erase."""
    area = S * S * (ERASE_SCALE[0] + (ERASE_SCALE[1] - ERASE_SCALE[0]) * u[0])
    lr0, lr1 = math.log(ERASE_RATIO[0]), math.log(ERASE_RATIO[1])
    ratio = np.exp(lr0 + (lr1 - lr0) * u[1])
    h = np.round(np.sqrt(area * ratio))
    w = np.round(np.sqrt(area / ratio))
    fits = (h < S) & (w < S)
    first = fits.argmax(axis=1)
    rows = np.arange(len(on))
    h, w = h[rows, first], w[rows, first]
    y = np.floor(u[2][rows, first] * (S - h + 1))
    x = np.floor(u[3][rows, first] * (S - w + 1))
    out = np.stack([x, y, w, h], axis=1).astype(np.int64)
    out[~(on & fits.any(axis=1)) | (w == 0) | (h == 0)] = 0
    return out
