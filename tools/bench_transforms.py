"""Device image transforms: kernel time per batch, fed-vs-resident training step, and the PIL chain on the host CPU.

    python tools/bench_transforms.py --kernels [--reps 50]   # config-2 batch (256 x 128x384) and a mixed-size batch;
                                                             # run under rocprofv3 --kernel-trace --stats for per-kernel times
    python tools/bench_transforms.py --steps [--rounds 3 --block 10 --rank 8]   # StepDriver on config 2 (P=16, K=4, r=8):
                                                             # resident inputs against a transforming DeviceFeeder, alternated
                                                             # in blocks, each fed block timed in steady state
    python tools/bench_transforms.py --pil [--images 200]    # ms per image of the PIL chain on one host core
Prints one JSON line per section.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29          # measured HBM copy rate of the MI355X (TB/s): the byte floor of a transform


def kernels(reps):
    from prcv2025reid_amd import transforms as T
    rng = np.random.default_rng(0)
    sets = {'config2_256x128x384': [rng.integers(0, 256, (128, 384, 3), dtype=np.uint8) for _ in range(256)],
            'mixed_256': [rng.integers(0, 256, (int(rng.integers(32, 1500)), int(rng.integers(32, 900)), 3), dtype=np.uint8)
                          for _ in range(256)]}
    t = T.TrainTransform(224, random_erase=0.3, seed=0)
    for name, images in sets.items():
        packed = T.Packed(images)
        params = t.draw_params(packed.sizes)
        out = torch.empty(len(images), 3, 224, 224, device='cuda')
        for _ in range(3):
            t.apply(packed, params, out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            t.apply(packed, params, out=out)
        e1.record()
        torch.cuda.synchronize()
        src = packed.src_bytes
        moved = src + out.numel() * 4 + 2 * len(images) * 3 * 224 * 224      # source read, fp32 written, uint8 scratch written + read
        print(json.dumps({'section': 'kernels', 'set': name, 'images': len(images), 'src_MB': round(src / 1e6, 2),
                          'apply_incl_h2d_us': round(e0.elapsed_time(e1) * 1e3 / reps, 1), 'bytes_moved_MB': round(moved / 1e6, 1),
                          'byte_floor_us': round(moved / (COPY_TBS * 1e12) * 1e6, 1),
                          'fp32_out_floor_us': round(out.numel() * 4 / (COPY_TBS * 1e12) * 1e6, 1)}), flush=True)


def steps(rounds, block, rank):
    import bench
    from prcv2025reid_amd import data as D
    from prcv2025reid_amd import transforms as T
    from prcv2025reid_amd.synthetic import synthetic_batch
    from prcv2025reid_amd.trainer import FusedAdamW, StepDriver
    P, K, C = 16, 4, 400
    dev = torch.device('cuda', 0)
    model = bench.build_model(0, rank, 'bf16', C)
    batch = synthetic_batch(P, K, model.arch, seed=1000, mask_drop=0.0, num_classes=C)
    images = {m: t.to(dev) for m, t in batch['images'].items()}
    masks = batch['modality_mask']
    tok = model.tokenizer(batch['texts'], return_tensors='pt', padding=True, truncation=True, max_length=77)
    tokens = {k: v.to(dev) for k, v in tok.items()}
    labels = batch['person_id'].to(dev)
    groups = [dict(params=[p for p in g['params'] if p.requires_grad], lr=g['lr'], name=g['name']) for g in model.get_learnable_params()]
    drv = StepDriver(model, FusedAdamW([g for g in groups if g['params']], weight_decay=1e-4), adaptive_clip=True)
    rng = np.random.default_rng(1)
    samples = [{'person_id': torch.tensor(i // K), 'images': {m: rng.integers(0, 256, (128, 384, 3), dtype=np.uint8) for m in D.MODALITIES},
                'modality_mask': {m: 1.0 for m in D.MODALITIES}, 'text_description': [batch['texts'][i]]} for i in range(P * K)]

    def resident(n):
        for _ in range(n):
            drv.step(images, tokens, masks, labels)

    def fed(n, warm=2, depth=2):
        # steady state: `warm` untimed steps from the same feeder first, and enough batches behind the timed ones that the
        # worker keeps transforming one batch per consumed batch throughout the n timed steps
        feeder = D.DeviceFeeder(samples, [list(range(P * K))] * (warm + n + depth + 1), model.tokenizer, dev, depth=depth,
                                transform=T.TrainTransform(224, random_erase=0.3, seed=0))
        it = iter(feeder)
        for _ in range(warm):
            b = next(it)
            drv.step(b['images'], b['tokens'], b['modality_mask'], b['person_id'])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            b = next(it)
            drv.step(b['images'], b['tokens'], b['modality_mask'], b['person_id'])
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        for _ in it:                                       # (drain the worker)
            pass
        return elapsed / n

    resident(3)
    fed(3)
    res, fd = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident(block)
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) / block * 1e3)
        fd.append(fed(block) * 1e3)
    print(json.dumps({'section': 'steps', 'P': P, 'K': K, 'lora_rank': rank, 'block': block, 'resident_ms': [round(x, 2) for x in res],
                      'fed_ms': [round(x, 2) for x in fd],
                      'fed_over_resident': round(float(np.median(fd) / np.median(res)), 4)}), flush=True)


def pil(n):
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(2)
    imgs = [Image.fromarray(rng.integers(0, 256, (128, 384, 3), dtype=np.uint8)) for _ in range(n)]
    mean = torch.tensor([0.485, 0.456, 0.406]).view(-1, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(-1, 1, 1)
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for im in imgs:
        p = im.crop((10, 5, 350, 120)).resize((224, 224), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT)
        p = ImageEnhance.Contrast(ImageEnhance.Brightness(p).enhance(1.1)).enhance(0.9)
        t = torch.from_numpy(np.array(p)).permute(2, 0, 1).contiguous().float().div(255).sub_(mean).div_(std)
        t[:, 10:60, 20:90] = 0
    ms = (time.perf_counter() - t0) / n * 1e3
    print(json.dumps({'section': 'pil', 'images': n, 'ms_per_image_one_core': round(ms, 3),
                      'cores_for_8300_images_per_s': round(8300 * ms / 1e3, 1)}), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--steps', action='store_true')
    ap.add_argument('--pil', action='store_true')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--rank', type=int, default=8, help='MER-LoRA rank of the step (BASELINE config 2: 8)')
    ap.add_argument('--images', type=int, default=200)
    a = ap.parse_args()
    if a.kernels:
        kernels(a.reps)
    if a.steps:
        steps(a.rounds, a.block, a.rank)
    if a.pil:
        pil(a.images)
