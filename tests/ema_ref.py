"""numpy float32 restatement of the weight EMA (include/reid_hip.h, reid_ema_update): the schedule in double, the update as three
float32 operations each rounded once -- the contract the GPU tests check bit for bit."""
import numpy as np


def ema_decay_at(decay, warmup, t):
    """d_t in double: min((double)(float)decay, (1 + t) / (10 + t)) under warm-up, else (double)(float)decay; t counts steps from 1."""
    d = float(np.float32(decay))                 # the C ABI takes the decay as a float
    if warmup:
        d = min(d, (1.0 + float(t)) / (10.0 + float(t)))
    return d


def ema_weight(decay, warmup, t):
    """w = (float)(1.0 - d_t)."""
    return np.float32(1.0 - ema_decay_at(decay, warmup, t))


def ema_update(p, s, w):
    """s + w * (p - s) on float32 arrays: difference, product and sum are separate float32 roundings (numpy never fuses them)."""
    p = np.asarray(p, dtype=np.float32)
    s = np.asarray(s, dtype=np.float32)
    w = np.float32(w)
    d = np.subtract(p, s, dtype=np.float32)
    wd = np.multiply(w, d, dtype=np.float32)
    return np.add(s, wd, dtype=np.float32)


def ema_update_fused(p, s, w):
    """What a contracted kernel would give: fma(w, p - s, s), one rounding for product and sum (float64 holds the product of two
    float32 values exactly, and its sum with a float32 to within 2^-53 relative -- double rounding can differ from a true fma only
    on exact ties of that sum, which the power test does not rely on)."""
    p = np.asarray(p, dtype=np.float32)
    s = np.asarray(s, dtype=np.float32)
    d = np.subtract(p, s, dtype=np.float32)
    return (np.float64(np.float32(w)) * d.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


KERNEL_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 131079)


def kernel_vectors(seed=20251, rounds=3):
    """The seeded vectors of the kernel bit test: s0 per entry, and ``rounds`` draws of p per entry (standard normal float32)."""
    rng = np.random.default_rng(seed)
    s0 = [rng.standard_normal(n).astype(np.float32) for n in KERNEL_SIZES]
    ps = [[rng.standard_normal(n).astype(np.float32) for n in KERNEL_SIZES] for _ in range(rounds)]
    return s0, ps
