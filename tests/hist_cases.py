"""Inputs and exact references shared by tests/test_histograms_kernels_host.py (the kernel source compiled for the host) and
tests/test_gpu_histograms.py (the device): values, class ids, ranges and edge tables of the per-class histogram ops, and the exactly
rounded moments they are held to."""
import math

import numpy as np

T = 8192                                                   # include/uad_hip.h: UAD_SELECT_TILE
SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)       # n = 0 is a case of its own (nothing is launched)
BINS = (1, 2, 50, 1024, 1025, 2049)                        # 1025 and 2049 cross the chunk edge (UAD_HISTOGRAM_MAX_BINS = 1024) once and twice
CLASSES = (1, 2, 4)
RANGE = (0.01, 0.075)                                      # the residual histograms' range (utils/Evaluation.py:376)
KINDS = ('random', 'edges', 'specials', 'ties', 'class0_empty', 'iqr0')
MOMENT_BAR = 1e-12                                         # the project's bar for fp64 reductions (tests/test_gpu_eval.py), relative to sum |terms| / count
CHAIN_MAX = 8192                                           # 8192 * 2^-53 = 9.1e-13 < MOMENT_BAR: any fixed-order sum with a chain this long holds the bar


def ids(n, n_classes, seed=0, extra=False):
    """uint8 class ids 0 .. n_classes - 1, about 2 % of them above 0 per class (lesion-like); every class is present from n >= n_classes
    on.  extra: a few ids ABOVE n_classes - 1, which the op must drop."""
    rng = np.random.default_rng(1000 + seed + 7 * n_classes)
    lab = np.zeros(n, np.uint8)
    if n_classes > 1:
        r = rng.random(n)
        for c in range(1, n_classes):
            lab[(r >= 0.02 * (c - 1) + 0.9) & (r < 0.02 * c + 0.9)] = c
        lab[:n_classes][:n] = np.arange(n_classes, dtype=np.uint8)[:n]
    if extra and n > 5:
        lab[5::11] = n_classes
        lab[-1] = 255
    return lab


def edge_table(bins, rng_=RANGE, dtype=np.float32):
    return np.histogram_bin_edges(np.empty(0, dtype), bins, rng_)


def values(kind, n, lab, bins=50, seed=0):
    """float32 values for the case `kind` (lab: the class ids, for the kinds that depend on the class)."""
    rng = np.random.default_rng(seed + n)
    lo, hi = np.float32(RANGE[0]), np.float32(RANGE[1])
    v = (rng.random(n).astype(np.float32) ** 2 * np.float32(0.1)).astype(np.float32)       # about a third below the range, a tenth above
    if kind == 'random':
        return v
    if kind == 'edges':
        # exactly on every (float32) edge, one ulp to either side of it, both range ends and one ulp outside them
        e = edge_table(bins)
        sp = np.concatenate([e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf)),
                             [lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))]]).astype(np.float32)
        rng.shuffle(sp)
        k = min(n, sp.size)
        v[:k] = sp[:k]
        return v
    if kind == 'specials':
        sp = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, 1e30, -1e30], np.float32)
        k = min(n, sp.size)
        v[n - k:] = sp[:k]
        return v
    if kind == 'ties':
        return np.where(rng.random(n) < 0.7, np.float32(0.02), np.float32(0.05)).astype(np.float32)
    if kind == 'class0_empty':
        v[lab == 0] = np.where(rng.random(int((lab == 0).sum())) < 0.5, np.float32(0.0), np.float32(0.5))
        return v
    if kind == 'iqr0':
        v[rng.random(n) < 0.8] = np.float32(0.03125)
        return v
    raise ValueError(kind)


def exact_moments(v, lab, n_classes):
    """Per class: (count, exactly rounded mean, exactly rounded sum of (v - mean)^2 / count, sum |v| / count, sum of the squares / count) --
    math.fsum over the fp64 values; None for a class that holds an infinity (its moments are inf / nan: compared with numpy's instead)."""
    out = []
    for c in range(n_classes):
        d = v[lab == c].astype(np.float64)
        if d.size == 0 or not np.isfinite(d).all():
            out.append(None)
            continue
        mean = math.fsum(d) / d.size
        sq = (d - mean) ** 2
        out.append((d.size, mean, math.fsum(sq) / d.size, math.fsum(np.abs(d)) / d.size, math.fsum(sq) / d.size))
    return out


def moments_hold(count, mean, var, exact):
    """the bar: 1e-12 relative to sum |terms| / count"""
    n, m, s2, abs_mean, sq_mean = exact
    return count == n and abs(mean - m) <= MOMENT_BAR * abs_mean and abs(var - s2) <= MOMENT_BAR * sq_mean


def reference_counts(v, lab, n_classes, edges):
    """int64 [n_classes, bins]: np.histogram of every class on the shared table"""
    return np.stack([np.histogram(v[lab == c], bins=edges)[0] for c in range(n_classes)]).astype(np.int64)
