"""NII.normalize(method='standardization') of the reference (utils/NII.py:53-75, and its copy dataloaders/NRRD.py:39-60) as a host statement:
clamp to the lower / upper percentile exactly as the 'scaling' method does, `c = v - np.mean(v)`, `out = c / np.std(c)` in float32 -- np.std
is taken of the CENTRED data, so it subtracts the float32 mean of c (near zero, not zero) once more before it squares; population variance.

Stated deviation: numpy adds its float32 sums in an order of its own.  Here the three sums are fp64 sums in a DEFINED order and each scalar
is rounded to float32 once:

    mean32 = f32(sum v / n)        c_i = f32(v_i - mean32)
    m2_32  = f32(sum c_i / n)      e_i = f32(c_i - m2_32)
    var32  = f32(sum f32(e_i * e_i) / n),  std32 = sqrtf(var32),  out_i = f32(c_i / std32)

`shifted_sums` adds in the order of csrc/uad_moments.hip (include/uad_hip.h: uad_shifted_sums) and returns the kernel's bits: tile T holds
the values [T * 8192, (T + 1) * 8192); thread t of a tile adds the values T * 8192 + (r * 256 + t) * 4 + e, r = 0 .. 7, e = 0 .. 3, below n in
that order to +0.0; the 256 runs of a tile are added as a tree (level d = 128, 64, ... 1: run t + d onto run t); the tile partials are added
as 256 strided runs (t, t + 256, ...) and the same tree.  A place past n adds +0.0, which changes no bit of a sum that started at +0.0.
This module is the path without a device engine and the reference of the device tests."""
import numpy as np

TILE, THREADS, RUN = 8192, 256, 32                                  # include/uad_hip.h: UAD_SELECT_TILE; csrc/uad_moments.hip: MS_THREADS, MS_RUN
MAX_N = 2 ** 31 - 1
SUM_CHAIN = 1072                                                    # include/uad_hip.h: UAD_SHIFTED_SUMS_CHAIN


def sum_chain(n):
    """The longest chain of dependent fp64 additions behind a sum of n terms: 32 + 8 + ceil(tiles / 256) + 8."""
    tiles = -(-int(n) // TILE)
    return RUN + 8 + -(-tiles // THREADS) + 8


def _tree(runs):
    """[..., 256] fp64 -> [...]: level d adds run t + d onto run t for t < d."""
    runs = np.array(runs, np.float64)
    d = THREADS // 2
    while d >= 1:
        runs[..., :d] = runs[..., :d] + runs[..., d:2 * d]
        d //= 2
    return runs[..., 0]


def ordered_sum(terms):
    """The fp64 sum of a 1-D array of terms in the order stated above (the terms are taken to fp64 exactly)."""
    x = np.asarray(terms).reshape(-1).astype(np.float64)
    n = x.size
    if n == 0:
        return np.float64(0.0)
    tiles = -(-n // TILE)
    pad = np.zeros(tiles * TILE, np.float64)
    pad[:n] = x
    chunks = pad.reshape(tiles, RUN // 4, THREADS, 4)               # [tile, round, thread, place]
    runs = np.zeros((tiles, THREADS), np.float64)
    for r in range(RUN // 4):
        for e in range(4):
            runs = runs + chunks[:, r, :, e]
    partials = _tree(runs)                                           # [tiles]
    rounds = -(-tiles // THREADS)
    pad = np.zeros(rounds * THREADS, np.float64)
    pad[:tiles] = partials
    runs = np.zeros(THREADS, np.float64)
    for k in range(rounds):
        runs = runs + pad[k * THREADS:(k + 1) * THREADS]
    return _tree(runs)


def clamp(v, clamp_lo=None, clamp_hi=None):
    """float32 copy of v with numpy's `v[v < lo] = lo; v[v > hi] = hi` (None = no bound)."""
    v = np.array(v, np.float32)
    if clamp_lo is not None:
        v[v < np.float32(clamp_lo)] = np.float32(clamp_lo)
    if clamp_hi is not None:
        v[v > np.float32(clamp_hi)] = np.float32(clamp_hi)
    return v


def shifted_terms(v, clamp_lo=None, clamp_hi=None, shift=0.0, centre=0.0):
    """(u, f32(u * u)) for u = f32(f32(clamp(v) - shift) - centre): the float32 terms shifted_sums adds."""
    with np.errstate(over='ignore', invalid='ignore'):
        u = (clamp(v, clamp_lo, clamp_hi).reshape(-1) - np.float32(shift)) - np.float32(centre)
        return u, u * u


def shifted_sums(v, clamp_lo=None, clamp_hi=None, shift=0.0, centre=0.0):
    """-> (sum u, sum f32(u * u)) as Python floats, fp64 sums in the kernel's order (uad_shifted_sums returns the same bits)."""
    if np.size(v) > MAX_N:
        raise ValueError(f'at most 2^31 - 1 values, got {np.size(v)}')
    u, q = shifted_terms(v, clamp_lo, clamp_hi, shift, centre)
    return float(ordered_sum(u)), float(ordered_sum(q))


def moments_from(sums_of, n):
    """The three reductions of the statement around a callable sums_of(shift, centre) -> (sum u, sum u^2): -> (mean32, std32) float32.
    The host statement and the device route share this, so the scalars are rounded in one place."""
    with np.errstate(invalid='ignore', divide='ignore'):
        mean32 = np.float32(np.float64(sums_of(0.0, 0.0)[0]) / n)
        m2_32 = np.float32(np.float64(sums_of(mean32, 0.0)[0]) / n)
        var32 = np.float32(np.float64(sums_of(mean32, m2_32)[1]) / n)
        return mean32, np.sqrt(var32)


def standardize_clamped(v, clamp_lo=None, clamp_hi=None, return_moments=False):
    """The statement with given clamp bounds (None = no bound): float32 array of v's shape[, (mean32, std32)]."""
    shape = np.shape(v)
    c = clamp(v, clamp_lo, clamp_hi)
    mean32, std32 = moments_from(lambda shift, centre: shifted_sums(c, None, None, shift, centre), c.size)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = ((c - mean32) / std32).reshape(shape)
    return (out, (mean32, std32)) if return_moments else out


def standardize(v, lower=0, upper=99.8, return_moments=False):
    """NII.normalize('standardization', lower, upper): the percentile clamp of nifti.normalize_scaling (np.percentile of the float32 copy, the
    upper percentile of the lower-clamped array), then the statement above.  A constant volume gives std32 == 0 and NaN everywhere (0 / 0), as
    numpy's expression does where its float32 mean of the constant is the constant."""
    v = np.asarray(v).astype(np.float32)
    if lower is not None:
        q = np.percentile(v, lower); v[v < q] = q
    if upper is not None:
        q = np.percentile(v, upper); v[v > q] = q
    return standardize_clamped(v, None, None, return_moments)
