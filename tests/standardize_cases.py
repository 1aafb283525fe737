"""Shared cases of the standardization tests (tests/test_standardize_host.py, test_standardize_kernels_host.py, test_standardize_pipeline_host.py,
test_gpu_standardize.py): sizes on the edges of the summation order, inputs, the phantom volumes of both loaders, and the error bound of
DESIGN §25 that holds the statement and numpy's float32 expression to the same expression in fp64."""
import math

import numpy as np

from tests.select_cases import phantom
from unsupervised_anomaly_detection_brain_mri_amd.utils import standardize as st

T = st.TILE                                                # include/uad_hip.h: UAD_SELECT_TILE
# a run (32), a tile (8192) and the partial pass's strided runs (256 tiles) from both sides
SIZES = (1, 2, 31, 32, 33, T - 1, T, T + 1, 256 * T - 1, 256 * T, 256 * T + 1)
GPU_SIZES = (1, 33, T - 1, T, T + 1, 256 * T + 1)
U32 = 2.0 ** -24                                           # unit roundoff of float32
U64 = 2.0 ** -53


def values(n, seed=0):
    """Intensity-like float32 values of both signs with a heavy upper tail."""
    rng = np.random.default_rng(seed + 104729 * (n % 9973))
    return (300.0 * rng.standard_normal(n) + 120.0 + 900.0 * (rng.random(n) < 0.01)).astype(np.float32)


def offset_values(n, seed=1):
    """A large offset and a small spread: 1e4 + 1e-2 * noise.  x^2 ~ 1e8 has a float32 spacing of 8 against a variance of 1e-4."""
    rng = np.random.default_rng(seed + n)
    return (1e4 + 1e-2 * rng.standard_normal(n)).astype(np.float32)


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def bound(v):
    """the largest |out_i - O_i| of an evaluation of `c = v - mean(v); c / std(c)` (std of the centred data, ddof 0) whose
    per-element arithmetic is float32 and whose three scalars (mean, mean of c, variance) each carry ONE float32 rounding -- 2^-24 times the
    mean of the absolute terms -- on top of the fp64 chain of the ordered sums.  O = the expression in fp64.  -> (O, bound per element)."""
    x = np.asarray(v, np.float64).reshape(-1)
    eps64 = st.SUM_CHAIN * U64
    C = x - x.mean()
    S = math.sqrt(np.mean(C * C))
    O = C / S
    cbar, cmax = np.mean(np.abs(C)), np.abs(C).max()
    em = (U32 + eps64) * np.mean(np.abs(x))                            # the mean
    dc = em + U32 * (np.abs(C) + em)                                          # |c_i - C_i|
    em2 = (U32 + eps64) * (cbar + em)                                 # the mean of c
    D = 2 * U32 * cmax + U32 * cbar + 2 * U32 * em + em2                      # |e_i - C_i|
    ev = (2 * cbar * D + D * D) / (S * S) + 2 * U32 * (1 + 2 * D / S) ** 2 + eps64        # the variance, relative
    assert ev < 0.5
    es = 1.0 - math.sqrt(1.0 - ev) * (1.0 - U32)                              # the standard deviation, relative
    return O, ((dc / S + np.abs(O) * es) / (1.0 - es)) * (1 + U32) + U32 * np.abs(O)


def numpy_float32(v, lower=None, upper=None):
    """The reference expression as numpy evaluates it in float32 (NII.py:53-75)."""
    v = np.array(v, np.float32)
    if lower is not None:
        q = np.percentile(v, lower); v[v < q] = q
    if upper is not None:
        q = np.percentile(v, upper); v[v > q] = q
    c = v - np.mean(v)
    with np.errstate(invalid='ignore', divide='ignore'):
        return v, c / np.std(c)


def mslub_phantom():
    """(volume, label, brain mask) of about 12 x 40 x 36."""
    return phantom((12, 40, 36), seed=5)


def brainweb_phantom():
    """(volume, tissue classes) of 12 x 40 x 36: background 0, a skull shell (class 7), grey matter 2, a lesion (10); a constant last slice."""
    vol, lesion, mask = phantom((12, 40, 36), seed=6)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in vol.shape], indexing='ij')
    r = np.sqrt((z / 0.75) ** 2 + (y / 0.85) ** 2 + (x / 0.8) ** 2)
    tissue = np.zeros(vol.shape, np.uint8)
    tissue[r < 1.0] = 7
    tissue[r < 0.9] = 2
    tissue[(lesion > 0) & (r < 0.9)] = 10
    vol = np.abs(vol)
    vol[-1] = 0.0
    tissue[-1] = 0
    return vol, tissue
