"""Shared cases of the order-statistic tests (tests/test_select_host.py, tests/test_gpu_select.py): value generators, a numpy MODEL of the
device ops' contract (include/uad_hip.h: uad_select_quantiles -- m, lo, hi from a sort --, uad_histogram_edges, uad_clamp_scale) and a
stand-in engine built from it.  The reference everywhere is the installed numpy (np.percentile / np.quantile / np.histogram)."""
import numpy as np
import scipy.ndimage
import torch

from unsupervised_anomaly_detection_brain_mri_amd.utils.order_stats import OrderStatOps, as_float32_exact

QS = (0.0, 0.5, 0.9, 0.998, 1.0, 0.25)        # 0.25: an integer virtual index at n = 5 and n = 39 277 ((n - 1) / 4 = 1, 9 819)
HOST_SIZES = (1, 2, 3, 5, 39277)
DENORM = np.float32(1.4e-45)                  # the smallest float32 denormal


def values(kind, n, seed=0):
    """float32 test vectors of n values.  Every kind is NaN-free (the op's precondition)."""
    rng = np.random.default_rng(seed + 7919 * n)
    if kind == 'distinct':
        return rng.permutation(np.arange(n, dtype=np.float32) * np.float32(0.37) - np.float32(0.11 * n))
    if kind == 'random':
        return rng.standard_normal(n).astype(np.float32)
    if kind == 'equal':
        return np.full(n, 0.7310586, np.float32)
    if kind == 'two':
        return np.where(rng.random(n) < 0.3, np.float32(0.25), np.float32(0.75)).astype(np.float32)
    if kind == 'denormal':
        return (rng.integers(-40, 40, n).astype(np.float32) * DENORM).astype(np.float32)
    if kind == 'zeros':                          # -0 / +0 mixed with a few values on both sides
        return rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.5, 2.5], np.float32), n).astype(np.float32)
    if kind == 'low_byte':                       # keys that differ in the lowest byte only: the first three passes see one digit
        return (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == 'high_byte':                      # keys that differ in the highest byte only (both signs; low 24 bits fixed; no overflow in b - a)
        top = rng.choice(np.array([0x3d, 0x3e, 0x3f, 0x40, 0x41, 0x42, 0xbe, 0xbf, 0xc0, 0xc1], np.uint32), n)
        return ((top << np.uint32(24)) | np.uint32(0x00345678)).astype(np.uint32).view(np.float32)
    if kind == 'inf':                            # +-inf at the ends, two of each: brackets away from the extremes stay finite
        v = rng.standard_normal(n).astype(np.float32)
        if n >= 16:
            v[:2], v[2:4] = -np.inf, np.inf
        return rng.permutation(v)
    raise KeyError(kind)


HOST_KINDS = ('distinct', 'equal', 'two', 'denormal', 'zeros')
GPU_KINDS = ('distinct', 'random', 'equal', 'two', 'denormal', 'zeros', 'low_byte', 'high_byte')


def bracket_indices(m, q, f32):
    """The two sorted-array indices of the op's contract: floor(v) and min(floor(v) + 1, m - 1) for v = (m - 1) * q, formed -- one multiply -- in
    float32 where numpy forms it in float32, else float64."""
    ft = np.float32 if f32 else np.float64
    last = ft(m - 1)
    v = last * ft(q)
    if v >= last:
        return m - 1, m - 1
    p = np.floor(v)
    return min(max(int(p), 0), m - 1), min(max(int(p + ft(1)), 0), m - 1)


def model_select(vals, fractions, f32_index, segments=None, nonneg_only=False):
    """(m [n_seg] int64, lo [n_seg,k] float32, hi [n_seg,k] float32) from one sort per segment."""
    a = as_float32_exact(np.asarray(vals)).reshape(1 if segments is None else int(segments), -1)
    k = len(fractions)
    m = np.zeros(a.shape[0], np.int64)
    lo, hi = np.full((a.shape[0], k), np.nan, np.float32), np.full((a.shape[0], k), np.nan, np.float32)
    for s, row in enumerate(a):
        x = np.sort(row[row >= 0] if nonneg_only else row)
        m[s] = x.size
        for j in range(k if x.size else 0):
            p, nx = bracket_indices(x.size, fractions[j], f32_index[j])
            lo[s, j], hi[s, j] = x[p], x[nx]
    return m, lo, hi


def model_histogram_edges(vals, edges32):
    """counts[i] = #(e[i] <= v < e[i+1]), last bin closed, outside dropped -- by direct comparison against every edge."""
    v = as_float32_exact(np.asarray(vals)).reshape(-1)
    e = np.asarray(edges32, np.float32)
    bins = e.size - 1
    inside = (v >= e[0]) & (v <= e[-1])
    idx = (v[inside][:, None] >= e[None, :bins]).sum(1) - 1
    return np.bincount(idx, minlength=bins).astype(np.int64)


class ModelEngine(OrderStatOps):
    """Stand-in engine: the raw ops from the numpy model, quantile / percentile / histogram from the package's own OrderStatOps (the wrapper's
    interpolation), `zoom` from scipy.  'Device' arrays are CPU torch tensors, as in the other host stand-ins."""
    device = torch.device('cpu')

    def __init__(self):
        self.calls = []

    def _dev(self, a):
        return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))

    def select_quantiles(self, vals, fractions, f32_index, segments=None, nonneg_only=False):
        self.calls.append(('select', len(fractions), segments))
        return model_select(np.asarray(vals), fractions, f32_index, segments, nonneg_only)

    def histogram_edges(self, vals, edges32):
        self.calls.append(('histogram', len(edges32) - 1))
        return model_histogram_edges(np.asarray(vals), edges32)

    def clamp_scale(self, vals, lo=None, hi=None, scale=1.0, out=None):
        self.calls.append(('clamp_scale',))
        v = np.array(self._dev(vals).numpy(), np.float32)
        if lo is not None:
            v[v < np.float32(lo)] = np.float32(lo)
        if hi is not None:
            v[v > np.float32(hi)] = np.float32(hi)
        return torch.from_numpy(v * np.float32(scale))

    def zoom(self, slices, out_hw, mode='constant', integer=False):
        s = slices.numpy() if isinstance(slices, torch.Tensor) else np.asarray(slices)
        self.calls.append(('zoom', isinstance(slices, torch.Tensor), mode))
        zf = (out_hw[0] / s.shape[1], out_hw[1] / s.shape[2])
        out = np.stack([scipy.ndimage.zoom(a.astype(np.float64), zf, mode=mode) for a in s])
        return torch.from_numpy(out.astype(np.float32))


def phantom(shape=(12, 37, 29), seed=3):
    """(volume, label, brain mask) [z,y,x]: an ellipsoid 'brain' whose axial extent leaves slices on both sides of the 0.2 empty-slice filter,
    smooth tissue contrast plus noise, negative values outside the mask (they become -0 under skull stripping) and a bright 'lesion'."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij')
    r = np.sqrt((z / 0.75) ** 2 + (y / 0.85) ** 2 + (x / 0.8) ** 2)
    mask = (r < 1.0).astype(np.float64)
    vol = 600.0 * np.clip(1.15 - r, 0, None) + 40.0 * rng.standard_normal(shape)
    vol[r >= 1.0] = -5.0 + rng.standard_normal(shape)[r >= 1.0]
    lesion = ((z - 0.1) ** 2 + (y + 0.2) ** 2 + (x - 0.15) ** 2) < 0.03
    vol[lesion] += 900.0
    return vol, lesion.astype(np.float64), mask
