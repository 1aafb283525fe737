"""utils/render.py -- the 8-bit renderings of the evaluation sample images (utils/Evaluation.py:302-321, 501-507), stated in numpy: the
host statement the device ops of csrc/uad_render.hip (uad_render_minmax_u8, uad_render_heatmap, uad_render_overlay) are held to bit for bit,
and the path an engine without those ops takes.  Batches are [N,H,W] with any H, W >= 1; every function returns uint8.  Inputs are finite;
what a NaN gives is unspecified.

minmax_u8 restates the DOCUMENTED arithmetic of cv2.normalize(x, None, 0, 255, NORM_MINMAX) followed by astype('uint8')
(normalize_and_squeeze, :368).  OpenCV is not a dependency and this statement HAS NOT BEEN COMPARED WITH OPENCV'S OWN OUTPUT, which may fuse
the multiply-add of the per-pixel map (the caveat of utils/resize.py).

Stated deviation (sic list): the reference passes the TP / FP / FN overlay through cv2.normalize(tmp, None, 0, 255) with the
default norm type (NORM_L2) and alpha = 0, which by OpenCV's documentation scales every image to zero -- `_vis.png` would be black.
overlay_rgb writes uint8(clip(v, 0, 1) * 255) instead."""
import math
import os

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
JET_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jet_u8.txt')
_jet = None


def jet_u8():
    """np.uint8(matplotlib.cm.jet(np.arange(256)) * 255) as committed data ([256,4] uint8; utils/jet_u8.txt, one "R G B A" row per index;
    tests/golden/jet_u8.npy is the same table and tests/test_render_host.py regenerates it from the installed matplotlib): nothing here needs
    matplotlib at run time."""
    global _jet
    if _jet is None:
        t = np.loadtxt(JET_PATH, dtype=np.int64, comments='#')
        assert t.shape == (256, 4) and t.min() >= 0 and t.max() <= 255
        _jet = t.astype(np.uint8)
    return _jet


def _batch(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    if a.ndim != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f'a batch must be [N,H,W] with H, W >= 1, got {a.shape}')
    return a


def _trunc_u8(v):
    """float32 -> uint8: truncated toward zero, clamped to 0 .. 255."""
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def minmax_u8(x):
    """normalize_and_squeeze (:368) per slice: smin, smax of the fp32 slice; in fp64 scale = 255 / (smax - smin) if smax - smin > DBL_EPSILON
    else 0 and shift = -smin * scale; per pixel in fp32, two roundings (no fused multiply-add): v = fl32(fl32(x * fl32(scale)) + fl32(shift));
    the output is v truncated toward zero and clamped to 0 .. 255.  A constant slice gives zeros."""
    x = _batch(x, np.float32)
    out = np.empty(x.shape, np.uint8)
    for k, s in enumerate(x):
        smin, smax = float(s.min()), float(s.max())
        diff = smax - smin
        scale = 255.0 / diff if diff > DBL_EPSILON else 0.0
        shift = -smin * scale
        v = (s * np.float32(scale)).astype(np.float32) + np.float32(shift)
        out[k] = _trunc_u8(v.astype(np.float32))
    return out


def label_u8(g):
    """`_gt.png` (:304): minmax_u8 of the label map cast to fp32."""
    return minmax_u8(np.asarray(g).astype(np.float32))


def _exp(t):
    """exp of a float64 array through math.exp -- the C library's exp, which the host build of the kernel source calls too (np.exp has
    vectorised loops of its own on some CPUs that may differ from it in the last place); evaluated once per distinct value."""
    def one(v):
        try:
            return math.exp(v)
        except OverflowError:               # the C function returns +inf
            return math.inf
    u, inv = np.unique(t, return_inverse=True)
    return np.array([one(v) for v in u.tolist()], np.float64)[inv].reshape(t.shape)


def heatmap_q256(d):
    """q * 256 of heatmap_index in fp64, [N,H,W]: in fp64 from the fp32 residual q = 2 * (1 / (1 + exp(-100 d)) - 0.5) (squash_intensities,
    :70-74), the colour bar q[i, W-1] = i / H (add_colorbar), q -= q.min(), q /= q.max() unless that is 0 (utils.apply_colormap,
    utils/utils.py:21-26).  The multiply by 256 is exact."""
    d = _batch(d, np.float32)
    n, h, w = d.shape
    out = np.empty(d.shape, np.float64)
    bar = np.arange(h, dtype=np.float64) / float(h)
    for k in range(n):
        t = -100.0 * d[k].astype(np.float64)
        q = 2.0 * (1.0 / (1.0 + _exp(t)) - 0.5)
        q[:, w - 1] = bar
        q = q - q.min()
        m = q.max()
        if m != 0:
            q = q / m
        out[k] = q * 256.0
    return out


def heatmap_index(d):
    """The colour index of heatmap_rgba, [N,H,W] uint8: min(int(q * 256), 255) of heatmap_q256 (matplotlib's Colormap.__call__ with N = 256)."""
    return np.minimum(heatmap_q256(d).astype(np.int64), 255).astype(np.uint8)


def heatmap_rgba(d, lut=None):
    """`_heatmap.png` (:319-321): lut[heatmap_index(d)] -> [N,H,W,4].  lut: any [256,4] uint8 table; None = the committed jet table."""
    lut = jet_u8() if lut is None else np.ascontiguousarray(lut, np.uint8)
    if lut.shape != (256, 4):
        raise ValueError(f'lut must be [256,4] uint8, got {lut.shape}')
    return lut[heatmap_index(d)]


def overlay_rgb(x, pred, gt):
    """image_utils.augment_prediction_and_groundtruth_to_image (utils/image_utils.py:22-45) -> [N,H,W,3]: the grey image on three channels with
    negatives set to 0; where pred | gt the colour of TP (0, 1, 0), FP (1, 0.5, 0) or FN (1, 0, 0); then uint8(clip(v, 0, 1) * 255) in fp32,
    truncated (0.5 -> 127) -- not the reference's cv2.normalize(tmp, None, 0, 255), see the module docstring."""
    x = _batch(x, np.float32)
    p = np.asarray(pred).astype(bool).reshape(x.shape)
    g = np.asarray(gt).astype(bool).reshape(x.shape)
    v = np.repeat(np.where(x < 0, np.float32(0), x)[..., None], 3, axis=3)
    v[p & g] = (0.0, 1.0, 0.0)
    v[p & ~g] = (1.0, 0.5, 0.0)
    v[~p & g] = (1.0, 0.0, 0.0)
    return _trunc_u8((np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.float32))
