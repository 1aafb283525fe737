"""Bilinear and nearest-neighbour resize of slices: the host statement of the two `cv2.resize` calls the reference's BrainWeb loader makes
when a slice is larger than `sliceResolution` (dataloaders/BRAINWEB.py:140-142: the default INTER_LINEAR for the image, INTER_NEAREST for
the label map).

OpenCV is not a dependency of this project: the arithmetic below restates OpenCV 4.2's `resize.cpp` for float32 input (`resize()`'s table
set-up for INTER_LINEAR, `resizeNN`), and it HAS NOT BEEN COMPARED WITH OPENCV'S OWN OUTPUT.  OpenCV's SIMD row and column passes (`HResizeLinear`, `VResizeLinear` with their vector branches) may
fuse a multiply-add or order the two products differently, so even a correct restatement can differ from a given OpenCV build in the last
bit.  What it was checked against: torch.nn.functional.interpolate in fp64 (`bilinear`, align_corners=False -- the same half-pixel
coordinate rule; `nearest` where the fp64 index equals the integer formula) and a scalar, loop-written restatement of both functions
(tests/test_resize_host.py); the device kernel (csrc/uad_resize.hip, device_ops.DeviceOps.resize) is held to this module bit for bit.

Per axis, with src -> dst samples:

    scale = 1.0 / (float64(dst) / float64(src))                  (OpenCV inverts inv_scale = dst / src; this is not src / dst)

INTER_LINEAR
    f  = float32((d + 0.5) * scale - 0.5)                        (fp64, rounded once)
    s  = floor(f);  f = f - float32(s)                           (fp32)
    s < 0         ->  s = 0,       f = 0
    s >= src - 1  ->  s = src - 1, f = 0
    taps s and min(s + 1, src - 1) with weights float32(1) - f and f
    horizontal pass first:  t = a[s0] * w0 + a[s1] * w1, then the vertical pass on t; every multiply and add is one fp32 operation, none
    is fused (numpy has no fused multiply-add)

INTER_NEAREST
    s = min(floor(d * scale), src - 1) in fp64.  This is NOT d * src // dst: for 22 -> 18, d = 9 gives 9 * (1 / (18 / 22)) =
    10.999999999999998 -> 10 where the integer formula says 11 (and for 14 -> 18, d = 9 reads 6, not 7).  Values are copied, bits kept."""
import numpy as np


def _scale(src, dst):
    return np.float64(1.0) / (np.float64(dst) / np.float64(src))


def linear_table(src, dst):
    """-> (s0 int64 [dst], s1 int64 [dst], w0 float32 [dst], w1 float32 [dst]): the taps and weights of one axis (BRAINWEB.py:141)."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * _scale(src, dst) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), np.float32(1) - f, f


def nearest_table(src, dst):
    """-> int64 [dst]: the source index of every output sample of one axis (BRAINWEB.py:142)."""
    d = np.arange(dst, dtype=np.float64)
    return np.minimum(np.floor(d * _scale(src, dst)), np.float64(src - 1)).astype(np.int64)


def _check(a, out_hw):
    a = np.asarray(a, np.float32)
    H, W = (int(v) for v in out_hw)
    if a.ndim < 2 or a.shape[-2] < 1 or a.shape[-1] < 1 or H < 1 or W < 1:
        raise ValueError(f'resize takes [..., h, w] with h, w >= 1 and an output (H, W) >= 1, got {a.shape} -> {(H, W)}')
    return a, H, W


def resize_linear(a, out_hw):
    """cv2.resize(a, (W, H)) (INTER_LINEAR) of float32 [..., h, w] -> float32 [..., H, W] as OpenCV 4.2's resize.cpp states it
    (dataloaders/BRAINWEB.py:141).  Not compared with OpenCV's own output, whose SIMD paths may fuse or reorder the multiply-adds; checked
    against torch's fp64 bilinear interpolation within the rounding derived in tests/test_resize_host.py and, bit for bit, against a scalar
    restatement."""
    a, H, W = _check(a, out_hw)
    x0, x1, wx0, wx1 = linear_table(a.shape[-1], W)
    y0, y1, wy0, wy1 = linear_table(a.shape[-2], H)
    t = a[..., :, x0] * wx0 + a[..., :, x1] * wx1                     # horizontal pass, [..., h, W]
    return t[..., y0, :] * wy0[:, None] + t[..., y1, :] * wy1[:, None]


def resize_nearest(a, out_hw):
    """cv2.resize(a, (W, H), interpolation=cv2.INTER_NEAREST) of float32 [..., h, w] -> float32 [..., H, W] (dataloaders/BRAINWEB.py:142):
    the fp64 index min(floor(d * scale), src - 1), which is not d * src // dst (22 -> 18: output 9 reads input 10).  Not compared with
    OpenCV's own output; checked against torch's 'nearest' where the two index rules agree and against a scalar restatement."""
    a, H, W = _check(a, out_hw)
    return a[..., nearest_table(a.shape[-2], H), :][..., :, nearest_table(a.shape[-1], W)]
