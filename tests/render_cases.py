"""Shapes, inputs and host-statement references shared by tests/test_render_kernels_host.py (the kernel source compiled for the host) and
tests/test_gpu_render.py (the device ops): built once per process, never written to.

Shapes.  The kernels of csrc/uad_render.hip give a thread quads of four pixels; a workgroup of the small path is 256 threads (one pass
= a tile of 1024 pixels) and keeps up to 16384 pixels (128 x 128) in registers, the large path (1024 threads) up to 65536 (256 x 256), larger
slices are read twice.  So: 1 pixel; 5 x 7 (nothing divisible by four); the tile at -1 / 0 / +1; the last slice of each path and one pixel
more.  n: 1, 3 and -- on 5 x 7 -- 1025, one more than the 1024 workgroups a launch has."""
import functools

import numpy as np

from unsupervised_anomaly_detection_brain_mri_amd.utils import render

TILE = 1024
SMALL_HW, LARGE_HW, MAX_GRID = 16384, 65536, 1024
SHAPES = [(1, 1), (5, 7), (33, 31), (32, 32), (25, 41), (128, 128), (113, 145), (256, 256), (1, 65537), (256, 260), (9, 1)]
assert [h * w for h, w in SHAPES[2:9]] == [TILE - 1, TILE, TILE + 1, SMALL_HW, SMALL_HW + 1, LARGE_HW, LARGE_HW + 1]
N_FOLD = MAX_GRID + 1
CASES = [(n, hw) for hw in SHAPES for n in ((1, 3) if hw[0] * hw[1] <= SMALL_HW + 1 else (1,))] + [(N_FOLD, (5, 7))]
GREY_KINDS = ('uniform', 'constant', 'negative', 'tiny')
HEAT_KINDS = ('lesions', 'zeros')

# a colour table that gives the index back (channel 0) and tells the channels apart
INDEX_LUT = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) & 255, np.full(256, 255)], axis=1).astype(np.uint8)


def case_id(case):
    n, (h, w) = case
    return f'{n}x{h}x{w}'


def _rng(*key):
    return np.random.default_rng([17, *key])


@functools.lru_cache(maxsize=None)
def grey_input(n, hw, kind):
    """uniform: [-0.2, 1.3) (negative values, values past 1); constant: one value per slice; negative: all below zero; tiny: smax - smin is
    below DBL_EPSILON in fp64 but not zero in fp32."""
    h, w = hw
    rng = _rng(n, h, w, GREY_KINDS.index(kind))
    if kind == 'uniform':
        a = rng.random((n, h, w), np.float32) * np.float32(1.5) - np.float32(0.2)
    elif kind == 'constant':
        a = np.broadcast_to(rng.random((n, 1, 1), np.float32) + np.float32(0.25), (n, h, w)).copy()
    elif kind == 'negative':
        a = -rng.random((n, h, w), np.float32) - np.float32(0.5)
    else:
        a = (rng.integers(1, 3, (n, h, w)) * 1e-20).astype(np.float32)
        if h * w > 1:
            a.reshape(n, -1)[:, 0], a.reshape(n, -1)[:, 1] = np.float32(1e-20), np.float32(2e-20)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def grey_reference(n, hw, kind):
    r = render.minmax_u8(grey_input(n, hw, kind))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def heat_input(n, hw, kind):
    """lesions: residuals drawn uniformly from [0, 0.05] on a quarter of the pixels over a zero background (the squash does not saturate);
    zeros: exactly 0 everywhere, the heat map is only the colour bar."""
    h, w = hw
    rng = _rng(n, h, w, 7 + HEAT_KINDS.index(kind))
    a = np.zeros((n, h, w), np.float32)
    if kind == 'lesions':
        a = np.where(rng.random((n, h, w)) < 0.25, rng.random((n, h, w), np.float32) * np.float32(0.05), np.float32(0)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def heat_q256(n, hw, kind):
    r = render.heatmap_q256(heat_input(n, hw, kind))
    r.setflags(write=False)
    return r


def heat_reference_index(n, hw, kind):
    return np.minimum(heat_q256(n, hw, kind).astype(np.int64), 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def overlay_input(n, hw):
    """x in [-0.3, 1.4) with exact 0, 0.5 and 1 among the values; pred (fp32 0 / 1) and gt (bool) cover TP, FP, FN and neither."""
    h, w = hw
    rng = _rng(n, h, w, 31)
    x = rng.random((n, h, w), np.float32) * np.float32(1.7) - np.float32(0.3)
    flat = x.reshape(-1)
    flat[::5] = np.float32(0.5); flat[1::11] = np.float32(1.0); flat[2::13] = np.float32(0.0)
    pred = (rng.random((n, h, w)) < 0.3).astype(np.float32)
    gt = rng.random((n, h, w)) < 0.3
    for a in (x, pred, gt):
        a.setflags(write=False)
    return x, pred, gt


@functools.lru_cache(maxsize=None)
def overlay_reference(n, hw):
    r = render.overlay_rgb(*overlay_input(n, hw))
    r.setflags(write=False)
    return r


EXEMPT_WINDOW = 1e-9        # a one-ulp exp difference moves q * 256 by about 1e-13: derived, not measured
EXEMPT_CAP = 1e-3           # at most 0.1 % of a test's pixels


def heat_mismatch(got_index, q256):
    """(pixels that differ from the statement's index, of those the ones the exemption does not cover): a pixel may differ only where the
    statement's fp64 q * 256 lies within EXEMPT_WINDOW of an integer, and then by one index."""
    ref = np.minimum(q256.astype(np.int64), 255)
    got = got_index.astype(np.int64)
    bad = got != ref
    near = np.abs(q256 - np.rint(q256)) <= EXEMPT_WINDOW
    covered = bad & near & (np.abs(got - ref) == 1)
    return int(bad.sum()), int((bad & ~covered).sum())
