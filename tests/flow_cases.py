"""Shared by tests/test_flow_kernels_host.py (CPU, the kernel source compiled for the host) and tests/test_gpu_flow.py (the device): the
volumes the curvature-flow kernel is held on and their reference -- always the host statement utils/curvature_flow.py, which
tests/test_flow_host.py pins on hand-derived cases and on an independent scalar re-statement.  Computed once per case and cached; callers
must not write into what they get.

Shapes [nz, ny, nx]: a single voxel, a line, sizes below one tile, and every tile edge of csrc/uad_flow.hip at -1, 0, +1 -- FLOW_TX = 32
along x (31, 32, 33 and 64, 65: two and three tiles), FLOW_TY = 8 along y (7, 8, 9 and 15, 16, 17), FLOW_ZC = 16 planes along z (15, 16,
17 and 33, 65: up to five chunks)."""
import functools

import numpy as np

from unsupervised_anomaly_detection_brain_mri_amd.utils.curvature_flow import curvature_flow

SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 4), (3, 7, 9), (5, 8, 32), (4, 9, 33), (9, 15, 31), (17, 17, 65), (33, 16, 64), (3, 65, 17), (65, 5, 6),
          (15, 9, 33), (16, 7, 31)]         # the last two: FLOW_ZC - 1 and FLOW_ZC planes, which the issue's list leaves out
SPACINGS = [(1.0, 1.0, 1.0), (0.9, 1.1, 3.0)]
ITERATIONS = [1, 3]
TIME_STEP = 0.125


@functools.lru_cache(maxsize=None)
def volume(shape):
    """Random uniform fp64 in [0, 1)."""
    v = np.random.default_rng(1000003 * shape[0] + 1009 * shape[1] + shape[2]).random(shape)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def volume_f32(shape):
    v = volume(shape).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def half_constant():
    """9 x 15 x 40: constant for x < 20, random beyond -- the gate (|grad|^2 < 1e-9 -> no update) is taken inside a tile, by some lanes of a wave."""
    v = np.random.default_rng(77).random((9, 15, 40))
    v[:, :, :20] = 0.375
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(shape, spacing, iterations, f32=False):
    """The host statement on volume(shape) (f32: on the fp32-rounded volume, widened exactly)."""
    src = volume_f32(shape) if f32 else volume(shape)
    r = curvature_flow(src, spacing, TIME_STEP, iterations)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def half_constant_reference(spacing, iterations):
    r = curvature_flow(half_constant(), spacing, TIME_STEP, iterations)
    r.setflags(write=False)
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
