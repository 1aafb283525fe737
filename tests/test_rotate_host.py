"""CPU: the semantics the device rotation (uad_affine_spline3) restates, pinned on scipy without a GPU.

tests/rotate_cases.py holds a numpy restatement of scipy.ndimage.rotate(reshape=False, order=3) as an affine_transform in both modes; it is
held to scipy at 1e-13 here.  The two traps of mode 'nearest' are each shown by a case that fails under the wrong rule: tap indices beyond
the 12-sample padding are CLAMPED, not mirrored, and the prefilter of the padded line starts from scipy's REFLECT initial values, not the
mirror ones the zoom path uses.  Also: the horizon at which the kernels cut the reflect sum, the C-ABI entries in header / ctypes table /
library with the refusals that need no device, and nifti.volume_to_slices' routing (host stand-in engines keep the scipy loop)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch

from tests import rotate_cases as rc
from unsupervised_anomaly_detection_brain_mri_amd import _lib
from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTATEMENT_BAR = 1e-13
SHAPES = rc.SHAPES + [(40, 40), (2, 9)]


def _plane(h, w):
    return np.random.default_rng(100 * h + w).random((h, w)).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize('mode', rc.MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_restatement_against_scipy_rotate(shape, mode):
    a = _plane(*shape)
    for angle in rc.ANGLES:
        m, off = rc.rotation_transform(angle, shape)
        ref = rc.scipy_rotate(a, angle, mode)
        np.testing.assert_array_equal(ref, scipy.ndimage.affine_transform(a, m, off, shape, order=3, mode=mode))    # rotate IS this call
        err = float(np.abs(rc.affine_restated(a, m, off, mode=mode) - ref).max())
        assert err <= RESTATEMENT_BAR, (angle, err)


def test_right_angles_have_an_exact_matrix():
    for angle, want in ((90, [[0, 1], [-1, 0]]), (180, [[-1, 0], [0, -1]]), (-90, [[0, -1], [1, 0]])):
        m, _ = rc.rotation_transform(angle, (33, 57))
        np.testing.assert_array_equal(m, np.array(want, np.float64))


def test_general_affine_with_another_output_shape():
    a = _plane(33, 57)
    m = np.array([[0.9, 0.2], [-0.1, 1.3]])
    off = np.array([1.5, -2.25])
    for mode in rc.MODES:
        ref = scipy.ndimage.affine_transform(a, m, off, (40, 29), order=3, mode=mode)
        assert np.abs(rc.affine_restated(a, m, off, (40, 29), mode=mode) - ref).max() <= RESTATEMENT_BAR


def test_offset_is_added_after_the_matrix_sum():
    """(Y m00 + X m01) + off0 is scipy's order; with the offset first the coordinate differs in the last bits at some pixel."""
    m, off = rc.rotation_transform(37.5, (128, 128))
    cy, _ = rc.coordinates(m, off, (128, 128))
    Y, X = np.meshgrid(np.arange(128.0), np.arange(128.0), indexing='ij')
    assert np.count_nonzero((off[0] + Y * m[0, 0]) + X * m[0, 1] != cy) > 0


def test_trap_taps_beyond_the_padding_are_clamped_not_mirrored():
    a = _plane(128, 128)
    m, off = rc.rotation_transform(37.5, a.shape)
    assert rc.beyond_padding(m, off, a.shape) > 0
    ref = rc.scipy_rotate(a, 37.5, 'nearest')
    assert np.abs(rc.affine_restated(a, m, off, mode='nearest') - ref).max() <= RESTATEMENT_BAR
    assert np.abs(rc.affine_restated(a, m, off, mode='nearest', nearest_taps='mirror') - ref).max() > 0.1
    # without a pixel beyond the padding the two rules agree: the trap only shows on such a case
    m, off = rc.rotation_transform(-10, a.shape)
    assert rc.beyond_padding(m, off, a.shape) == 0
    np.testing.assert_array_equal(rc.affine_restated(a, m, off, mode='nearest'), rc.affine_restated(a, m, off, mode='nearest', nearest_taps='mirror'))


def test_trap_the_padded_line_is_filtered_with_the_reflect_initial_values():
    for n in (26, 29, 48, 49, 81, 152, 241):
        line = np.random.default_rng(n).random(n)
        ref = scipy.ndimage.spline_filter1d(line, order=3, mode='nearest')
        assert np.abs(rc.prefilter_line(line, 'reflect') - ref).max() <= 2e-15 * 6
        assert np.abs(rc.prefilter_line(line, 'mirror') - ref).max() > 1e-3             # the ends of the line differ
        np.testing.assert_allclose(rc.prefilter_line(line, 'mirror'), scipy.ndimage.spline_filter1d(line, order=3, mode='mirror'), rtol=0, atol=2e-15 * 6)
    a = _plane(128, 128)
    m, off = rc.rotation_transform(37.5, a.shape)
    ref = rc.scipy_rotate(a, 37.5, 'nearest')
    err = float(np.abs(rc.affine_restated(a, m, off, mode='nearest', nearest_init='mirror') - ref).max())
    assert 1e-8 < err < 1e-6            # far above the restatement's 1e-13, and too much beside the final fp32 rounding under the 1.2e-7 bar


def test_reflect_sum_may_stop_at_the_horizon():
    """The kernels cut the causal initial sum of a line longer than 48 samples after 48 terms: the rest is below fp64 round-off of the sum."""
    horizon, z = 48, rc.POLE
    assert abs(z) ** horizon < 1e-27
    for n in (49, 64, 152, 241):
        c = np.random.default_rng(n).random(n) * 6.0
        zn = z ** n
        full = c[0] + (z / (1 - zn * zn)) * np.sum(z ** np.arange(n) * (c + zn * c[::-1]))
        cut = c[0] + z * np.sum(z ** np.arange(horizon) * c[:horizon])
        assert abs(full - cut) <= 2 * np.finfo(np.float64).eps * abs(full)
        # worst case over inputs in [0, 6]: the dropped tail is bounded by 6 |z|^48 / (1 - |z|)
        assert 6 * abs(z) ** horizon / (1 - abs(z)) < 1e-26


def test_integer_inputs_of_the_gpu_test_have_no_rounding_tie():
    m, un, want = rc.integer_reference(1, 33, 57, 'nearest')
    assert rc.near_ties(un) == 0
    np.testing.assert_array_equal(rc.round_half_away(un), want)          # scipy's integer output is the spline rounded half away from zero


def test_the_two_entries_are_declared_bound_and_exported():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'uad_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(uad_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('uad_affine_spline3_workspace', 'uad_affine_spline3'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SYMBOLS[name]
    ws = lib.uad_affine_spline3_workspace
    assert ws(110, 128, 128, _lib.ZOOM_CONSTANT) == 110 * 128 * 128 * 8
    assert ws(110, 128, 128, _lib.ZOOM_NEAREST) == 110 * (128 + 24) * (128 + 24) * 8
    assert _lib.AFFINE_MAX_K == 16


def test_bad_arguments_are_refused_before_any_device_work():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.uad_affine_spline3
    fn.restype, fn.argtypes = _lib.SYMBOLS['uad_affine_spline3']
    xf = (ctypes.c_double * (6 * 17))(*([1, 0, 0, 1, 0, 0] * 17))
    p = ctypes.c_void_p(4096)                    # never dereferenced: every call below is refused on its arguments
    big = 1 << 40

    def call(n=1, h=8, w=8, H=8, W=8, K=1, boundary=0, out_kind=0, ws=p, nbytes=big):
        return fn(p, n, h, w, H, W, xf, K, boundary, out_kind, p, ws, nbytes, None)
    invalid, unsupported = 1, 3                  # UAD_ERR_INVALID, UAD_ERR_UNSUPPORTED: the zoom op's codes (ValueError in _lib.check)
    assert call(h=1) == invalid and call(w=1) == invalid
    assert call(K=0) == invalid and call(K=17) == invalid
    assert call(boundary=2) == invalid and call(out_kind=2) == invalid
    assert call(nbytes=8 * 8 * 8 - 1) == invalid
    assert call(ws=ctypes.c_void_p(4096 + 8)) == invalid
    assert call(n=1 << 20, h=4096, w=8) == unsupported
    assert call(H=1 << 16, W=1 << 16) == unsupported


class _HostZoomEngine:
    """A host stand-in with the zoom op only (tests/test_resample_host.py: ZoomingHostEngine): no `rotate`, so the scipy loop must stay."""
    device = torch.device('cpu')

    def zoom(self, slices, out_hw, mode='constant', integer=False):
        s = slices.numpy() if isinstance(slices, torch.Tensor) else np.asarray(slices)
        zf = (out_hw[0] / s.shape[1], out_hw[1] / s.shape[2])
        return torch.from_numpy(np.stack([scipy.ndimage.zoom(a.astype(np.float64), zf, mode=mode) for a in s]).astype(np.float32))


class _HostRotateEngine(_HostZoomEngine):
    """... plus a scipy-backed `rotate` with device_ops.DeviceOps.rotate's signature that records its calls."""

    def __init__(self):
        self.calls = []

    def rotate(self, slices, angles, mode='constant', integer=False):
        s = slices.numpy() if isinstance(slices, torch.Tensor) else np.asarray(slices)
        self.calls.append((tuple(s.shape), tuple(angles), mode, integer))
        out = np.stack([np.stack([rc.scipy_rotate(a.astype(np.float64), ang, mode) for ang in angles]) for a in s])
        return torch.from_numpy(out.astype(np.float32))


def _volume():
    rng = np.random.default_rng(4)
    vol = np.clip(scipy.ndimage.gaussian_filter(rng.random((12, 50, 45)), 2.0) * 2.0, 0, None)
    seg = (scipy.ndimage.gaussian_filter(rng.standard_normal((12, 50, 45)), 3.0) > 0.02).astype(np.float64)
    return vol, seg


def test_volume_to_slices_routes_the_rotations_through_an_engine_that_has_rotate():
    vol, seg = _volume()
    kw = dict(slice_start=1, slice_end=11, slice_resolution=(32, 32), skull_stripping=False, empty_thresh=0.0, rotations=(0, 15, -10), center_crop=(24, 20))
    plain = _HostZoomEngine()
    im_h, lb_h, kept_h = nifti.volume_to_slices(vol, seg, engine=plain, **kw)            # no rotate op: the scipy loop, untouched
    eng = _HostRotateEngine()
    im_d, lb_d, kept_d = nifti.volume_to_slices(vol, seg, engine=eng, **kw)
    n = len(kept_h) // 3
    assert eng.calls == [((n, 32, 29), (15, -10), 'constant', False), ((n, 32, 29), (15, -10), 'nearest', False)]     # angle 0 is skipped by the caller
    assert kept_d == kept_h and kept_h[:4] == [kept_h[0]] * 3 + [kept_h[3]]              # slice-major, angle-minor
    assert im_d.shape == im_h.shape == (3 * n, 20, 24) and im_d.dtype == im_h.dtype == np.float32 and lb_d.dtype == lb_h.dtype == np.float32
    assert np.abs(im_d.astype(np.float64) - im_h).max() <= rc.F32_BAR and np.abs(lb_d.astype(np.float64) - lb_h).max() <= rc.F32_BAR
    np.testing.assert_array_equal(im_d[0::3], im_h[0::3])                                # the 0-degree entries pass through
    eng.calls.clear()
    im_o, _, _ = nifti.volume_to_slices(vol, seg, engine=eng, device_rotate=False, **kw)
    assert eng.calls == []
    np.testing.assert_array_equal(im_o, im_h)
    with pytest.raises(ValueError):
        nifti.volume_to_slices(vol, seg, engine=plain, device_rotate=True, **kw)
    eng.calls.clear()
    nifti.volume_to_slices(vol, seg, engine=eng, **dict(kw, rotations=(0,)))
    assert eng.calls == []                                                               # nothing to rotate: the op is not called
