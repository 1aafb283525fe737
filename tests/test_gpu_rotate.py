"""GPU: the device cubic-spline rotation (uad_affine_spline3 through device_ops.DeviceOps.affine / rotate) and nifti.volume_to_slices' rotation
augmentation on it.

The reference is always scipy (ndimage.rotate / affine_transform) run in fp64 on the fp32-rounded input, never the code under test; inputs,
references and the host formula come from tests/rotate_cases.py, computed once and shared.  Bars (tests/test_gpu_resample.py):
  fp32 output: max-abs error <= 1.2e-7 with |ref| < 2 asserted -- fp64 arithmetic leaves about 1e-15, the final fp32 rounding half an ulp,
      6e-8 for |v| < 2; the bar is twice that.
  int32 output: exact equality with scipy's integer result, on inputs that have ZERO voxels whose unrounded value lies within 1e-9 of a
      half-integer (asserted, on scipy alone)."""
import os

import numpy as np
import pytest
import scipy.ndimage
import torch

from tests import rotate_cases as rc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps, rotation_transform
    from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti
except Exception:
    DeviceOps = None

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'zoom_parent_golden.npz')


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


@pytest.mark.parametrize('mode', rc.MODES)
@pytest.mark.parametrize('shape', rc.SHAPES, ids=lambda s: '%dx%d' % s)
def test_fp32_output_against_scipy_fp64(eng, shape, mode):
    h, w = shape
    for n in rc.BATCHES:
        a, ref = rc.float_reference(n, h, w, mode)
        got = eng.rotate(a.copy(), rc.ANGLES, mode=mode)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, len(rc.ANGLES), h, w)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max(axis=(0, 2, 3))
        print(f'rotate fp32 {shape} {mode} n={n}: max-abs err per angle {", ".join(f"{e:.3e}" for e in err)} (|ref| max {np.abs(ref).max():.3f})')
        assert np.abs(ref).max() < 2.0
        assert err.max() <= rc.F32_BAR


@pytest.mark.parametrize('mode', rc.MODES)
@pytest.mark.parametrize('shape', rc.SHAPES, ids=lambda s: '%dx%d' % s)
def test_int32_output_equals_scipy_on_integer_maps(eng, shape, mode):
    h, w = shape
    for n in rc.BATCHES:
        m, unrounded, want = rc.integer_reference(n, h, w, mode)
        assert rc.near_ties(unrounded) == 0                    # the condition on the inputs, on scipy alone
        assert np.issubdtype(want.dtype, np.integer)
        got = eng.rotate(m, rc.ANGLES, mode=mode, integer=True)
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
        wrong = int(np.count_nonzero(got.cpu().numpy() != want))
        print(f'rotate int32 {shape} {mode} n={n}: {wrong} of {want.size} voxels differ')
        assert wrong == 0


def test_nearest_cases_reach_beyond_the_padding():
    """Host formula only: among the 'nearest' cases above there are pixels with a tap outside the padded plane (clamped, not mirrored)."""
    counts = {(s, a): rc.beyond_padding(*rc.rotation_transform(a, s), s) for s in rc.SHAPES for a in rc.ANGLES}
    print({k: v for k, v in counts.items() if v})
    assert counts[((128, 128), 37.5)] > 0 and counts[((33, 57), 45)] > 0
    assert counts[((7, 5), 45)] == 0


def test_three_transforms_in_one_call_equal_three_single_calls(eng):
    for mode in rc.MODES:
        a, _ = rc.float_reference(7, 33, 57, mode)
        full = eng.rotate(a.copy(), (15, 45, 90), mode=mode).cpu().numpy()
        for k, angle in enumerate((15, 45, 90)):
            alone = eng.rotate(a.copy(), (angle,), mode=mode).cpu().numpy()
            assert np.array_equal(alone[:, 0].view(np.uint32), full[:, k].view(np.uint32))


@pytest.mark.parametrize('mode', rc.MODES)
def test_a_slice_alone_and_inside_a_batch_give_the_same_bits(eng, mode):
    a = rc.float_batch(70, 100, 60, seed=11)                   # 70 x (100 [+ 24]) rows: the slices straddle the row pass's 64-row groups
    full = eng.rotate(a.copy(), (37.5, -10), mode=mode).cpu().numpy()
    for k in (0, 33, 69):
        alone = eng.rotate(a[k:k + 1], (37.5, -10), mode=mode).cpu().numpy()
        assert np.array_equal(alone[0].view(np.uint32), full[k].view(np.uint32))


def test_engine_affine_with_a_shear_and_scale_matrix_and_another_output_shape(eng):
    a, _ = rc.float_reference(7, 33, 57, 'constant')
    m, off = np.array([[0.9, 0.2], [-0.1, 1.3]]), np.array([1.5, -2.25])
    for mode in rc.MODES:
        ref = np.stack([scipy.ndimage.affine_transform(x.astype(np.float64), m, off, (40, 29), order=3, mode=mode) for x in a])
        got = eng.affine(a.copy(), m, off, out_hw=(40, 29), mode=mode)
        assert tuple(got.shape) == (7, 1, 40, 29)
        err = float(np.abs(got[:, 0].cpu().numpy().astype(np.float64) - ref).max())
        print(f'affine {mode}: max-abs err {err:.3e}')
        assert np.abs(ref).max() < 2.0 and err <= rc.F32_BAR
    two = eng.affine(a.copy(), np.stack([m, np.eye(2)]), np.stack([off, np.zeros(2)]), out_hw=(33, 57)).cpu().numpy()
    assert np.array_equal(two[:, 1], a)                        # the identity transform at the knots: the samples themselves, to fp32


def test_rotate_forms_scipys_matrix_and_offset():
    for angle in rc.ANGLES:
        m, off = rotation_transform(angle, (33, 57))
        want_m, want_off = rc.rotation_transform(angle, (33, 57))
        assert np.array_equal(m, want_m) and np.array_equal(off, want_off)


def test_bad_arguments_are_refused(eng):
    z = np.zeros((1, 4, 4), np.float32)
    with pytest.raises(ValueError):
        eng.rotate(np.zeros((4, 4), np.float32), (15,))
    with pytest.raises(ValueError):
        eng.rotate(z, (15,), mode='reflect')
    with pytest.raises(ValueError):
        eng.rotate(np.zeros((1, 1, 4), np.float32), (15,))      # a 1-sample line has no spline
    with pytest.raises(ValueError):
        eng.rotate(z, ())
    with pytest.raises(ValueError):
        eng.rotate(z, tuple(range(1, 18)))                       # 17 transforms
    with pytest.raises(ValueError):
        eng.affine(z, np.eye(3), np.zeros(3))
    with pytest.raises(ValueError):
        eng.affine(z, np.eye(2) * np.nan, np.zeros(2))


def test_volume_to_slices_rotations_on_the_device_against_the_host_call(eng):
    rng = np.random.default_rng(4)
    vol = np.clip(scipy.ndimage.gaussian_filter(rng.random((20, 100, 90)), 2.0) * 2.0, 0, None)
    seg = (scipy.ndimage.gaussian_filter(rng.standard_normal((20, 100, 90)), 3.0) > 0.02).astype(np.float64)
    kw = dict(slice_start=2, slice_end=18, slice_resolution=(64, 64), skull_stripping=False, empty_thresh=0.0)
    rot = dict(rotations=(0, 15, -10), center_crop=(48, 40))
    im_h, lb_h, kept_h = nifti.volume_to_slices(vol, seg, **kw, **rot)                   # the host call: scipy throughout
    # the condition on the label input of tests/test_gpu_resample.py, on scipy alone: no resampled label value within the fp32 bar of the 0.9 cut
    padded = [np.pad(seg[s], ((0, 0), (5, 5)), 'constant') for s in kept_h[::3]]
    un = np.stack([scipy.ndimage.zoom(p, 64 / 100.0, mode='nearest') for p in padded])
    assert np.count_nonzero(np.abs(un - 0.9) < rc.F32_BAR) == 0
    im_d, lb_d, kept_d = nifti.volume_to_slices(vol, seg, engine=eng, **kw, **rot)
    assert kept_d == kept_h and len(kept_h) == 3 * 16 and kept_h[:4] == [2, 2, 2, 3]
    assert im_d.shape == im_h.shape == (48, 40, 48) and lb_d.shape == lb_h.shape
    assert im_d.dtype == im_h.dtype == np.float32 and lb_d.dtype == lb_h.dtype == np.float32
    err_i = float(np.abs(im_d.astype(np.float64) - im_h.astype(np.float64)).max())
    err_l = float(np.abs(lb_d.astype(np.float64) - lb_h.astype(np.float64)).max())
    print(f'volume_to_slices with rotations: images max-abs err {err_i:.3e}, labels {err_l:.3e}')
    assert np.abs(im_h).max() < 2.0 and np.abs(lb_h).max() < 2.0
    assert err_i <= rc.F32_BAR and err_l <= rc.F32_BAR
    im_0, lb_0, kept_0 = nifti.volume_to_slices(vol, seg, engine=eng, center_crop=(48, 40), **kw)     # the unrotated device output
    assert kept_0 == kept_h[::3]
    assert np.array_equal(im_d[0::3].view(np.uint32), im_0.view(np.uint32)) and np.array_equal(lb_d[0::3], lb_0)
    im_s, lb_s, _ = nifti.volume_to_slices(vol, seg, engine=eng, device_rotate=False, **kw, **rot)    # device zoom, host rotation loop
    assert np.abs(im_d.astype(np.float64) - im_s).max() <= rc.F32_BAR and np.abs(lb_d.astype(np.float64) - lb_s).max() <= rc.F32_BAR


def test_zoom_keeps_the_bits_of_the_parent_commit(eng):
    """eng.zoom on one case of tests/test_gpu_resample.py's list (100x60 -> 50x90, three slices, both modes and outputs) against the output recorded
    from the library of the commit before the prefilter kernels got their boundary parameter (tests/golden/make_zoom_parent_golden.py)."""
    g = np.load(GOLDEN)
    a = rc.float_batch(3, 100, 60, seed=int(g['seed']))
    assert np.array_equal(a, g['input'])
    for mode in rc.MODES:
        got = eng.zoom(a, (50, 90), mode=mode).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), g[f'f32_{mode}'].view(np.uint32))
        m = (a * 3).astype(np.int64)
        assert np.array_equal(eng.zoom(m, (50, 90), mode=mode, integer=True).cpu().numpy(), g[f'i32_{mode}'])
