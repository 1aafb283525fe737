"""CPU: the host statement of the curvature-flow filter (utils/curvature_flow.py; nii.denoise(), utils/NII.py:85-87) held to its
specification on cases whose answers are derived by hand, to an independent scalar re-statement that lives in this file, and the C-ABI
entry's declaration, export, binding and argument refusals.  SimpleITK is not available: the specification is ITK's
CurvatureFlowFunction::ComputeUpdate written down from its source, and nothing here compares with SimpleITK's output.

The hand cases use one iteration, time step 0.125, on a 5 x 9 x 11 grid with x in [-5, 5], y in [-4, 4]; "interior" is [1:-1, 1:-1, 1:-1].
With u = u(x, y) and unit spacing the update is (u_yy u_x^2 + u_xx u_y^2 - 2 u_x u_y u_xy) / (u_x^2 + u_y^2) in central differences."""
import ctypes
import os
import re

import numpy as np
import pytest

from unsupervised_anomaly_detection_brain_mri_amd import _lib
from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti
from unsupervised_anomaly_detection_brain_mri_amd.utils.curvature_flow import curvature_flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, Y, X = np.meshgrid(np.arange(5.0), np.arange(-4.0, 5.0), np.arange(-5.0, 6.0), indexing='ij')
R2 = (X * X + Y * Y)[1:-1, 1:-1, 1:-1]
IN = (slice(1, -1),) * 3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_constants_come_back_unchanged():
    np.testing.assert_array_equal(_bits(curvature_flow(np.full((1, 1, 1), 3.25))), _bits(np.full((1, 1, 1), 3.25)))
    c = np.full((5, 9, 11), -7.125)
    for spacing in ((1, 1, 1), (0.5, 2.0, 0.25)):
        np.testing.assert_array_equal(_bits(curvature_flow(c, spacing)), _bits(c))


def test_paraboloid_pins_the_second_difference_terms_and_the_squared_scales():
    u = X * X + Y * Y
    out = curvature_flow(u, iterations=1)
    # u_x = 2x, u_y = 2y, u_xx = u_yy = 2: update = 8 (x^2 + y^2) / (4 (x^2 + y^2)) = 2, times 0.125
    np.testing.assert_array_equal(out[IN][R2 > 0], (u + 0.25)[IN][R2 > 0])
    np.testing.assert_array_equal(out[IN][R2 == 0], u[IN][R2 == 0])            # no gradient on the axis: the gate
    # spacing (0.5, 0.5, 4): first differences double, second differences quadruple: update = 8, times 0.125
    out = curvature_flow(u, (0.5, 0.5, 4.0), iterations=1)
    np.testing.assert_array_equal(out[IN][R2 > 0], (u + 1.0)[IN][R2 > 0])


def test_linear_ramp_is_a_fixed_point_inside_and_shows_the_replicate_rule_at_the_boundary():
    u = 3 * X - 2 * Y + 5 * Z + 1
    out = curvature_flow(u, (0.5, 2.0, 0.25), iterations=1)
    np.testing.assert_array_equal(_bits(out[IN]), _bits(u[IN]))
    assert np.count_nonzero(out != u) > 0


def test_cross_term_pins_the_corner_taps_and_their_sign():
    u = X * Y
    out = curvature_flow(u, iterations=1)
    # u_x = y, u_y = x, u_xy = 1, second differences 0: update = -2 x y / (x^2 + y^2); every intermediate is exact except the one division
    with np.errstate(invalid='ignore'):
        w = np.where(X * X + Y * Y == 0, 0.0, (-2 * X * Y / (X * X + Y * Y)) * 0.125)
    np.testing.assert_array_equal(out[IN], (u + w)[IN])
    assert np.count_nonzero(w[IN]) > 0


def test_gate_at_a_squared_gradient_of_1e_minus_9():
    u = 1e-5 * (X * X + Y * Y)
    out = curvature_flow(u, iterations=1)
    # |grad|^2 = 4e-10 (x^2 + y^2): <= 8e-10 for x^2 + y^2 in {0, 1, 2}, >= 1.6e-9 from 4 on
    np.testing.assert_array_equal(_bits(out[IN][R2 <= 2]), _bits(u[IN][R2 <= 2]))
    assert np.all(out[IN][R2 >= 4] != u[IN][R2 >= 4]) and np.count_nonzero(R2 == 3) == 0


def test_iteration_semantics():
    u = np.random.default_rng(5).random((6, 7, 8))
    keep = u.copy()
    sp = (0.9, 1.1, 3.0)
    three = curvature_flow(u, sp, 0.125, 3)
    step = u
    for _ in range(3):
        step = curvature_flow(step, sp, 0.125, 1)
    np.testing.assert_array_equal(_bits(three), _bits(step))
    zero = curvature_flow(u, sp, 0.125, 0)
    np.testing.assert_array_equal(_bits(zero), _bits(u))
    assert zero is not u and not np.shares_memory(zero, u) and np.array_equal(u, keep)
    assert curvature_flow(u.astype(np.float32)).dtype == np.float64
    for bad in (dict(spacing=(1, 0, 1)), dict(spacing=(1, -1, 1)), dict(spacing=(1, np.nan, 1)), dict(spacing=(1, 1)), dict(iterations=-1)):
        with pytest.raises(ValueError):
            curvature_flow(u, **bad)
    with pytest.raises(ValueError):
        curvature_flow(u[0])


def _scalar_restatement(u, spacing, time_step):
    """One iteration, voxel by voxel, straight from the specification; imports nothing from the module under test."""
    nz, ny, nx = u.shape
    hi = (nx - 1, ny - 1, nz - 1)
    a = [1.0 / float(s) for s in spacing]
    out = np.empty_like(u)

    def e(i, sign):
        d = [0, 0, 0]
        d[i] = sign
        return d

    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                def p(d):
                    q = [min(max(v + dv, 0), h) for v, dv, h in zip((x, y, z), d, hi)]
                    return float(u[q[2], q[1], q[0]])
                c = p((0, 0, 0))
                f, s, cr = [0.0] * 3, [0.0] * 3, {}
                mag = 0.0
                for i in range(3):
                    f[i] = (0.5 * (p(e(i, 1)) - p(e(i, -1)))) * a[i]
                    s[i] = ((p(e(i, 1)) - 2 * c) + p(e(i, -1))) * (a[i] * a[i])
                    for j in range(i + 1, 3):
                        mm, mp, pm, pp = ([si * ei + sj * ej for ei, ej in zip(e(i, 1), e(j, 1))] for si, sj in ((-1, -1), (-1, 1), (1, -1), (1, 1)))
                        cr[i, j] = ((0.25 * (((p(mm) - p(mp)) - p(pm)) + p(pp))) * a[i]) * a[j]
                    mag = mag + f[i] * f[i]
                upd = 0.0
                if not mag < 1e-9:
                    for i in range(3):
                        t = 0.0
                        for j in range(3):
                            if j != i:
                                t = t + s[j]
                        upd = upd + t * (f[i] * f[i])
                    for i in range(3):
                        for j in range(i + 1, 3):
                            upd = upd - ((2 * f[i]) * f[j]) * cr[i, j]
                    upd = upd / mag
                out[z, y, x] = c + upd * time_step
    return out


@pytest.mark.parametrize('shape', [(4, 5, 6), (1, 1, 7)], ids=lambda s: '%dx%dx%d' % s)
def test_vectorised_statement_equals_an_independent_scalar_restatement(shape):
    u = np.random.default_rng(sum(shape)).random(shape)
    sp = (0.9, 1.1, 3.0)
    np.testing.assert_array_equal(_bits(curvature_flow(u, sp, 0.125, 1)), _bits(_scalar_restatement(u, sp, 0.125)))
    two = _scalar_restatement(_scalar_restatement(u, sp, 0.125), sp, 0.125)
    np.testing.assert_array_equal(_bits(curvature_flow(u, sp, 0.125, 2)), _bits(two))


def test_the_two_entries_are_declared_bound_and_exported():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'uad_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(uad_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('uad_curvature_flow_workspace', 'uad_curvature_flow'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SYMBOLS[name]
    ws = lib.uad_curvature_flow_workspace
    assert ws(110, 217, 181) == 110 * 217 * 181 * 8
    assert ws(192, 512, 512) == 192 * 512 * 512 * 8
    assert ws(1024, 1024, 1024) == 2 ** 33                            # a byte count that does not fit an int
    assert ws(0, 4, 4) == 0


def test_bad_arguments_are_refused_before_any_device_work():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.uad_curvature_flow
    fn.restype, fn.argtypes = _lib.SYMBOLS['uad_curvature_flow']
    p, q, w = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)       # never dereferenced: every call below is refused

    def call(nz=4, ny=4, nx=4, spacing=(1.0, 1.0, 1.0), iterations=3, src=p, dst=q, ws=w, f32=0):
        sp = None if spacing is None else (ctypes.c_double * 3)(*spacing)
        return fn(src, f32, nz, ny, nx, sp, 0.125, iterations, dst, ws, None)
    invalid = 1                                   # UAD_ERR_INVALID (ValueError in _lib.check)
    assert call(nz=0) == invalid and call(ny=0) == invalid and call(nx=-3) == invalid
    assert call(spacing=(0.0, 1.0, 1.0)) == invalid and call(spacing=(1.0, -2.0, 1.0)) == invalid
    assert call(spacing=(1.0, 1.0, float('nan'))) == invalid and call(spacing=(float('inf'), 1.0, 1.0)) == invalid and call(spacing=None) == invalid
    assert call(iterations=-1) == invalid
    assert call(src=None) == invalid and call(dst=None) == invalid and call(ws=None) == invalid
    assert call(dst=p) == invalid                 # out may not alias in
    with pytest.raises(ValueError):
        _lib.check(call(f32=1, iterations=-2))


class _FlowEngine:
    """A host stand-in with device_ops.DeviceOps.curvature_flow's signature that records its calls (no other op: the rest of the path stays on the host)."""

    def __init__(self):
        self.calls = []

    def curvature_flow(self, vol, spacing=(1, 1, 1), time_step=0.125, iterations=3):
        import torch
        self.calls.append((tuple(np.shape(vol)), tuple(spacing), time_step, iterations))
        return torch.from_numpy(curvature_flow(vol, spacing, time_step, iterations))


def _phantom(seed, shape=(12, 40, 40)):
    """tests/test_nifti.py's phantom."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing='ij')
    brain = (x ** 2 + y ** 2 + (z * 0.8) ** 2) < 0.7
    vol = (500 + 200 * x + 100 * rng.standard_normal(shape)) * brain + 30 * rng.random(shape)
    seg = ((x - 0.2) ** 2 + (y + 0.1) ** 2 + z ** 2 < 0.03).astype(np.float32)
    return vol, seg, brain.astype(np.float32)


def test_volume_to_slices_filters_before_the_skull_map():
    vol, seg, brain = _phantom(1)
    vol[3, 4, 5] = np.nan
    kw = dict(slice_start=1, slice_end=11, slice_resolution=(32, 32))
    sp = (0.5, 0.5, 3.0)
    plain = nifti.volume_to_slices(vol, seg, brain, **kw)
    for off in (None, False):
        same = nifti.volume_to_slices(vol, seg, brain, curvature_flow=off, spacing=sp, **kw)
        assert same[2] == plain[2] and np.array_equal(_bits(same[0]), _bits(plain[0])) and np.array_equal(same[1], plain[1])
    im, lb, kept = nifti.volume_to_slices(vol, seg, brain, curvature_flow=True, spacing=sp, **kw)
    # by hand: zero the NaN, filter, then the unfiltered pipeline (which multiplies by the skull map first thing)
    by_hand = nifti.volume_to_slices(curvature_flow(np.nan_to_num(vol, nan=0.0), sp, 0.125, 3), seg, brain, **kw)
    assert kept == by_hand[2] and np.array_equal(_bits(im), _bits(by_hand[0])) and np.array_equal(lb, by_hand[1])
    assert len(kept) > 3 and (kept != plain[2] or not np.array_equal(im, plain[0]))
    pair = nifti.volume_to_slices(vol, seg, brain, curvature_flow=(1, 0.0625), spacing=sp, **kw)
    by_hand = nifti.volume_to_slices(curvature_flow(np.nan_to_num(vol, nan=0.0), sp, 0.0625, 1), seg, brain, **kw)
    assert np.array_equal(_bits(pair[0]), _bits(by_hand[0]))
    eng = _FlowEngine()
    routed = nifti.volume_to_slices(vol, seg, brain, curvature_flow=(2, 0.125), spacing=sp, engine=eng, device_stats=False, device_rotate=False,
                                    **dict(kw, slice_resolution=None))
    assert eng.calls == [((12, 40, 40), sp, 0.125, 2)]
    host = nifti.volume_to_slices(vol, seg, brain, curvature_flow=(2, 0.125), spacing=sp, **dict(kw, slice_resolution=None))
    assert routed[2] == host[2] and np.array_equal(_bits(routed[0]), _bits(host[0]))
    for bad in (5, (1, 2, 3), (-1, 0.125), (1.5, 0.125)):
        with pytest.raises(ValueError):
            nifti.volume_to_slices(vol, seg, brain, curvature_flow=bad, **kw)
    with pytest.raises(NotImplementedError):                                   # unchanged: the reference's own switch still has no meaning here
        nifti.volume_to_slices(vol, denoise=True, curvature_flow=True)


def test_build_cache_passes_the_header_spacing(tmp_path, monkeypatch):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    patients = []
    for i in range(2):
        vol, seg, brain = _phantom(20 + i)
        d = tmp_path / f'p{i}'
        d.mkdir()
        nifti.write_nifti(str(d / 'flair.nii.gz'), vol, pixdim=(0.5, -0.5, 3.0) if i == 0 else (0.0, 2.0, 1.0))
        nifti.write_nifti(str(d / 'gt.nii.gz'), seg, dtype='u1')
        nifti.write_nifti(str(d / 'mask.nii.gz'), brain, dtype='u1')
        patients.append({'name': f'p{i}', 'volume': str(d / 'flair.nii.gz'), 'groundtruth': str(d / 'gt.nii.gz'), 'skullmap': str(d / 'mask.nii.gz')})
    seen = []
    real = nifti.volume_to_slices

    def spy(*a, **k):
        seen.append(k.get('spacing'))
        return real(*a, **k)
    monkeypatch.setattr(nifti, 'volume_to_slices', spy)
    kw = dict(partition={'TRAIN': 0.5, 'VAL': 0.5}, seed=0, slice_start=1, slice_end=11, slice_resolution=(32, 32))
    nifti.build_cache(str(tmp_path / 'flow'), patients, curvature_flow=True, **kw)
    assert seen == [(0.5, 0.5, 3.0), (1.0, 2.0, 1.0)]                        # abs(pixdim[1:4]), zero -> 1
    nifti.build_cache(str(tmp_path / 'plain'), patients, **kw)
    a, _, ia = read_cache(str(tmp_path / 'flow'))
    b, _, _ = read_cache(str(tmp_path / 'plain'))
    assert ia['options']['curvature_flow'] is True
    assert a.shape != b.shape or not np.array_equal(a, b)
    # the host pipeline by hand, with the header's spacing
    monkeypatch.setattr(nifti, 'volume_to_slices', real)
    want = []
    for i, sp in ((0, (0.5, 0.5, 3.0)), (1, (1.0, 2.0, 1.0))):
        vol, seg, brain = (nifti.read_nifti(patients[i][k])[0] for k in ('volume', 'groundtruth', 'skullmap'))
        want.append(nifti.volume_to_slices(curvature_flow(vol, sp), seg, brain, slice_start=1, slice_end=11, slice_resolution=(32, 32))[0])
    order = [int(n[1:]) for n in dict.fromkeys(ia['patients'])]
    np.testing.assert_array_equal(a[..., 0], np.concatenate([want[i] for i in order]))
