"""CPU: the arithmetic of uad_affine_spline3's kernels (csrc/uad_resample.hip: the mirror / reflect prefilter and affine_interp_kernel) against
scipy.ndimage.rotate, without a GPU -- tests/native/affine_emu.cpp compiles the kernel source itself for the host and runs it with the real
launch geometry.  Reference, shapes, angles and bars are those of tests/test_gpu_rotate.py (tests/rotate_cases.py), plus a 2 x 9 slice:
scipy in fp64 on the fp32-rounded input; fp32 output within 1.2e-7 with |ref| < 2; int32 output exactly scipy's on inputs that have no
unrounded value within 1e-9 of a half-integer (asserted)."""
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage

from tests import rotate_cases as rc
from tests.emu_build import build_emu

SHAPES = rc.SHAPES + [(2, 9)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'affine_emu', 'uad_resample.hip')

    def run(a, xf, out_hw, mode, integer):
        n, h, w = a.shape
        xf = np.ascontiguousarray(xf, np.float64).reshape(-1, 6)
        d = os.path.dirname(exe)
        a.astype(np.float32).tofile(os.path.join(d, 'in.f32'))
        xf.tofile(os.path.join(d, 'xf.f64'))
        subprocess.run([exe, os.path.join(d, 'in.f32'), *map(str, (n, h, w, *out_hw)), os.path.join(d, 'xf.f64'), str(len(xf)), str(int(mode == 'nearest')),
                        str(int(integer)), os.path.join(d, 'out.bin')], check=True)
        return np.fromfile(os.path.join(d, 'out.bin'), np.int32 if integer else np.float32).reshape(n, len(xf), *out_hw)
    return run


def _table(angles, shape):
    return np.stack([np.concatenate([m.ravel(), off]) for m, off in (rc.rotation_transform(a, shape) for a in angles)])


@pytest.mark.parametrize('mode', rc.MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_kernel_arithmetic_against_scipy(emu, shape, mode):
    h, w = shape
    xf = _table(rc.ANGLES, shape)
    for n in (1, 3):
        a, ref = rc.float_reference(n, h, w, mode)
        got = emu(a, xf, shape, mode, False)
        assert np.abs(ref).max() < 2.0
        assert np.abs(got.astype(np.float64) - ref).max() <= rc.F32_BAR
        m, un, want = rc.integer_reference(n, h, w, mode)
        assert rc.near_ties(un) == 0
        assert np.count_nonzero(emu(m, xf, shape, mode, True) != want) == 0


def test_a_transform_inside_a_table_has_the_bits_of_the_single_call(emu):
    a, _ = rc.float_reference(3, 33, 57, 'nearest')
    xf = _table((15, 45, 90), (33, 57))
    for mode in rc.MODES:
        full = emu(a, xf, (33, 57), mode, False)
        for k in range(3):
            assert np.array_equal(emu(a, xf[k], (33, 57), mode, False)[:, 0].view(np.uint32), full[:, k].view(np.uint32))


def test_general_matrix_and_another_output_shape(emu):
    a, _ = rc.float_reference(3, 33, 57, 'constant')
    m, off = np.array([[0.9, 0.2], [-0.1, 1.3]]), np.array([1.5, -2.25])
    for mode in rc.MODES:
        ref = np.stack([scipy.ndimage.affine_transform(x.astype(np.float64), m, off, (40, 29), order=3, mode=mode) for x in a])
        got = emu(a, np.concatenate([m.ravel(), off]), (40, 29), mode, False)[:, 0]
        assert np.abs(ref).max() < 2.0 and np.abs(got.astype(np.float64) - ref).max() <= rc.F32_BAR
