"""CPU: the arithmetic of the three kernels of csrc/uad_resample.hip against scipy.ndimage.zoom, without a GPU -- tests/native/resample_emu.cpp
compiles the kernel source itself for the host (the compiler hipcc wraps; sequential blocks, real threads around the row pass's barrier) and runs it
with the launch geometry of uad_zoom_spline3.  Same reference and bars as tests/test_gpu_resample.py: scipy in fp64 on the fp32-rounded input;
fp32 output within 1.2e-7 (twice the half-ulp of the final rounding for |v| < 2); int32 output equal wherever scipy's unrounded value is not
within 1e-9 of a half-integer (2-sample lines do produce such ties; the GPU test's inputs have none)."""
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage

from tests.emu_build import build_emu

CASES = [(217, 181, 128, 128), (128, 128, 217, 181), (80, 80, 64, 64), (64, 64, 80, 80), (100, 60, 50, 90), (5, 40, 8, 64), (2, 3, 5, 4), (30, 150, 31, 70)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'resample_emu', 'uad_resample.hip')

    def run(a, H, W, mode, integer):
        n, h, w = a.shape
        d = os.path.dirname(exe)
        a.astype(np.float32).tofile(os.path.join(d, 'in.f32'))
        subprocess.run([exe, os.path.join(d, 'in.f32'), *map(str, (n, h, w, H, W, int(mode == 'nearest'), int(integer))), os.path.join(d, 'out.bin')], check=True)
        return np.fromfile(os.path.join(d, 'out.bin'), np.int32 if integer else np.float32).reshape(n, H, W)
    return run


@pytest.mark.parametrize('mode', ('constant', 'nearest'))
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%d-%dx%d' % c)
def test_kernel_arithmetic_against_scipy(emu, case, mode):
    h, w, H, W = case
    rng = np.random.default_rng(h * 1000 + W)
    zf = (H / h, W / w)
    for n in (1, 3):
        a = rng.random((n, h, w)).astype(np.float32)
        ref = np.stack([scipy.ndimage.zoom(x.astype(np.float64), zf, mode=mode) for x in a])
        assert ref.shape == (n, H, W)
        assert np.abs(emu(a, H, W, mode, False).astype(np.float64) - ref).max() <= 1.2e-7
        f = scipy.ndimage.gaussian_filter(rng.standard_normal((n, h, w)), (0, min(h, 8) / 4, min(w, 8) / 4))
        m = (f > np.quantile(f, 0.55)).astype(int) + (f > np.quantile(f, 0.9)).astype(int)
        unrounded = np.stack([scipy.ndimage.zoom(x.astype(np.float64), zf, mode=mode) for x in m])
        tie = np.abs(np.abs(unrounded - np.floor(unrounded)) - 0.5) < 1e-9
        if min(h, w) > 2:
            assert np.count_nonzero(tie) <= 1e-5 * tie.size
        want = np.stack([scipy.ndimage.zoom(x, zf, mode=mode) for x in m])
        assert np.count_nonzero((emu(m, H, W, mode, True) != want) & ~tie) == 0


def test_constant_mode_writes_zero_where_scipy_sees_the_last_sample_outside(emu):
    a = np.random.default_rng(0).random((1, 128, 128)).astype(np.float32) + 0.5
    ref = scipy.ndimage.zoom(a[0].astype(np.float64), (217 / 128, 181 / 128), mode='constant')
    assert np.all(ref[:, 180] == 0) and np.all(ref[:, :180] != 0)          # 180 * (127 / 180) rounds above 127: scipy's cval column
    got = emu(a, 217, 181, 'constant', False)[0]
    assert np.all(got[:, 180] == 0) and np.abs(got - ref).max() <= 1.2e-7
