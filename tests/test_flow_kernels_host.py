"""CPU: the arithmetic and the LDS ring of uad_curvature_flow's kernel (csrc/uad_flow.hip) against the host statement
utils/curvature_flow.py, without a GPU -- tests/native/flow_emu.cpp compiles the kernel source itself for the host with -ffp-contract=off,
runs every workgroup's threads as real threads around a std::barrier and drives them with the library's launch geometry and ping-pong.
The bar is bit equality: both sides perform the same IEEE fp64 operations in the same order.  Shapes, spacings and iteration counts are
those of tests/test_gpu_flow.py (tests/flow_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import flow_cases as fc
from tests.emu_build import build_emu


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'flow_emu', 'uad_flow.hip')

    def run(vol, spacing, iterations, time_step=fc.TIME_STEP):
        d = os.path.dirname(exe)
        f32 = vol.dtype == np.float32
        np.ascontiguousarray(vol, np.float32 if f32 else np.float64).tofile(os.path.join(d, 'in.bin'))
        subprocess.run([exe, os.path.join(d, 'in.bin'), str(int(f32)), *map(str, vol.shape), *(repr(float(s)) for s in spacing), repr(float(time_step)),
                        str(iterations), os.path.join(d, 'out.f64')], check=True)
        return np.fromfile(os.path.join(d, 'out.f64'), np.float64).reshape(vol.shape)
    return run


@pytest.mark.parametrize('shape', fc.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_kernel_has_the_bits_of_the_host_statement(emu, shape):
    for spacing in fc.SPACINGS:
        for it in fc.ITERATIONS:
            assert fc.same_bits(emu(fc.volume(shape), spacing, it), fc.reference(shape, spacing, it)), (spacing, it)


def test_the_gate_taken_inside_a_tile(emu):
    for spacing in fc.SPACINGS:
        for it in fc.ITERATIONS:
            ref = fc.half_constant_reference(spacing, it)
            assert fc.same_bits(emu(fc.half_constant(), spacing, it), ref)
    one = fc.half_constant_reference(fc.SPACINGS[0], 1)
    assert np.array_equal(one[:, :, :19], fc.half_constant()[:, :, :19]) and np.count_nonzero(one[:, :, 20:] != fc.half_constant()[:, :, 20:]) > 0


def test_fp32_input_is_widened_exactly_and_two_iterations_end_in_the_output(emu):
    shape = (17, 17, 65)
    for it in (1, 2, 3):                    # 2: the first sweep goes to the workspace
        assert fc.same_bits(emu(fc.volume_f32(shape), fc.SPACINGS[1], it), fc.reference(shape, fc.SPACINGS[1], it, True))
    assert fc.same_bits(emu(fc.volume(shape), fc.SPACINGS[1], 2), fc.reference(shape, fc.SPACINGS[1], 2))
    assert fc.same_bits(emu(fc.volume_f32(shape), fc.SPACINGS[1], 0), fc.volume_f32(shape).astype(np.float64))
    assert fc.same_bits(emu(fc.volume(shape), fc.SPACINGS[1], 0), fc.volume(shape))
