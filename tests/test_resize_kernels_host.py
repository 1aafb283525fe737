"""CPU: the arithmetic, the LDS tables and the store paths of uad_resize2d's kernel and of uad_mask_by_label's (csrc/uad_resize.hip) against
the host statement utils/resize.py and numpy, without a GPU -- tests/native/resize_emu.cpp compiles the kernel source itself for the host
with -ffp-contract=off, runs every workgroup's threads as real threads around a std::barrier and drives them with the library's launch
geometry.  The bar is bit equality: both sides perform the same IEEE operations in the same order.  The emulator puts the output between
guard words and fails when one is written, and poisons the LDS tables before every workgroup.  Shapes and inputs are those of tests/test_gpu_resize.py (tests/resize_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import resize_cases as rc
from tests.emu_build import build_emu


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'resize_emu', 'uad_resize.hip')
    d = os.path.dirname(exe)

    def resize(a, out_hw, mode, index=None):
        n_in, h, w = a.shape
        np.ascontiguousarray(a, np.float32).tofile(os.path.join(d, 'in.f32'))
        idx = '-'
        if index is not None:
            idx = os.path.join(d, 'idx.i32')
            np.asarray(index, np.int32).tofile(idx)
        n = n_in if index is None else len(index)
        subprocess.run([exe, 'resize', os.path.join(d, 'in.f32'), *map(str, (n_in, h, w)), idx, *map(str, (n, out_hw[0], out_hw[1], int(mode == 'nearest'))),
                        os.path.join(d, 'out.f32')], check=True)
        return np.fromfile(os.path.join(d, 'out.f32'), np.float32).reshape(n, *out_hw)

    def mask(vol, labels, lut, lesion_label, want_lesion, in_place):
        vol.tofile(os.path.join(d, 'vol.f32')); labels.tofile(os.path.join(d, 'lab.u8')); lut.tofile(os.path.join(d, 'lut.u8'))
        subprocess.run([exe, 'mask', os.path.join(d, 'vol.f32'), os.path.join(d, 'lab.u8'), str(vol.size), os.path.join(d, 'lut.u8'), str(lesion_label),
                        str(int(want_lesion)), str(int(in_place)), os.path.join(d, 'mout.f32'), os.path.join(d, 'mles.f32')], check=True)
        return np.fromfile(os.path.join(d, 'mout.f32'), np.float32), (np.fromfile(os.path.join(d, 'mles.f32'), np.float32) if want_lesion else None)
    return resize, mask


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_kernel_has_the_bits_of_the_host_statement(emu, case):
    hw, out_hw = case
    for mode in rc.MODES:
        for kind in rc.KINDS:
            assert rc.same_bits(emu[0](rc.batch(hw, kind), out_hw, mode), rc.reference(hw, out_hw, mode, kind)), (mode, kind)


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_the_slice_gather_and_the_batch_size(emu, case):
    hw, out_hw = case
    for mode in rc.MODES:
        kind = 'special' if mode == 'nearest' else 'uniform'      # nearest copies bits: held on the +-0 / denormal / 1e30 input
        a = rc.batch(hw, kind, rc.N_RESIDENT)
        ref = rc.reference(hw, out_hw, mode, kind, rc.N_RESIDENT)
        if out_hw[0] * out_hw[1] <= 2048:                                                    # (the larger outputs: seconds of host threads)
            assert rc.same_bits(emu[0](a, out_hw, mode), ref)                                # n = 7 without an index
        assert rc.same_bits(emu[0](a, out_hw, mode, rc.INDEX), ref[rc.INDEX])                # non-monotone, one entry twice
        assert rc.same_bits(emu[0](a[4:5], out_hw, mode), ref[4:5])                          # the same slice alone: bits independent of n
        assert rc.same_bits(emu[0](a, out_hw, mode, [4]), ref[4:5])


def mask_inputs():
    rng = np.random.default_rng(5)
    n = 4099                                                    # 1024 quads and three single elements; more than one workgroup
    vol = rng.standard_normal(n).astype(np.float32)
    vol[::97] = -0.0
    labels = np.concatenate([np.arange(256), rng.integers(0, 256, n - 256)]).astype(np.uint8)
    rng.shuffle(labels)
    lut = (rng.random(256) < 0.6).astype(np.uint8)
    return vol, labels, lut


def test_mask_by_label_kernel(emu):
    vol, labels, lut = mask_inputs()
    want = np.where(lut[labels] != 0, vol, np.float32(0))
    for in_place in (False, True):
        for want_lesion in (False, True):
            out, les = emu[1](vol, labels, lut, 10, want_lesion, in_place)
            assert rc.same_bits(out, want)
            if want_lesion:
                assert rc.same_bits(les, (labels == 10).astype(np.float32))
