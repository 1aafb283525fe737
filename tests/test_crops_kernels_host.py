"""CPU: the four kernels of uad_cc_props and the kernel of uad_crop2d (csrc/uad_crops.hip) against the host statement utils/crops.py, without a
GPU -- tests/native/crops_emu.cpp compiles the kernel source itself for the host, runs every workgroup's threads as real threads around a
std::barrier with the compiler's atomics and drives them with the library's launch geometry and workspace layout.  The bar is equality: the
measurements are integers, the gather copies words.  The emulator puts every output between guard words and fails when one is written (a
row past the count or the cap among them), poisons the LDS before every workgroup and the workspace before the call.  The label volumes are
the model of uad_cc_label's output (tests/crops_cases.py: labels_model); shapes and inputs are those of tests/test_gpu_crops.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import crops_cases as cc
from tests.emu_build import build_emu


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'crops_emu', 'uad_crops.hip')
    d = os.path.dirname(exe)

    def props(labels, max_components):
        D, H, W = labels.shape
        np.ascontiguousarray(labels, np.int32).tofile(os.path.join(d, 'lab.i32'))
        subprocess.run([exe, 'props', os.path.join(d, 'lab.i32'), *map(str, (D, H, W, max_components)), os.path.join(d, 'props.i64'), os.path.join(d, 'n.i32')],
                       check=True)
        return np.fromfile(os.path.join(d, 'props.i64'), np.int64).reshape(-1, 5), int(np.fromfile(os.path.join(d, 'n.i32'), np.int32)[0])

    def crop(batch, origins, size):
        n, h, w = batch.shape
        np.ascontiguousarray(batch, np.float32).tofile(os.path.join(d, 'in.f32'))
        np.ascontiguousarray(origins, np.int32).tofile(os.path.join(d, 'org.i32'))
        subprocess.run([exe, 'crop', os.path.join(d, 'in.f32'), *map(str, (n, h, w)), os.path.join(d, 'org.i32'), *map(str, (len(origins), size[0], size[1])),
                        os.path.join(d, 'out.f32')], check=True)
        return np.fromfile(os.path.join(d, 'out.f32'), np.float32).reshape(len(origins), *size)
    return props, crop


def _hold(emu, shape, kind, slab):
    want = cc.props_reference(shape, kind, slab)
    got, n = emu[0](cc.labels_model(shape, kind, slab), max(len(want), 1))
    assert n == len(want) and np.array_equal(got, want), (shape, kind, slab)
    return want


@pytest.mark.parametrize('shape', cc.PROPS_SHAPES, ids=cc.shape_id)
def test_props_kernels_equal_the_host_statement(emu, shape):
    # (the largest shape on fewer variants: 64 workgroups of 256 host threads a launch)
    variants = [(k, s) for k in cc.KINDS for s in cc.SLABS] if shape != (4, 128, 128) else [('fill2', 1), ('fill30', 0), ('chain', 2)]
    for kind, slab in variants:
        _hold(emu, shape, kind, slab)


def test_props_kernels_on_the_structured_volumes(emu):
    for slab in cc.SLABS:
        want = _hold(emu, cc.SPAN_SHAPE, 'span', slab)
        assert len(want) == {0: 1, 1: 5, 2: 3}[slab]
        assert _hold(emu, cc.SPAN_SHAPE, 'empty', slab).shape == (0, 5)
        _hold(emu, (3, 9, 9), 'corner', slab)
        _hold(emu, (3, 9, 33), 'full', slab)


def test_props_kernels_under_a_cap(emu):
    shape, kind = (9, 16, 70), 'fill2'
    want = cc.props_reference(shape, kind, 1)
    assert len(want) > 8
    for cap in (1, 7, len(want) - 1):
        got, n = emu[0](cc.labels_model(shape, kind, 1), cap)     # the emulator fails when a word past row cap - 1 is written
        assert n == len(want) and np.array_equal(got, want[:cap])


@pytest.mark.parametrize('size', cc.CROP_SIZES, ids=lambda s: '%dx%d' % s)
def test_crop_kernel_copies_the_words(emu, size):
    batch, origins, want = cc.crop_batch(), cc.crop_origins(size), cc.crop_reference(size)
    assert cc.same_bits(emu[1](batch, origins, size), want)
    assert cc.same_bits(emu[1](batch, origins[4:5], size), want[4:5])                 # k = 1: the same window alone
    if size[1] % 4 == 0:
        assert cc.same_bits(emu[1](batch, origins[1:2], size), want[1:2])
