"""CPU: the kernels of uad_brain_boxes / uad_brain_boxes_f32 and uad_assemble_batch (csrc/uad_batch.hip) against the numpy statement of
tests/batch_cases.py, without a GPU -- tests/native/batch_emu.cpp compiles the kernel source itself for the host with -ffp-contract=off, runs
the threads of a boxes workgroup as real threads around a std::barrier with the LDS poisoned before every workgroup, and drives the kernels
with the library's launch geometry.  Every output sits between guard words; the emulator fails when one is written, or when an output that
was not asked for is touched.  Boxes are integers and masking copies or multiplies by 0 / 1: the bar is equality, for the batch as uint32
so that -0.0 and NaN payloads count.  With noise the bar is the generator's (tests/test_gpu_rng.py), scaled by sigma, plus one ulp of |x|.
The element count of a slice is a multiple of 4 (a DeviceDataset precondition, checked by the entry point), so a slice with a ragged last
quad cannot occur and no case has one."""
import os
import subprocess

import numpy as np
import pytest

from tests import batch_cases as bc
from tests.emu_build import build_emu


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'batch_emu', 'uad_batch.hip')
    d = os.path.dirname(exe)
    f = lambda name: os.path.join(d, name)

    def boxes_u8(labels, lut, offset=0):
        n, H, W = labels.shape
        np.ascontiguousarray(labels, np.uint8).tofile(f('lab.u8'))
        if lut is not None:
            np.ascontiguousarray(lut, np.uint8).tofile(f('lut.u8'))
        subprocess.run([exe, 'boxes_u8', f('lab.u8'), str(offset), *map(str, (n, H, W)), f('lut.u8') if lut is not None else '-', f('box.i32')], check=True)
        return np.fromfile(f('box.i32'), np.int32).reshape(n, 4)

    def boxes_f32(masks):
        n, H, W = masks.shape
        np.ascontiguousarray(masks, np.float32).tofile(f('mask.f32'))
        subprocess.run([exe, 'boxes_f32', f('mask.f32'), *map(str, (n, H, W)), f('box.i32')], check=True)
        return np.fromfile(f('box.i32'), np.int32).reshape(n, 4)

    def assemble(src, idx, rects, noise=None, want_x=True):
        N, H, W, C = src.shape
        n = N if idx is None else len(idx)
        np.ascontiguousarray(src, np.float32).tofile(f('src.f32'))
        if idx is not None:
            np.ascontiguousarray(idx, np.int32).tofile(f('idx.i32'))
        if rects is not None:
            np.ascontiguousarray(rects, np.int32).tofile(f('rects.i32'))
        sigma, seed, step, sample0, stream = noise if noise is not None else (0.0, 0, 0, 0, 0)
        subprocess.run([exe, 'assemble', f('src.f32'), str(N), f('idx.i32') if idx is not None else '-', *map(str, (n, H, W, C)),
                        f('rects.i32') if rects is not None else '-', repr(float(sigma)), str(seed), str(step), str(sample0), str(stream), str(int(want_x)),
                        f('x.f32'), f('ce.f32')], check=True)
        x = np.fromfile(f('x.f32'), np.float32).reshape(n, H, W, C) if want_x else None
        ce = np.fromfile(f('ce.f32'), np.float32).reshape(n, H, W, C) if rects is not None else None
        return x, ce
    return boxes_u8, boxes_f32, assemble


# ---------------------------------------------------------------------------------------------------------------- boxes
@pytest.mark.parametrize('shape', bc.BOX_SHAPES, ids=bc.shape_id)
def test_boxes_kernel_equals_argwhere(emu, shape):
    names, _ = bc.mask_stack(shape)
    for lut_kind in (None, 'brain', 'random'):
        labels, lut, want = bc.label_store(shape, lut_kind)
        ref = bc.boxes_reference(want)
        assert (ref[names.index('empty')] == -1).all() and (ref[names.index('full')] == (0, shape[0] - 1, 0, shape[1] - 1)).all()
        for offset in ((0, 1, 2, 3) if shape != (128, 128) else (0, 3)):
            assert np.array_equal(emu[0](labels, lut, offset), ref), (lut_kind, offset)
    masks, want = bc.f32_masks(shape)
    assert np.array_equal(emu[1](masks), bc.boxes_reference(want))


def test_boxes_kernel_on_single_slices(emu):
    """n = 1 and a store of one pattern repeated: a slice's box depends on neither n nor its place in the store."""
    labels, lut, want = bc.label_store((26, 30), 'brain')
    ref = bc.boxes_reference(want)
    for i in (0, 5, len(labels) - 1):
        assert np.array_equal(emu[0](labels[i:i + 1], lut, 1), ref[i:i + 1])
    rep = np.repeat(labels[4:5], 5, axis=0)
    assert np.array_equal(emu[0](rep, lut, 2), np.repeat(ref[4:5], 5, axis=0))


# ---------------------------------------------------------------------------------------------------------------- assemble without noise
@pytest.mark.parametrize('n', [1, 3, 64])
@pytest.mark.parametrize('shape', bc.ASM_SHAPES, ids=bc.shape_id)
def test_assemble_kernel_gathers_and_masks_the_words(emu, shape, n):
    N = max(n, 5)
    src = bc.source(N, shape, seed=n)
    rects = bc.rects_case('mixed', n, shape)
    assert bc.masks_something(rects, shape)                         # no masking case passes vacuously
    for kind in (None, 'perm', 'repeat'):
        idx = bc.index_case(kind, N, n) if (kind is not None or n != N) else None
        if idx is None and n != N:
            idx = np.arange(n, dtype=np.int32)
        want_x, want_ce, mask = bc.assemble_reference(src, idx, rects)
        under = want_x[mask == 0]
        if n == 64:                                                 # the inputs under the windows: negatives, +-0, +-inf, NaN, denormals
            assert (under < 0).any() and np.isinf(under).any() and np.isnan(under).any() and (np.abs(under[under != 0]) < 1e-38).any()
            assert (np.signbit(under) & (under == 0)).any()
        x, ce = emu[2](src, idx, rects)
        assert bc.same_bits(x, want_x) and bc.same_bits(ce, want_ce), kind
        x, ce = emu[2](src, idx, rects, want_x=False)               # the context mask alone
        assert x is None and bc.same_bits(ce, want_ce)
    x, ce = emu[2](src[:n], None, None)                             # the gather alone: a copy of the words
    assert ce is None and bc.same_bits(x, src[:n])


def test_assemble_kernel_without_a_window(emu):
    """The named no-window cases: an unused table gives x_ce = x * 1, which keeps every word but a signalling NaN's quiet bit."""
    shape = (26, 30, 1)
    src = bc.source(3, shape, seed=9)
    rects = bc.rects_case('none', 3, shape)
    assert not bc.masks_something(rects, shape)
    want_x, want_ce, _ = bc.assemble_reference(src, None, rects)
    x, ce = emu[2](src, None, rects)
    assert bc.same_bits(x, want_x) and bc.same_bits(ce, want_ce) and bc.same_bits(ce, src)


# ---------------------------------------------------------------------------------------------------------------- assemble with noise
@pytest.mark.parametrize('sigma', [0.01, 1.0])
@pytest.mark.parametrize('shape', [(26, 30, 1), (32, 32, 2)], ids=bc.shape_id)
def test_assemble_kernel_adds_the_generators_noise(emu, shape, sigma):
    n, N = 8, 11
    src = bc.source(N, shape, seed=2, special=False)
    idx = bc.index_case('repeat', N, n)
    rects = bc.rects_case('mixed', n, shape)
    assert bc.masks_something(rects, shape)
    noise = (sigma, 0x1234567890ABCDEF, (1 << 33) + 17, 40, 64)
    ref = bc.noise_reference(n, shape, noise)
    gathered = src[idx]
    x, ce = emu[2](src, idx, rects, noise)
    err = np.abs(x.astype(np.float64) - (gathered.astype(np.float64) + np.float64(np.float32(sigma)) * ref.astype(np.float64)))
    bound = bc.noise_bound(gathered, ref, sigma)
    print(f'assemble noise {bc.shape_id(shape)} sigma {sigma}: max err {err.max():.3e}, smallest bound {bound.min():.3e}, worst ratio {(err / bound).max():.3f}')
    assert (err <= bound).all()
    assert bc.same_bits(ce, x * bc.rect_masks(rects, shape))        # the mask multiplies the NOISY batch
    assert ((x - gathered) / np.float32(sigma)).std() > 0.9   # and it is noise of the asked size, not a copy
    # two halves with sample0 = 40, 44 are the whole: a sample's noise does not depend on the split
    xa, _ = emu[2](src, idx[:4], rects[:4], noise)
    xb, _ = emu[2](src, idx[4:], rects[4:], noise[:3] + (44,) + noise[4:])
    assert bc.same_bits(np.concatenate([xa, xb]), x)
    # another step or another stream id: other numbers
    assert not bc.same_bits(emu[2](src, idx, rects, noise[:2] + (noise[2] + 1,) + noise[3:])[0], x)
    assert not bc.same_bits(emu[2](src, idx, rects, noise[:4] + (0,))[0], x)
