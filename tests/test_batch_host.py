"""CPU: the host half of the device context masking and instance noise -- draw_context_squares (the draw of the reference's
trainers/CE.py:127-137 without the pixels) against retrieve_masked_batch and its oracle restatement, the window-table check of
DeviceOps.context_mask, the declaration / binding / export of the three entry points of csrc/uad_batch.hip, and the argument handling of
DeviceDataset that needs no device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from oracle import vae as ovae
from tests import batch_cases as bc
from unsupervised_anomaly_detection_brain_mri_amd import _lib
from unsupervised_anomaly_detection_brain_mri_amd.device_ops import check_rects
from unsupervised_anomaly_detection_brain_mri_amd.trainers.CE import draw_context_squares, retrieve_masked_batch, squares_to_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('uad_brain_boxes', 'uad_brain_boxes_f32', 'uad_assemble_batch')


def _box_mask(h, w, boxes):
    """[n,h,w,1] brain masks that are exactly the given (r0, r1, c0, c1) boxes' corners -- two pixels span a box."""
    bm = np.zeros((len(boxes), h, w, 1), bool)
    for i, (r0, r1, c0, c1) in enumerate(boxes):
        bm[i, r0, c0] = bm[i, r1, c1] = True
    return bm


def _cases():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'cemask_golden.npz'))
    out = [(f'golden{i}', g[f'bm{i}'], int(g[f'seed{i}'])) for i in range(4)]
    rng = np.random.default_rng(0)
    blobs = np.zeros((5, 64, 64, 1), bool)
    for i in range(5):
        r, c = rng.integers(0, 30, 2)
        blobs[i, r:r + int(rng.integers(5, 34)), c:c + int(rng.integers(5, 34))] = True
    out.append(('fresh_blobs', blobs, 21))
    # too small for a square in the rows only, the columns only, both; r0 >= r1 - 20 is "does not draw"
    out.append(('too_small', _box_mask(64, 64, [(10, 30, 5, 50), (5, 50, 10, 30), (10, 30, 10, 30), (0, 63, 0, 63)]), 3))
    # exactly 22 rows / columns: r1 - r0 = 21 is the smallest box that draws (r0 < r1 - 20): two positions, r0 and r0 + 1
    out.append(('rows22', _box_mask(64, 64, [(7, 28, 9, 30), (7, 27, 9, 30), (0, 63, 0, 63)]), 4))
    # the last sample draws nothing while earlier ones do: under A3 the batch comes back unmasked
    out.append(('last_draws_nothing', _box_mask(64, 64, [(0, 63, 0, 63), (2, 60, 3, 61), (10, 25, 10, 25)]), 5))
    return out


CASES = _cases()


def _boxes(bm):
    return bc.boxes_reference(bm[..., 0])


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_draw_then_multiply_equals_retrieve_masked_batch(case):
    name, bm, seed = case
    rng0 = np.random.default_rng(seed)
    batch = rng0.standard_normal(bm.shape).astype(np.float32)
    r_new, r_old, r_orc = random.Random(seed), random.Random(seed), random.Random(seed)
    rects = draw_context_squares(_boxes(bm), r_new)
    assert rects.dtype == np.int32 and rects.shape == (len(bm), 3, 4)
    check_rects(rects, len(bm), bm.shape[1], bm.shape[2])                                     # every drawn window lies inside the slice
    got = batch * squares_to_mask(rects[-1], batch.shape[1:])                                  # A3: the last sample's mask for all
    assert bc.same_bits(got, retrieve_masked_batch(batch, bm, r_old))
    assert bc.same_bits(got, ovae.retrieve_masked_batch(batch, bm, r_orc).astype(np.float32))
    assert r_new.getstate() == r_old.getstate() == r_orc.getstate()                            # the same draws, in the same order
    # per-sample mode: batch[i] * mask_i, from the same draws
    r_ps = random.Random(seed)
    per = retrieve_masked_batch(batch, bm, r_ps, per_sample=True)
    assert r_ps.getstate() == r_new.getstate()
    for i in range(len(bm)):
        assert bc.same_bits(per[i], batch[i] * squares_to_mask(rects[i], batch.shape[1:]))
    used = rects[..., 2] != 0
    assert ((rects[used][:, 2:] == 20).all())
    if name == 'too_small':
        assert not used[:3].any() and used[3].any()
    if name == 'rows22':
        assert used[0].any() and np.isin(rects[0][used[0]][:, 0], (7, 8)).all() and np.isin(rects[0][used[0]][:, 1], (9, 10)).all() and not used[1].any()
    if name == 'last_draws_nothing':
        assert used[0].any() and used[1].any() and not used[2].any()
        assert bc.same_bits(got, batch) and not bc.same_bits(per, batch)


def test_draw_consumes_the_rng_as_the_reference_does():
    class Counting:
        def __init__(self):
            self.calls = []

        def randint(self, a, b):
            self.calls.append((a, b))
            return b
    rng = Counting()
    rects = draw_context_squares([(0, 63, 0, 63), (10, 30, 10, 30), (7, 28, 9, 30)], rng)
    # sample 0: the count (3), then (row, col) per square; sample 1: the count alone; sample 2: the count, then three squares at the last of two positions
    assert rng.calls == [(1, 3)] + [(0, 43), (0, 43)] * 3 + [(1, 3)] + [(1, 3)] + [(7, 8), (9, 10)] * 3
    assert (rects[0] == (43, 43, 20, 20)).all() and not rects[1].any() and (rects[2] == (8, 10, 20, 20)).all()
    # the module-level default is Python's `random`, as in the reference
    random.seed(9)
    a = draw_context_squares([(0, 63, 0, 63)] * 4)
    assert np.array_equal(a, draw_context_squares([(0, 63, 0, 63)] * 4, random.Random(9)))


def test_an_empty_brain_mask_keeps_raising():
    bm = _box_mask(32, 32, [(0, 31, 0, 31), (0, 31, 0, 31)])
    bm[1] = False
    with pytest.raises(ValueError):
        retrieve_masked_batch(np.ones(bm.shape, np.float32), bm, random.Random(0))
    with pytest.raises(ValueError):
        draw_context_squares(_boxes(bm), random.Random(0))


def test_check_rects_refuses_what_the_kernel_may_not_see():
    ok = bc.rects_case('mixed', 8, (26, 30, 1))
    assert np.array_equal(check_rects(ok, 8, 26, 30), ok) and check_rects(ok.astype(np.int64), 8, 26, 30).dtype == np.int32
    for bad in ((0, 11, 5, 20), (22, 0, 5, 4), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, -2, 2), (0, 0, 2, 0)):
        r = ok.copy()
        r[3, 1] = bad
        with pytest.raises(ValueError):
            check_rects(r, 8, 26, 30)
    r = ok.copy()
    r[3, 1] = (99, 99, 0, 99)                                     # height 0: unused, whatever else it holds
    check_rects(r, 8, 26, 30)
    for shape_bad in (ok[:7], ok.reshape(8, 12), ok[:, :2], ok.astype(np.float32)):
        with pytest.raises(ValueError):
            check_rects(shape_bad, 8, 26, 30)


def test_the_three_entries_are_declared_bound_and_exported():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'uad_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(uad_[a-z0-9_]+)\s*\(', header))
    version_script = open(os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc', 'libuad_hip.map')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
        assert name in version_script and re.search(r'global:\s*uad_\*;', version_script)
    from unsupervised_anomaly_detection_brain_mri_amd import build
    assert 'uad_batch.hip' in build.SOURCES and build.EXTRA_FLAGS['uad_batch.hip'] == ['-ffp-contract=off']


def test_device_dataset_arguments_that_need_no_device():
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import DeviceDataset
    imgs, sets = np.zeros((4, 8, 8, 1), np.float32), np.zeros(4, np.int64)
    for bad in (-0.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='instance_noise'):
            DeviceDataset(imgs, sets, instance_noise=bad)           # refused before any device is touched
    assert DeviceDataset.NOISE_STREAM not in range(8)               # the trainers' noise jobs of a step use stream ids 0 .. 7
