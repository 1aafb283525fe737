"""Inputs of the per-segment confusion counts (uad_confusion_by_segment, csrc/uad_confusion.hip), shared by tests/test_confusion_host.py (the
numpy statement utils/confusion.py against trainers/Metrics.py), tests/test_confusion_kernels_host.py (the kernel source compiled for the host
against the statement) and tests/test_gpu_confusion.py (the device against the statement).

A case is (pred float32 [n], gt uint8 [n], offsets int64 [P + 1], pred_shift, gt_shift): segment s is [offsets[s], offsets[s + 1]) of the flat
arrays; voxels in front of offsets[0] and behind offsets[P] belong to no segment.  pred_shift (elements, 0 .. 3) and gt_shift (bytes, 0 .. 15) move the
bases of the two arrays off their allocation's alignment.  The lengths sit on the tile (UAD_SELECT_TILE = 8192) edges, two tiles and a bit, and
on 0, 1, 3 and 5, so that inside ONE call the segment starts fall on different 16-byte phases of the values and 4-byte phases of the labels;
a prefix of 1, 2 and 3 voxels and the base shifts move every start through all of them."""
import types

import numpy as np

from unsupervised_anomaly_detection_brain_mri_amd.utils.confusion import confusion_counts

T = 8192                                                     # UAD_SELECT_TILE
LENGTHS = (0, 1, 3, T - 1, T, T + 1, 5, 0, 2 * T + 1)
THRESHOLDS = (0.0, 0.5)
F32 = np.float32
PRED_VALUES = np.array([0.0, 1.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1.0, 0.5], F32)     # 1e-40: a denormal
GT_VALUES = np.array([0, 1, 2, 255], np.uint8)


def _case(name, pred, gt, offsets, pred_shift=0, gt_shift=0):
    offsets = np.asarray(offsets, np.int64)
    assert pred.dtype == F32 and gt.dtype == np.uint8 and pred.size == gt.size and 0 <= offsets[0] and offsets[-1] <= pred.size
    return types.SimpleNamespace(name=name, pred=pred, gt=gt, offsets=offsets, pred_shift=pred_shift, gt_shift=gt_shift)


def drawn(n, seed, positive=0.3):
    """n predictions drawn from PRED_VALUES and n label bytes from GT_VALUES (about `positive` of them non-zero)."""
    rng = np.random.default_rng(seed)
    pred = PRED_VALUES[rng.integers(0, PRED_VALUES.size, n)]
    gt = np.where(rng.random(n) < positive, GT_VALUES[rng.integers(1, GT_VALUES.size, n)], 0).astype(np.uint8)
    return pred, gt


def offsets_of(lengths, front=0):
    return front + np.r_[0, np.cumsum(np.asarray(lengths, np.int64))]


def prefix_cases():
    """LENGTHS in one call, and the same behind a segment of 1, 2 and 3 voxels."""
    out = []
    for k in range(4):
        lengths = ((k,) if k else ()) + LENGTHS
        pred, gt = drawn(sum(lengths), 100 + k)
        out.append(_case(f'prefix{k}', pred, gt, offsets_of(lengths)))
    return out


def shift_cases():
    """The values base 0 .. 3 elements and the label base 0 .. 15 bytes off their allocation's alignment, every pair."""
    pred, gt = drawn(sum(LENGTHS), 200)
    return [_case(f'shift{ps}_{gs}', pred, gt, offsets_of(LENGTHS), ps, gs) for ps in range(4) for gs in range(16)]


def small_cases():
    out = []
    out.append(_case('one_voxel', np.array([1.0], F32), np.array([255], np.uint8), [0, 1]))
    pred, gt = drawn(11, 301)
    out.append(_case('all_empty', pred, gt, [4, 4, 4, 4]))
    out.append(_case('no_segment_voxels', np.zeros(0, F32), np.zeros(0, np.uint8), [0, 0, 0]))
    # voxels outside every segment are positives of both arrays: counted, they would show as TP
    front, back = 5, 9
    pred, gt = drawn(front + sum(LENGTHS) + back, 302)
    pred[:front] = pred[pred.size - back:] = 1.0
    gt[:front] = gt[gt.size - back:] = 1
    out.append(_case('outside', pred, gt, offsets_of(LENGTHS, front)))
    return out


def class_cases():
    """One-class labels (all zero, all non-zero) and a prediction that is nowhere above either threshold: the nan scalars."""
    lengths = (3, T + 1, 0, 7)
    n = sum(lengths)
    pred, gt = drawn(n, 400)
    out = [_case('gt_all_zero', pred, np.zeros(n, np.uint8), offsets_of(lengths)),
           _case('gt_all_nonzero', pred, GT_VALUES[1 + np.arange(n) % 3], offsets_of(lengths))]
    quiet = np.array([0.0, -0.0, np.nan, -np.inf, -1e-40, -1.0], F32)
    out.append(_case('pred_all_false', quiet[np.arange(n) % quiet.size], gt, offsets_of(lengths)))
    out.append(_case('pred_all_false_gt_all_zero', quiet[np.arange(n) % quiet.size], np.zeros(n, np.uint8), offsets_of(lengths)))
    return out


def all_cases():
    return prefix_cases() + shift_cases() + small_cases() + class_cases()


def statement(case, thr):
    """utils.confusion.confusion_counts on the voxels the case's segments cover."""
    a, b = int(case.offsets[0]), int(case.offsets[-1])
    return confusion_counts(case.pred[a:b], case.gt[a:b], np.diff(case.offsets), thr)


def brute(case, thr):
    """{TP, FP, FN, TN} per segment by a plain loop over Python numbers: what the statement itself is held to."""
    out = np.zeros((case.offsets.size - 1, 4), np.int64)
    t = float(F32(thr))
    for s in range(case.offsets.size - 1):
        for i in range(int(case.offsets[s]), int(case.offsets[s + 1])):
            p, g = float(case.pred[i]) > t, int(case.gt[i]) != 0
            out[s, (0 if g else 1) if p else (2 if g else 3)] += 1
    return out
