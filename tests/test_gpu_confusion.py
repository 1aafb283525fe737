"""GPU: the per-segment confusion counts (uad_confusion_by_segment, csrc/uad_confusion.hip) through engine.confusion_counts and through the raw
C entry, held to the numpy statement utils/confusion.py (itself held to trainers/Metrics.py by tests/test_confusion_host.py) with `==` on
int64: every case of tests/confusion_cases.py (segment starts on every 16-byte phase of the values and 4-byte phase of the labels, both bases
shifted off their alignment, empty segments, voxels outside every segment, NaN / inf / -0.0 / denormal predictions, one-class labels), a
segment of 3 000 001 voxels whose workgroups take several tiles each, a reused output, the Dice of engine.scores at the same threshold, the
error codes of the contract, and Evaluation._score_diffs against the host stand-in engine, key by key.  tests/test_confusion_kernels_host.py
runs the same cases on the kernel source compiled for the host."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import confusion_cases as cc
from tests import scoring_cases as sc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, confusion
except Exception:
    DeviceOps = None


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def shifted(eng, a, shift, dtype):
    """a device copy of `a` whose base lies `shift` elements behind a fresh allocation's"""
    buf = torch.empty(a.size + shift + 16, device=eng.device, dtype=dtype)
    buf[shift:shift + a.size] = torch.from_numpy(a).to(eng.device)
    return buf[shift:shift + a.size]


def raw(eng, pred, thr, gt, n, offsets, n_seg, max_len, counts):
    return eng.lib.uad_confusion_by_segment(C.c_void_p(pred), float(thr), C.c_void_p(gt), n, C.c_void_p(offsets), n_seg, max_len, C.c_void_p(counts),
                                            eng._stream())


def raw_counts(eng, case, thr, pred, gt):
    """the C entry on the case's whole arrays and its offsets table; the output is garbage before the call"""
    off = torch.from_numpy(case.offsets).to(eng.device)
    n_seg = case.offsets.size - 1
    counts = torch.full((n_seg, 4), -7, device=eng.device, dtype=torch.int64)
    _lib.check(raw(eng, pred.data_ptr(), thr, gt.data_ptr(), case.pred.size, off.data_ptr(), n_seg, int(np.diff(case.offsets).max()), counts.data_ptr()))
    return counts.cpu().numpy()


def check_case(eng, case):
    pred, gt = shifted(eng, case.pred, case.pred_shift, torch.float32), shifted(eng, case.gt, case.gt_shift, torch.uint8)
    assert case.pred.size == 0 or (pred.data_ptr() % 16 == 4 * case.pred_shift and gt.data_ptr() % 16 == case.gt_shift)
    a, b = int(case.offsets[0]), int(case.offsets[-1])
    for thr in cc.THRESHOLDS:
        want = cc.statement(case, thr)
        got = raw_counts(eng, case, thr, pred, gt)
        assert np.array_equal(got, want), (case.name, thr, 'raw', got.tolist(), want.tolist())
        # the engine counts segments that cover its arrays: the voxels outside are cut off, which shifts both bases once more
        got = eng.confusion_counts(pred[a:b], gt[a:b], np.diff(case.offsets), thr)
        assert got.dtype == np.int64 and np.array_equal(got, want), (case.name, thr, 'engine', got.tolist(), want.tolist())


@pytest.mark.parametrize('case', cc.prefix_cases() + cc.small_cases() + cc.class_cases(), ids=lambda c: c.name)
def test_cases_equal_the_statement(eng, case):
    check_case(eng, case)


def test_every_base_alignment_equals_the_statement(eng):
    for case in cc.shift_cases():
        check_case(eng, case)


def test_host_arrays_and_label_dtypes(eng):
    case = cc.prefix_cases()[1]
    lengths = np.diff(case.offsets)
    want = cc.statement(case, 0.5)
    for gt in (case.gt, case.gt.astype(np.int64) - 3 * (case.gt == 2), case.gt != 0, torch.from_numpy(case.gt.astype(np.int32)),
               torch.from_numpy(case.gt != 0), torch.from_numpy(case.gt).to(eng.device)):
        assert np.array_equal(eng.confusion_counts(case.pred, gt, lengths, 0.5), want)
    assert np.array_equal(eng.confusion_counts(case.pred.reshape(1, -1), case.gt.reshape(-1, 1), list(lengths), 0.5), want)
    empty = eng.confusion_counts(case.pred[:0], case.gt[:0], [], 0.5)
    assert empty.shape == (0, 4) and empty.dtype == np.int64
    for bad in (dict(lengths=lengths[:-1]), dict(lengths=-lengths), dict(lengths=lengths.astype(np.float64)), dict(gt=case.gt.astype(np.float32)),
                dict(gt=case.gt[:-1]), dict(lengths=np.r_[np.zeros(65535, np.int64), lengths])):
        kw = dict(pred=case.pred, gt=case.gt, lengths=lengths)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.confusion_counts(kw['pred'], kw['gt'], kw['lengths'], 0.5)


def test_long_segment_strides_over_tiles_and_output_reuse(eng):
    n_long, n_short = 3_000_001, 77
    rng = np.random.default_rng(5)
    pred = cc.PRED_VALUES[rng.integers(0, cc.PRED_VALUES.size, n_long + n_short)]
    gt = np.where(rng.random(pred.size) < 0.02, 255, 0).astype(np.uint8)
    lengths = [n_long, n_short]
    want = confusion.confusion_counts(pred, gt, lengths, 0.0)
    assert -(-n_long // cc.T) == 367                          # the library gives a segment one workgroup per four tiles: 92 here, each strides
    pd, gd = torch.from_numpy(pred).to(eng.device), torch.from_numpy(gt).to(eng.device)
    assert np.array_equal(eng.confusion_counts(pd, gd, lengths, 0.0), want)
    # the same call twice on one output: no stale counts; then another threshold on it
    case = types.SimpleNamespace(pred=pred, offsets=np.array([0, n_long, n_long + n_short], np.int64))
    off = torch.from_numpy(case.offsets).to(eng.device)
    counts = torch.full((2, 4), 12345, device=eng.device, dtype=torch.int64)
    for thr in (0.0, 0.0, 0.5):
        _lib.check(raw(eng, pd.data_ptr(), thr, gd.data_ptr(), pred.size, off.data_ptr(), 2, n_long, counts.data_ptr()))
        assert np.array_equal(counts.cpu().numpy(), want if thr == 0.0 else confusion.confusion_counts(pred, gt, lengths, 0.5))
    # a max_seg_len that is too small sizes the grid only
    _lib.check(raw(eng, pd.data_ptr(), 0.0, gd.data_ptr(), pred.size, off.data_ptr(), 2, 1, counts.data_ptr()))
    assert np.array_equal(counts.cpu().numpy(), want)


def test_dice_from_counts_equals_the_sorted_scores_dice(eng):
    """Raw residuals at a threshold t: both sides divide the same integers once in fp64."""
    case = sc.distinct_case(8193)
    dev = eng.scores(case.p, case.y)
    for t in (0.25, 0.5, 0.0, 0.999):
        tp, fp, fn, _ = (int(v) for v in eng.confusion_counts(case.p, case.y, [case.p.size], t)[0])
        with np.errstate(divide='ignore', invalid='ignore'):
            want = np.float64(2 * tp) / np.float64(2 * tp + fp + fn)
        got = dev.dice_at([float(np.float32(t))])[0]
        assert got == want and tp > 0
        assert confusion.metrics_from_counts(np.array([tp, fp, fn, 0]))['dice'] == got
    dev.close()


def test_error_codes(eng):
    pred = torch.zeros(64, device=eng.device)
    gt = torch.zeros(64, device=eng.device, dtype=torch.uint8)
    off = torch.tensor([0, 32, 64, 0], device=eng.device, dtype=torch.int64)
    counts = torch.full((3, 4), 5, device=eng.device, dtype=torch.int64)
    p, g, o, c = pred.data_ptr(), gt.data_ptr(), off.data_ptr(), counts.data_ptr()
    ok = lambda **kw: raw(eng, **{**dict(pred=p, thr=0.0, gt=g, n=64, offsets=o, n_seg=2, max_len=32, counts=c), **kw})
    assert ok() == _lib.UAD_OK
    assert ok(n_seg=0, counts=None) == _lib.UAD_OK
    for kw in (dict(pred=None), dict(gt=None), dict(offsets=None), dict(counts=None), dict(n=-1), dict(n_seg=-1), dict(max_len=-1), dict(n_seg=65536),
               dict(pred=p + 2), dict(offsets=o + 4), dict(counts=c + 4)):
        assert ok(**kw) == 1, kw                              # UAD_ERR_INVALID
        assert b'confusion_by_segment' in eng.lib.uad_last_error()
    assert ok(n=2 ** 31) == 3                                 # UAD_ERR_UNSUPPORTED, before anything is launched
    assert ok(n=2 ** 31 - 1, offsets=o + 16, n_seg=1, max_len=0) == _lib.UAD_OK      # the largest n: the one segment [64, 0) is empty, nothing is read
    torch.cuda.synchronize(eng.device)
    assert counts.cpu().numpy()[0].tolist() == [0, 0, 0, 0]
    counts.fill_(5)
    assert ok(n=0, pred=None, gt=None, offsets=None) == _lib.UAD_OK        # n == 0: zeroed, nothing launched
    assert counts.cpu().numpy()[:2].tolist() == [[0, 0, 0, 0]] * 2 and counts.cpu().numpy()[2].tolist() == [5] * 4


def same_value(g, w):
    if isinstance(w, list):
        return isinstance(g, list) and len(g) == len(w) and all(same_value(a, b) for a, b in zip(g, w))
    if type(g) is not type(w):
        return False
    return g == w or (isinstance(w, (float, np.floating)) and np.isnan(g) and np.isnan(w))


def two_patients():
    """Two small patients of 24 and 17 slices: a detected lesion, a missed one, a false blob, sparse speckle on an exactly-zero background."""
    rng = np.random.default_rng(23)
    diffs, labels = [], []
    for k, slices in enumerate((24, 17)):
        lab = np.zeros((slices, 32, 32), bool)
        lab[2:6, 4:10, 4:10] = True
        lab[10:12, 22:25, 22:25] = True
        d = (rng.random(lab.shape) * 0.2 * (rng.random(lab.shape) < 0.01)).astype(np.float32)
        d[3:7, 5:11, 5:11] += np.float32(0.5 + 0.1 * k)
        d[12:15, 2:6, 24:29] += np.float32(0.45)
        diffs.append(d)
        labels.append(lab.astype(np.int64))
    return diffs, labels


def score_both(eng, diffs, labels, options):
    from tests.test_lesionwise_host import _HostEngine
    assert not hasattr(_HostEngine, 'confusion_counts')
    with np.errstate(divide='ignore', invalid='ignore'):
        want = Evaluation._score_diffs(types.SimpleNamespace(engine=_HostEngine()), [torch.from_numpy(d) for d in diffs], labels, dict(options))
        got = Evaluation._score_diffs(types.SimpleNamespace(engine=eng), [torch.from_numpy(d).to(eng.device) for d in diffs], labels, dict(options))
    assert list(got) == list(want)
    for key, w in want.items():
        if key in ('diff_AUC', 'diff_AUPRC'):                 # the sorted-scores reductions: the bar of tests/test_gpu_scoring_edges.py
            assert sc.same(got[key], w, sc.REL), (key, got[key], w)
        else:
            assert same_value(got[key], w), (key, got[key], w)
    return got


@pytest.mark.parametrize('threshold', ['bestdice', 0.3])
def test_score_diffs_equals_the_host_route(eng, threshold):
    got = score_both(eng, *two_patients(), {'threshold': threshold})
    assert got['TP'] > 0 and got['FP'] > 0 and got['FN'] > 0 and got['TN'] > 0 and len(got['DiceScorePerPatient']) == 2


@pytest.mark.parametrize('positive', [False, True])
@pytest.mark.parametrize('threshold', ['bestdice', 0.3])
def test_score_diffs_single_class_equals_the_host_route(eng, positive, threshold):
    got = score_both(eng, *sc.healthy_patients(positive), {'threshold': threshold})
    assert np.isnan(got['VD']) if not positive else got['FP'] == 0
