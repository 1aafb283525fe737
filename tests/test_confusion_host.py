"""CPU: the host side of the per-segment confusion counts.  utils/confusion.py (the statement the device op is held to) against
trainers/Metrics.py on the boolean arrays of every case of tests/confusion_cases.py, bit for bit, nan for nan; the C-ABI name in the header, the
ctypes table and the version script; and the wiring of Evaluation._score_diffs: with an engine that has `confusion_counts`, the prediction
volume is never downloaded and the dictionary equals the plain host route's."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from tests import confusion_cases as cc
from tests.test_lesionwise_host import _HostEngine, _two_patients
from unsupervised_anomaly_detection_brain_mri_amd import _lib
from unsupervised_anomaly_detection_brain_mri_amd.trainers import Metrics
from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, confusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.prefix_cases() + cc.shift_cases()[:1] + cc.small_cases() + cc.class_cases()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float64 and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def boolean_arrays(case, thr, s):
    a, b = int(case.offsets[s]), int(case.offsets[s + 1])
    with np.errstate(invalid='ignore'):
        return case.pred[a:b] > np.float32(thr), case.gt[a:b] != 0


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_statement_and_scalars_equal_metrics_on_the_boolean_arrays(case):
    for thr in cc.THRESHOLDS:
        counts = cc.statement(case, thr)
        assert counts.dtype == np.int64 and counts.shape == (case.offsets.size - 1, 4)
        rows = [(counts[s], *boolean_arrays(case, thr, s)) for s in range(counts.shape[0])]
        a, b = int(case.offsets[0]), int(case.offsets[-1])
        with np.errstate(invalid='ignore'):
            rows.append((counts.sum(axis=0), case.pred[a:b] > np.float32(thr), case.gt[a:b] != 0))      # the overall values: column sums
        for row, P, G in rows:
            m = confusion.metrics_from_counts(row)
            with np.errstate(divide='ignore', invalid='ignore'):
                want = Metrics.confusion_matrix(P, G)
                assert tuple(int(v) for v in row) == (int(want[0]), int(want[1]), int(want[3]), int(want[2]))     # {TP, FP, FN, TN} against (TP, FP, TN, FN)
                assert all(type(g) is type(w) and g == w for g, w in zip(m['confusion'], want))
                for key, fn in (('dice', Metrics.dice), ('precision', Metrics.precision), ('recall', Metrics.recall), ('tpr', Metrics.tpr), ('vd', Metrics.vd)):
                    w = fn(P, G)
                    assert type(m[key]) is type(w) and same_bits(m[key], w), (case.name, thr, key, m[key], w)


def test_the_nan_scalars_appear_where_the_reference_divides_zero_by_zero():
    with np.errstate(all='raise'):                            # metrics_from_counts quiets its own divisions
        m = confusion.metrics_from_counts(np.array([0, 0, 0, 9], np.int64))
    assert all(np.isnan(m[k]) and type(m[k]) is np.float64 for k in ('dice', 'precision', 'recall', 'tpr', 'vd'))
    m = confusion.metrics_from_counts(np.array([0, 0, 4, 5], np.int64))
    assert np.isnan(m['precision']) and m['dice'] == 0.0 and m['recall'] == 0.0 and m['vd'] == 1.0
    m = confusion.metrics_from_counts(np.array([0, 3, 0, 5], np.int64))
    assert m['precision'] == 0.0 and m['dice'] == 0.0 and np.isnan(m['recall']) and np.isnan(m['vd'])


@pytest.mark.parametrize('case', cc.prefix_cases()[:2] + cc.small_cases() + cc.class_cases()[2:3], ids=lambda c: c.name)
def test_statement_against_a_plain_loop(case):
    for thr in cc.THRESHOLDS:
        assert np.array_equal(cc.statement(case, thr), cc.brute(case, thr))


def test_statement_validates_its_arguments():
    p, g = np.zeros(10, np.float32), np.zeros(10, np.uint8)
    for lengths in ([4, 5], [11], [-1, 11], [[5, 5]], [5.0, 5.0]):
        with pytest.raises(ValueError):
            confusion.confusion_counts(p, g, lengths)
    with pytest.raises(ValueError):
        confusion.confusion_counts(p, g[:9], [10])
    with pytest.raises(ValueError):
        confusion.metrics_from_counts(np.zeros(4))
    assert confusion.confusion_counts(p[:0], g[:0], []).shape == (0, 4)
    assert np.array_equal(confusion.confusion_counts(p.reshape(2, 5), g.reshape(2, 5).astype(bool), [10]), [[0, 0, 0, 10]])


def test_the_entry_is_declared_bound_and_exported():
    name = 'uad_confusion_by_segment'
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'uad_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(uad_[a-z0-9_]+)\s*\(', header))
    version_script = open(os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc', 'libuad_hip.map')).read()
    assert name in declared, f'{name} is not declared in include/uad_hip.h'
    assert name in _lib.SYMBOLS, f'{name} is missing from _lib.SYMBOLS'
    assert name in version_script and re.search(r'global:\s*uad_\*;', version_script)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    args = re.search(name + r'\s*\(([^)]*)\)', header).group(1)
    assert len(args.split(',')) == len(_lib.SYMBOLS[name][1]) == 9 and _lib.SYMBOLS[name][0] is ctypes.c_int
    from unsupervised_anomaly_detection_brain_mri_amd import build
    assert 'uad_confusion.hip' in build.SOURCES


# ---------------------------------------------------------------------------------------------------------------------------------
class _Resident:
    """A stand-in for a device-resident volume: what _score_diffs may do with the filtered prediction -- slice it per patient, hand it to the
    engine -- works; a download (.cpu() / .numpy()) raises unless it happens inside _lesionwise_keys, whose host fallback of the lesion-wise
    counts downloads one patient at a time on an engine without detection_rate."""

    def __init__(self, t):
        self._t = t
        self.shape = t.shape

    def __getitem__(self, key):
        return _Resident(self._t[key])

    def _download(self):
        f = sys._getframe(2)
        while f is not None and f.f_code.co_name != '_lesionwise_keys':
            f = f.f_back
        if f is None:
            raise AssertionError('the prediction volume was downloaded outside the lesion-wise host fallback')
        return self._t

    def cpu(self):
        return self._download()

    def numpy(self):
        return self._download().numpy()


class _CountingEngine(_HostEngine):
    """_HostEngine plus confusion_counts (the numpy statement) on a cc_filter result that cannot be downloaded."""
    calls = 0

    def cc_filter(self, volume, max_voxels=7):
        return _Resident(super().cc_filter(volume, max_voxels))

    def confusion_counts(self, pred, gt, lengths, thr=0.0):
        type(self).calls += 1
        assert isinstance(pred, _Resident)
        return confusion.confusion_counts(pred._t.numpy(), gt, lengths, thr)


def same_value(g, w):
    if isinstance(w, list):
        return isinstance(g, list) and len(g) == len(w) and all(same_value(a, b) for a, b in zip(g, w))
    if type(g) is not type(w):
        return False
    return g == w or (isinstance(w, (float, np.floating)) and np.isnan(g) and np.isnan(w))


@pytest.mark.parametrize('threshold', ['bestdice', 0.3])
def test_score_diffs_takes_the_counts_and_downloads_no_prediction(threshold):
    diffs, labels = _two_patients()
    diffs.append(diffs[0][:7] * 0)                           # a third patient of another slice count without a prediction: nan scalars
    labels.append(np.zeros((7, 32, 32), np.int64))
    _CountingEngine.calls = 0
    with np.errstate(divide='ignore', invalid='ignore'):
        want = Evaluation._score_diffs(types.SimpleNamespace(engine=_HostEngine()), diffs, labels, {'threshold': threshold})
        keep = {}
        got = Evaluation._score_diffs(types.SimpleNamespace(engine=_CountingEngine()), diffs, labels, {'threshold': threshold}, keep=keep)
    assert _CountingEngine.calls == 1 and isinstance(keep['pred_dev'], _Resident)
    assert list(got) == list(want)                           # the keys, in the order they are written
    for key, w in want.items():
        assert same_value(got[key], w), (key, got[key], w)
    assert np.isnan(got['PrecisionPerPatient'][2]) and got['TP'] > 0 and got['FP'] > 0 and got['FN'] > 0
    assert got['Dice'] is got['DiceScorePerPatient']
