"""GPU: the device scoring sort and scans (uad_scores_*, csrc/uad_eval.hip: 8-bit LSD radix sort, three-phase scans, flag compaction,
AUROC / AUPRC reduction, binary-search Dice, threshold at a precision) at the sizes and values where their code paths change, against
the exact host model of tests/scoring_cases.py (itself held to oracle.scoring and trainers/Metrics.py by tests/test_scoring_edges_host.py).

* Dice is compared with `==`: both sides divide the same integers once in fp64, so a Dice value at count c pins the sorted order's label
  prefix sum at c.  `positives` and `threshold_at_precision` are exact too.  AUROC / AUPRC: the oracle at rel 1e-12 (its own summation
  error at the large size is measured < 1e-13 by the host module).
* sizes: every n in {1, 2, 63..65, 255..257, 2047..2049, 4095..4097, 8191..8193} with all n + 1 thresholds (wave, scatter round, scan
  block and sort tile edges; a partly filled last round next to real digit-0 keys), and n = 2 * 2048 * 1024 + 4097 = 4 198 401, where
  scan_single_block_kernel's carry loop runs three times for the label scan and the flag scan (distinct scores: positions around both
  carry boundaries; heavy ties: the compaction's scan carries into an irregular flag pattern).
  NOT covered: the carry loop of the [digit][tile] histogram scan, which needs 256 * ceil(n / 4096) > 2 097 152, i.e. n > 33.5 M --
  out of reach of a seconds-long test.
* values: +-inf, +-3.4e38, denormals, -0.0 / +0.0 (one threshold), negative scores.
* single-class labels: nan where the reference's numpy divisions give nan, also through Evaluation._score_diffs.
* a handle reused across threshold batches of 64 / 65 / 129 and a threshold_at_precision call in between (it borrows the batch scratch)."""
import types

import numpy as np
import pytest
import torch

from tests import scoring_cases as sc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.trainers import Metrics
    from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation
except Exception:
    DeviceOps = None


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def check_dice(dev, thresholds, want):
    got = dev.dice_at(thresholds)
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert bad.size == 0, f'{bad.size} of {want.size} Dice probes differ, first at threshold {thresholds[bad[0]]!r}: {got[bad[0]]!r} != {want[bad[0]]!r}'


def check_scalars(dev, case):
    print(f'auroc {dev.auroc!r} (oracle {case.auroc!r})  auprc {dev.auprc!r} (oracle {case.auprc!r})')
    assert dev.positives == case.model.P
    assert sc.same(dev.auroc, case.auroc, sc.REL) and sc.same(dev.auprc, case.auprc, sc.REL)


def check_precision_thresholds(dev, case):
    with np.errstate(divide='ignore', invalid='ignore'):
        want = [sc.host_threshold(case.p, case.y, q) for q in sc.PRECISIONS]
    got = [dev.threshold_at_precision(q) for q in sc.PRECISIONS]
    assert got == want
    return want


@pytest.mark.parametrize('n', sc.SMALL_SIZES)
def test_small_sizes_exact(eng, n):
    case = sc.distinct_case(n)
    m = case.model
    dev = eng.scores(case.p, case.y)
    counts = np.arange(n + 1)
    check_dice(dev, m.thresholds_for_counts(counts), m.dice_at_counts(counts))
    check_scalars(dev, sc._with_oracle(case))
    check_precision_thresholds(dev, case)
    dev.close()


def test_large_distinct_positions(eng):
    case = sc.big_distinct()
    m = case.model
    dev = eng.scores(case.p, case.y)
    counts = sc.big_counts()
    check_dice(dev, m.thresholds_for_counts(counts), m.dice_at_counts(counts))
    check_scalars(dev, case)
    want = check_precision_thresholds(dev, case)
    assert len(set(want)) >= 2
    dev.close()


def test_large_heavy_ties(eng):
    case = sc.big_ties()
    dev = eng.scores(case.p, case.y)
    check_dice(dev, case.thresholds, case.model.dice(case.thresholds))
    check_scalars(dev, case)
    want = check_precision_thresholds(dev, case)
    assert len(set(want)) >= 2
    dev.close()


@pytest.mark.parametrize('n', [4097, 5000])
def test_special_values(eng, n):
    """The oracle's AUPRC changes when -0.0 gets a threshold of its own (asserted by the host module for these labels), so agreeing with it
    means the device merged the pair."""
    case = sc.values_case(n)
    dev = eng.scores(case.p, case.y)
    check_dice(dev, case.thresholds, case.model.dice(case.thresholds))
    check_scalars(dev, case)
    want = check_precision_thresholds(dev, case)
    assert len(set(want)) >= 2
    dev.close()


@pytest.mark.parametrize('name,p,y', sc.single_class_cases(), ids=[c[0] for c in sc.single_class_cases()])
def test_single_class_labels(eng, name, p, y):
    (o_auc, o_ap), (h_auc, h_ap) = sc.host_metrics(p, y)
    dev = eng.scores(p, y)
    print(name, 'device', dev.auroc, dev.auprc, 'oracle', o_auc, o_ap)
    assert dev.positives == y.sum()
    assert sc.same(dev.auroc, o_auc, sc.REL) and sc.same(dev.auroc, h_auc, sc.REL)
    assert sc.same(dev.auprc, o_ap, sc.REL) and sc.same(dev.auprc, h_ap, sc.REL)
    ts = np.r_[np.unique(p).astype(np.float64), -1.0, 2.0, 0.3]
    check_dice(dev, ts, sc.SortedModel(p, y).dice(ts))
    with np.errstate(divide='ignore', invalid='ignore'):
        host = Metrics.compute_dice_curve_recursive(p.astype(np.float64), y, granularity=5)
        assert dev.threshold_at_precision(0.7) == sc.host_threshold(p, y, 0.7)
    got = Metrics.compute_dice_curve_recursive_device(dev, granularity=5)
    assert sc.same(got[0], host[0]) and got[1] == host[1]
    dev.close()


@pytest.mark.parametrize('positive', [False, True])
def test_score_diffs_single_class_matches_host_path(eng, positive):
    """A healthy-only test set (and its mirror) through Evaluation._score_diffs: the device engine's dictionary equals the one of the host
    stand-in engine (pinned by tests/test_scoring_edges_host.py), nan for nan."""
    from tests.test_lesionwise_host import _HostEngine
    diffs, labels = sc.healthy_patients(positive)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = Evaluation._score_diffs(types.SimpleNamespace(engine=_HostEngine()), [torch.from_numpy(d) for d in diffs], labels, {})
        got = Evaluation._score_diffs(types.SimpleNamespace(engine=eng), [torch.from_numpy(d).to(eng.device) for d in diffs], labels, {})
    assert set(got) == set(want) and np.isnan(got['diff_AUC'])
    for key, w in want.items():
        g = got[key]
        if isinstance(w, list):
            assert len(g) == len(w) and all(sc.same(a, b) for a, b in zip(g, w)), key
        elif isinstance(w, str):
            assert g == w, key
        else:
            assert sc.same(g, w, sc.REL if key == 'diff_AUPRC' else 0.0), (key, g, w)


def test_handle_reuse_across_threshold_batches(eng):
    case = sc.distinct_case(8193)
    m = case.model
    dev = eng.scores(case.p, case.y)
    counts = np.random.default_rng(129).permutation(8194)[:129]
    ts, want = m.thresholds_for_counts(counts), m.dice_at_counts(counts)
    first = [dev.dice_at(ts[:k]) for k in (sc.DICE_CAP, sc.DICE_CAP + 1, 2 * sc.DICE_CAP + 1)]
    t70 = dev.threshold_at_precision(0.7)                          # writes into the batch's output scratch
    again = [dev.dice_at(ts[:k]) for k in (sc.DICE_CAP, sc.DICE_CAP + 1, 2 * sc.DICE_CAP + 1)]
    single = np.array([dev.dice_at([t])[0] for t in ts])
    for a, b in zip(first, again):
        assert np.array_equal(a, b) and np.array_equal(a, want[:a.size]) and np.array_equal(a, single[:a.size])
    assert t70 == dev.threshold_at_precision(0.7) == sc.host_threshold(case.p, case.y, 0.7)
    dev.close()
