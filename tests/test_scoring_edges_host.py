"""CPU: tests/scoring_cases.py -- the inputs and the exact host model that tests/test_gpu_scoring_edges.py holds the device scoring sort
to -- checked against oracle.scoring and trainers/Metrics.py, so the device test cannot pass against a wrong reference:
the scores are distinct and the midpoint thresholds separate them, the exact-Dice formula equals oracle.scoring.dice on thresholded
arrays, the -0.0 / +0.0 case is sensitive to a split, the oracle's own summation error at the large size is far below the 1e-12 bar,
the oracle and Metrics agree on single-class labels, Evaluation._score_diffs lives with the NaNs, and two deliberately wrong host models
(a scan that drops its carry, a sort that shifts one tile by one element) change the probes' expectations."""
import math
import types

import numpy as np
import pytest
import torch

from oracle import scoring as osc
from tests import scoring_cases as sc
from tests.test_lesionwise_host import _HostEngine
from unsupervised_anomaly_detection_brain_mri_amd.trainers import Metrics
from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation


def thresholded_dice(case, t):
    with np.errstate(divide='ignore', invalid='ignore'):
        return osc.dice((case.p.astype(np.float64) > t).astype(np.int64), case.y)


@pytest.mark.parametrize('n', sc.SMALL_SIZES)
def test_small_sizes_distinct_scores_and_exact_dice_formula(n):
    case = sc.distinct_case(n)
    m = case.model
    assert np.unique(case.p).size == n and case.p.dtype == np.float32
    assert m.P == case.y.sum() and (n < 2 or 0 < m.P < n)
    counts = np.arange(n + 1)
    ts = m.thresholds_for_counts(counts)                          # asserts strict separation in fp64
    assert np.array_equal(m.counts_above(ts), counts)
    want = m.dice_at_counts(counts)
    for c, t in zip(counts, ts):                                  # every probe: the formula IS the oracle's Dice of the thresholded array
        assert sc.same(want[c], thresholded_dice(case, t)), (n, c)
    assert np.array_equal(m.dice(ts), want, equal_nan=True)


def test_last_round_holds_a_digit_zero_key_next_to_invalid_lanes():
    """Every small size whose last tile ends inside a wave, from 255 on, has a real key with a zero low byte in that wave (smaller n have
    no such score among k / n); the value cases end in -inf, whose key's two low bytes are zero."""
    for n in sc.SMALL_SIZES:
        if n >= 255 and n % sc.WAVE:
            assert sc.partial_wave_has_digit0(sc.distinct_case(n).p), n
    for n in (4097, 5000):
        assert sc.partial_wave_has_digit0(sc.values_case(n).p)
    assert sc.BIG_N % sc.RS_TILE == 1 and sc.partial_wave_has_digit0(sc.big_distinct().p)
    # the restated key orders like the scores, descending, and +0.0 sorts before -0.0
    v = sc.VALUE_SET
    assert np.array_equal(np.argsort(sc.desc_key(v), kind='stable'), np.arange(v.size)[::-1])


def test_large_case_probes_and_formula_on_a_sample():
    case = sc.big_distinct()
    m = case.model
    counts = sc.big_counts()
    assert counts.size > 2000 > sc.DICE_CAP and counts.max() == sc.BIG_N
    for c in (1, 2047, 2048, 2049, sc.CARRY - 1, sc.CARRY, sc.CARRY + 1, 2 * sc.CARRY - 1, 2 * sc.CARRY, 2 * sc.CARRY + 1,
              sc.BIG_N - 2, sc.BIG_N - 1, sc.BIG_N):
        assert c in counts
    assert sc.BIG_N > 2 * sc.CARRY and -(-sc.BIG_N // sc.SC_BLOCK) > 2 * sc.SCAN_CHUNK          # three passes of the carry loop
    ts = m.thresholds_for_counts(counts)
    assert np.array_equal(m.counts_above(ts), counts)
    want = m.dice_at_counts(counts)
    for c in (1, 2048, sc.CARRY - 1, sc.CARRY, sc.CARRY + 1, 2 * sc.CARRY, 2 * sc.CARRY + 1, sc.BIG_N - 1, int(counts[777])):
        i = int(np.searchsorted(counts, c))
        assert want[i] == thresholded_dice(case, ts[i]), c


def test_large_ties_case_probes_run_ends():
    case = sc.big_ties()
    m = case.model
    assert (case.p == 0).sum() > 0.49 * sc.BIG_N
    ends = np.r_[np.nonzero(np.diff(m.ps))[0], m.n - 1]            # the run-closing positions
    assert 8000 < ends.size <= 8193
    assert m.ps[sc.CARRY - 1] == m.ps[sc.CARRY] == 0              # the zeros lie across the first carry boundary ...
    for lo in (0, sc.CARRY, 2 * sc.CARRY):                        # ... and every pass of the flag scan's carry loop has flags to place
        assert ((ends >= lo) & (ends < lo + sc.CARRY)).sum() >= 8
    cnt = m.counts_above(case.thresholds)
    assert set(cnt[cnt > 0] - 1) == set(ends) and (cnt == 0).sum() >= 1
    want = m.dice(case.thresholds)
    for i in (0, 1, 2000, 4096, 4097, 8192, 8193, 12000, case.thresholds.size - 2, case.thresholds.size - 1):
        assert sc.same(want[i], thresholded_dice(case, case.thresholds[i])), i


def _fsum_metrics(p, y):
    """AUROC / AUPRC from the oracle's own counts, the terms added exactly (math.fsum) instead of by numpy's pairwise sum."""
    tps, fps, npos = osc._sorted_counts(p, y)
    prec, rec = tps / (tps + fps), tps / npos
    ap = math.fsum(np.diff(np.r_[0.0, rec]) * prec)
    tpr, fpr = np.r_[0.0, tps / npos], np.r_[0.0, fps / (np.asarray(y).size - npos)]
    return math.fsum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0), ap


@pytest.mark.parametrize('which', ['distinct', 'ties'])
def test_reference_summation_spread_is_far_below_the_bar(which, capsys):
    """The 1e-12 bar of the device comparison rests on this: at n = 4 198 401 the oracle's value and the exact sum of the same terms differ
    by < 1e-13 relative (measured: about 1e-15 at most), so a device result within 1e-12 of the oracle is within ~1e-12 of the true sum."""
    case = sc.big_distinct() if which == 'distinct' else sc.big_ties()
    auc, ap = _fsum_metrics(case.p, case.y)
    s_auc, s_ap = abs(case.auroc - auc) / auc, abs(case.auprc - ap) / ap
    with capsys.disabled():
        print(f'\n[{which}] oracle-vs-fsum relative spread: AUROC {s_auc:.2e}, AUPRC {s_ap:.2e}')
    assert s_auc < 1e-13 and s_ap < 1e-13
    assert 0.0 < case.auroc < 1.0 and 0.0 < case.auprc < 1.0
    with np.errstate(invalid='ignore'):                           # threshold_at_precision has non-trivial answers at this size
        assert len({sc.host_threshold(case.p, case.y, q) for q in sc.PRECISIONS} - {float(case.p.min())}) >= 2


@pytest.mark.parametrize('n', [4097, 5000])
def test_value_case_is_sensitive_to_splitting_the_zeros(n):
    case = sc.values_case(n)
    m = case.model
    assert set(case.p.view(np.uint32)) == set(sc.VALUE_SET.view(np.uint32))
    assert np.isfinite(sc.VALUE_SET[[1, 3, 6, 7, 10]]).all() and (np.abs(sc.VALUE_SET[[3, 6, 7]]) < np.finfo(np.float32).tiny).all()      # denormals stay denormal
    with np.errstate(invalid='ignore'):
        split = osc.average_precision(case.p_split, case.y), osc.auroc(case.p_split, case.y)
    assert abs(split[0] - case.auprc) > 1e-6 * case.auprc and abs(split[1] - case.auroc) > 1e-6 * case.auroc
    (o_auc, o_ap), (h_auc, h_ap) = sc.host_metrics(case.p, case.y)
    assert sc.same(h_auc, o_auc, sc.REL) and sc.same(h_ap, o_ap, sc.REL) and np.isfinite([o_auc, o_ap]).all()
    # every threshold: the model equals the oracle's Dice of the thresholded array
    want = m.dice(case.thresholds)
    for t, w in zip(case.thresholds, want):
        assert sc.same(w, thresholded_dice(case, t)), t
    with np.errstate(invalid='ignore'):
        assert len({sc.host_threshold(case.p, case.y, q) for q in sc.PRECISIONS}) >= 2


def test_infinite_scores_do_not_tie_in_the_reference():
    """np.diff of two equal infinities is nan, and nan != 0: the oracle and Metrics give every +-inf score a threshold of its own, unlike
    every finite tie.  The device follows (closes_run in csrc/uad_eval.hip); this pins what it follows."""
    p = np.array([np.inf, np.inf, 1.0, 1.0, -np.inf, -np.inf], np.float32)
    y = np.array([0, 1, 1, 0, 1, 0], bool)
    with np.errstate(invalid='ignore'):
        tps, fps, _ = osc._sorted_counts(p, y)
        thr = Metrics.compute_prc(p.astype(np.float64), y)[3]
    assert tps.tolist() == [0, 1, 2, 3, 3] and fps.tolist() == [1, 1, 2, 2, 3]
    assert thr.tolist() == [-np.inf, -np.inf, 1.0, np.inf, np.inf]


@pytest.mark.parametrize('name,p,y', sc.single_class_cases(), ids=[c[0] for c in sc.single_class_cases()])
def test_single_class_oracle_and_metrics_agree(name, p, y):
    (o_auc, o_ap), (h_auc, h_ap) = sc.host_metrics(p, y)
    assert sc.same(o_auc, h_auc, sc.REL) and sc.same(o_ap, h_ap, sc.REL)
    if name.startswith('neg'):
        assert np.isnan(o_auc) and np.isnan(o_ap)
    elif name.startswith('pos'):
        assert np.isnan(o_auc) and o_ap == pytest.approx(1.0, rel=sc.REL)
    else:
        assert o_auc == 0.5 and o_ap == pytest.approx(y.mean(), rel=sc.REL)
    m = sc.SortedModel(p, y)
    ts = np.r_[np.unique(p), -1.0, 2.0, 0.3]
    with np.errstate(divide='ignore', invalid='ignore'):
        for t, w in zip(ts, m.dice(ts)):
            ref = osc.dice((p.astype(np.float64) > t).astype(np.int64), y)
            assert sc.same(w, ref) and sc.same(w, Metrics.dice(p.astype(np.float64) > t, y)), t
    if name.startswith('neg'):                                    # nothing predicted and nothing labelled: 0/0
        assert np.isnan(m.dice([2.0])[0]) and m.dice([-1.0])[0] == 0.0


@pytest.mark.parametrize('positive', [False, True])
def test_score_diffs_lives_with_single_class_labels(positive):
    """A healthy-only test set (and its mirror) on the host stand-in engine: AUROC (and AUPRC without positives) are nan, the Dice sweep
    and the lesion-wise keys go through.  tests/test_gpu_scoring_edges.py holds the device engine to this dictionary."""
    diffs, labels = sc.healthy_patients(positive)
    model = types.SimpleNamespace(engine=_HostEngine())
    with np.errstate(divide='ignore', invalid='ignore'):
        ev = Evaluation._score_diffs(model, [torch.from_numpy(d) for d in diffs], labels, {'threshold': 'bestdice'})
        d_all, l_all = np.concatenate([d.reshape(-1) for d in diffs]).astype(np.float64), np.concatenate([l.reshape(-1) for l in labels])
        best = Metrics.compute_dice_curve_recursive(d_all, l_all, granularity=10)
    assert np.isnan(ev['diff_AUC'])
    assert np.isnan(ev['diff_AUPRC']) if not positive else ev['diff_AUPRC'] == pytest.approx(1.0, rel=sc.REL)
    assert sc.same(ev['bestDiceScore'], best[0]) and ev['bestThreshold'] == best[1]
    if positive:
        assert ev['bestDiceScore'] > 0 and (ev['TPCC'], ev['FNCC']) != (0, 0) and ev['FP'] == ev['TN'] == 0
    else:
        # the sweep's first threshold above every score predicts nothing: Dice 0/0, and numpy's argmax picks the nan
        assert np.isnan(ev['bestDiceScore']) and ev['bestThreshold'] >= d_all.max()
        assert (ev['TPCC'], ev['FNCC'], ev['TP'], ev['FN']) == (0, 0, 0, 0) and ev['TPRCC'] == 0.0 and np.isnan(ev['TPR']) and np.isnan(ev['VD'])


# ---------------------------------------------------------------------------------------------------------------- wrong host models
def test_mutation_dropped_scan_carry_changes_the_position_probes():
    """A scan whose single-block phase forgets the carry (every chunk of 1024 block sums restarts at 0) gives prefix sums that miss the
    first 1024 * 2048 labels' total behind the boundary: the expected Dice changes at every probe count > 2 097 152, so the device
    comparison at those counts (test_large_distinct_positions) would fail for such a kernel."""
    m = sc.big_distinct().model
    counts = sc.big_counts()
    wrong = m.ctp.copy()
    wrong[sc.CARRY:2 * sc.CARRY] -= m.ctp[sc.CARRY - 1]
    wrong[2 * sc.CARRY:] -= m.ctp[2 * sc.CARRY - 1]
    good, bad = m.dice_at_counts(counts), m.dice_at_counts(counts, ctp=wrong)
    changed = good != bad
    assert np.array_equal(changed, counts > sc.CARRY)              # count c reads tp[c - 1]
    for c in (sc.CARRY + 1, 2 * sc.CARRY, 2 * sc.CARRY + 1, sc.BIG_N):
        assert changed[np.searchsorted(counts, c)]
    assert not changed[np.searchsorted(counts, sc.CARRY)]


@pytest.mark.parametrize('n', [s for s in sc.SMALL_SIZES if s >= 2])
def test_mutation_shifted_tile_changes_the_small_size_probes(n):
    """A scatter that places one tile's elements one slot late (the first tile rotated by one): the all-count Dice probes of
    test_small_sizes_exact change."""
    m = sc.distinct_case(n).model
    ys = m.ys.copy()
    e = min(n, sc.RS_TILE)
    ys[:e] = np.roll(ys[:e], 1)
    counts = np.arange(n + 1)
    good, bad = m.dice_at_counts(counts), m.dice_at_counts(counts, ctp=np.cumsum(ys, dtype=np.int64))
    assert (good != bad).any()
