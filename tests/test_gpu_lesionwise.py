"""GPU: the device 3-D labelling (uad_cc_label), the lesion-wise detection counts built on it (uad_detection_rate), the threshold at a given
precision read off the device sort (uad_scores_threshold_at_precision) and the lesion-wise keys of Evaluation._score_diffs, against
scipy.ndimage.label with the full 3x3x3 structure, the host Evaluation.compute_detection_rate (pinned by tests/test_host_cpu.py) and
Metrics.compute_prc.  Everything compared is an integer, or a float computed on the host from identical integers: all comparisons are exact."""
import types

import numpy as np
import pytest
import scipy.ndimage
import torch

from tests.scoring_cases import host_threshold

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.trainers import Metrics
    from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation
except Exception:
    DeviceOps = None

FULL = np.ones((3, 3, 3), bool)
SHAPES = [(7, 37, 53), (41, 128, 128), (110, 256, 256)]


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def expected_labels(mask, slab=0):
    """1 + the smallest linear index of the voxel's scipy component, slab by slab; also the number of components."""
    mask = np.asarray(mask) != 0
    D = mask.shape[0]
    slab = D if slab <= 0 or slab >= D else slab
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    out = np.zeros(mask.shape, np.int32)
    total = 0
    for s0 in range(0, D, slab):
        lab, n = scipy.ndimage.label(mask[s0:s0 + slab], structure=FULL)
        total += n
        if n:
            mins = np.asarray(scipy.ndimage.minimum(idx[s0:s0 + slab], lab, index=np.arange(1, n + 1))).astype(np.int64)
            out[s0:s0 + slab] = np.where(lab > 0, mins[np.maximum(lab, 1) - 1] + 1, 0)
    return out, total


def check(eng, mask, slab=0):
    got = eng.cc_label(mask, slab=slab)
    assert got.dtype == torch.int32 and tuple(got.shape) == mask.shape
    got = got.cpu().numpy()
    want, n = expected_labels(mask, slab)
    # equal label arrays: the same partition AND every label = 1 + the minimum linear index of its scipy component
    assert np.array_equal(got, want), f'{int((got != want).sum())} voxels differ'
    assert len(np.unique(got[got > 0])) == n
    return got, n


def blobs(rng, shape, fill):
    """Smooth random blobs at about `fill` foreground (a box-filtered uniform field thresholded at its quantile)."""
    f = scipy.ndimage.uniform_filter(rng.random(shape).astype(np.float32), 3, mode='constant')
    return f > np.quantile(f, 1.0 - fill)


def diagonal_chain(shape):
    v = np.zeros(shape, bool)
    T = max(shape)
    t = np.arange(T)
    z, y, x = (np.round(t * (s - 1) / max(T - 1, 1)).astype(int) for s in shape)       # every coordinate moves by at most 1 per step
    v[z, y, x] = True
    return v


def spiral(h, w):
    """One-pixel-wide rectangular spiral with one background pixel between its arms: a single 8-connected component."""
    g = np.zeros((h, w), bool)
    y, x, dy, dx = 0, 0, 0, 1
    g[0, 0] = True

    def blocked(y, x, dy, dx):
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= y1 < h and 0 <= x1 < w) or g[y1, x1]:
            return True
        return 0 <= y2 < h and 0 <= x2 < w and g[y2, x2]
    while True:
        if blocked(y, x, dy, dx):
            dy, dx = dx, -dy                                   # turn right
            if blocked(y, x, dy, dx):
                return g
        y, x = y + dy, x + dx
        g[y, x] = True


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('fill', [0.02, 0.30, 0.60])
def test_cc_label_random_blobs(eng, shape, fill):
    rng = np.random.default_rng(int(fill * 100) + shape[0])
    mask = blobs(rng, shape, fill)
    _, n = check(eng, mask)
    assert n >= 1


@pytest.mark.parametrize('shape', SHAPES)
def test_cc_label_structured_volumes(eng, shape):
    D, H, W = shape
    chain = diagonal_chain(shape)
    got, n = check(eng, chain)
    assert n == 1 and got.max() == 1                            # starts at voxel 0
    sp = np.zeros(shape, bool)
    sp[D // 2] = spiral(H, W)
    assert sp.sum() > 4 * max(H, W)                             # an arm far longer than any tile edge
    _, n = check(eng, sp)
    assert n == 1
    z, y, x = np.indices(shape)
    _, n = check(eng, (x + y + z) % 2 == 0)                     # 26-connected: one component (6-connectivity would give none joined)
    assert n == 1
    got, n = check(eng, np.zeros(shape, bool))
    assert n == 0 and not got.any()
    got, n = check(eng, np.ones(shape, bool))
    assert n == 1 and (got == 1).all()


@pytest.mark.parametrize('h,w', [(37, 53), (128, 128), (256, 256)])
def test_cc_label_single_slice(eng, h, w):
    rng = np.random.default_rng(h)
    check(eng, blobs(rng, (1, h, w), 0.3))
    check(eng, spiral(h, w)[None])
    # non-binary float input: non-zero is foreground, the sign does not matter
    v = (rng.standard_normal((1, h, w)) * (rng.random((1, h, w)) < 0.3)).astype(np.float32)
    assert np.array_equal(eng.cc_label(v).cpu().numpy(), expected_labels(v != 0)[0])


def test_cc_label_slab_groups_are_independent(eng):
    shape = (41, 128, 128)
    rng = np.random.default_rng(41)
    mask = blobs(rng, shape, 0.02)
    mask[12:30, 60:64, 60:64] = True                            # crosses slice 19 / 20
    got, _ = check(eng, mask, slab=20)                           # scipy on slices 0:20, 20:40, 40:41 separately
    assert got[19, 61, 61] != got[20, 61, 61] and got[19, 61, 61] > 0 and got[20, 61, 61] > 0          # counted twice
    whole, _ = check(eng, mask, slab=0)
    assert whole[19, 61, 61] == whole[20, 61, 61]
    assert np.array_equal(eng.cc_label(mask, slab=41).cpu().numpy(), whole) and np.array_equal(eng.cc_label(mask, slab=100).cpu().numpy(), whole)
    check(eng, mask, slab=1)
    check(eng, mask, slab=3)                                     # group boundaries inside the 4-slice tiles


def test_cc_label_is_deterministic(eng):
    rng = np.random.default_rng(5)
    mask = torch.from_numpy(blobs(rng, (110, 256, 256), 0.30).astype(np.float32)).to(eng.device)
    a = eng.cc_label(mask)
    b = eng.cc_label(mask)
    assert torch.equal(a, b)
    assert torch.equal(eng.cc_label(mask, slab=20), eng.cc_label(mask, slab=20))


# ---------------------------------------------------------------------------------------------------------------- detection rate
def both(eng, pred, gt):
    want = tuple(int(v) for v in Evaluation.compute_detection_rate(pred, gt))
    got = eng.detection_rate(pred, gt)
    assert all(type(v) is int for v in got)
    assert got == want, (got, want)
    return want


def test_detection_rate_constructed_cases(eng):
    # the case of tests/test_host_cpu.py: hit lesion, 27-voxel false blob (the 1-voxel one is ignored), missed lesion
    gt = np.zeros((25, 32, 32), int); gt[3:6, 5:9, 5:9] = 1; gt[22:24, 20:23, 20:23] = 1
    pr = np.zeros_like(gt); pr[4:7, 6:10, 6:10] = 1; pr[10:13, 1:4, 1:4] = 1; pr[0, 0, 0] = 1
    assert both(eng, pr, gt) == (1, 1, 1)
    # predicted components of exactly 7 and exactly 8 voxels, neither touching a lesion: only the 8-voxel one is a false positive
    pr = np.zeros((25, 32, 32), int); pr[2, 2, 2:9] = 1; pr[8, 10, 10:18] = 1
    gt = np.zeros_like(pr); gt[15:17, 20:24, 20:24] = 1
    assert both(eng, pr, gt) == (0, 1, 1)
    # an intersection whose first voxel lies in a predicted component of fewer than 8 voxels: still a TP, still clears its lesion
    pr = np.zeros((25, 32, 32), int); pr[5, 5, 5:8] = 1
    gt = np.zeros_like(pr); gt[4:8, 4:9, 4:9] = 1
    assert both(eng, pr, gt) == (1, 0, 0)
    # two intersection components inside one lesion: 2 TPs, the lesion is cleared once
    pr = np.zeros((25, 32, 32), int); pr[10:12, 4:7, 4:7] = 1; pr[10:12, 4:7, 12:15] = 1
    gt = np.zeros_like(pr); gt[9:13, 3:8, 3:16] = 1
    assert both(eng, pr, gt) == (2, 0, 0)
    # a lesion and its prediction across slice 19 / 20: counted in both chunks
    pr = np.zeros((41, 32, 32), int); pr[15:25, 8:12, 8:12] = 1
    gt = np.zeros_like(pr); gt[14:26, 7:13, 7:13] = 1
    assert both(eng, pr, gt) == (2, 0, 0)
    assert eng.detection_rate(pr, gt, slab=0) == (1, 0, 0)
    assert both(eng, np.zeros((3, 9, 9)), np.zeros((3, 9, 9))) == (0, 0, 0)


def lesion_pair(seed, shape=(110, 128, 128)):
    """Ground-truth blobs; the prediction keeps a shifted copy of about half of them and adds blobs and specks of its own."""
    rng = np.random.default_rng(seed)
    gt = blobs(rng, shape, 0.01)
    lab, n = scipy.ndimage.label(gt, structure=FULL)
    keep = np.zeros(n + 1, bool)
    keep[1:] = rng.random(n) < 0.5
    pred = np.roll(keep[lab], (1, 2, -1), axis=(0, 1, 2)) | blobs(rng, shape, 0.008) | (rng.random(shape) < 2e-4)
    return pred, gt


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_detection_rate_random_pairs(eng, seed):
    pred, gt = lesion_pair(seed)
    want = both(eng, pred, gt)
    assert min(want) > 0, want                                  # the comparison cannot pass on zeros
    assert eng.detection_rate(torch.from_numpy(pred).to(eng.device), torch.from_numpy(gt).to(eng.device)) == want


# ---------------------------------------------------------------------------------------------------------------- threshold at precision
@pytest.mark.parametrize('n,levels', [(1000, 17), (300000, 4096), (2000003, 0)])
def test_threshold_at_precision_matches_host_formula(eng, n, levels):
    rng = np.random.default_rng(n)
    p = rng.random(n).astype(np.float32)
    y = rng.random(n) < np.where(p < 0.6, 0.98, 0.5)             # precision falls from ~0.79 at the lowest threshold to ~0.5: 0.7 is crossed mid-curve
    if levels:
        p = (np.floor(p * levels) / levels).astype(np.float32)   # ties
    sc = eng.scores(p, y)
    hit = 0
    for precision in (0.7, 0.75, 0.6, 0.55, 0.999, 0.01):
        want = host_threshold(p, y, precision)
        assert sc.threshold_at_precision(precision) == want, precision
        hit += want != float(p.min())
    assert hit >= 2                                             # not only the "first point qualifies" answer
    sc.close()
    # no point qualifies: the smallest threshold
    y1 = np.ones(64, bool); y1[3::7] = False                    # (the top score is a positive: every precision stays above 0.5)
    p1 = np.linspace(0.1, 0.9, 64).astype(np.float32)
    sc = eng.scores(p1, y1)
    assert sc.threshold_at_precision(0.5) == host_threshold(p1, y1, 0.5) == float(p1[0])
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- _score_diffs
def two_patients(eng):
    rng = np.random.default_rng(23)
    diffs, labels = [], []
    for k in range(2):
        shape = (44, 64, 64)
        lab = blobs(rng, shape, 0.01)
        lab[15:25, 8:12, 8:12] = True                           # a lesion across slice 19 / 20
        soft = scipy.ndimage.uniform_filter(lab.astype(np.float32), 3)
        d = soft * (rng.random(shape) < 0.7) * rng.random(shape) + 0.6 * blobs(rng, shape, 0.006) * rng.random(shape) \
            + 0.3 * (rng.random(shape) < 0.003)
        d = (np.round(d.astype(np.float32) * 512) / 512).astype(np.float32)         # exact zeros and ties, like masked residuals
        diffs.append(torch.from_numpy(d).to(eng.device)); labels.append(lab.astype(np.int64))
    return diffs, labels


@pytest.mark.parametrize('threshold', ['bestdice', 0.25])
def test_score_diffs_end_to_end(eng, threshold):
    diffs, labels = two_patients(eng)
    model = types.SimpleNamespace(engine=eng)
    ev = Evaluation._score_diffs(model, diffs, labels, {'threshold': threshold})
    # every pre-existing key, from the pieces the function calls
    d_all = torch.cat([d.reshape(-1) for d in diffs])
    ll = np.concatenate(labels).astype(bool)
    sc = eng.scores(d_all, ll.flatten())
    assert ev['diff_AUC'] == sc.auroc and ev['diff_AUPRC'] == sc.auprc
    assert (ev['bestDiceScore'], ev['bestThreshold']) == Metrics.compute_dice_curve_recursive_device(sc, granularity=10)
    t70_dev = sc.threshold_at_precision(0.7)
    sc.close()
    thr = ev['bestThreshold'] if threshold == 'bestdice' else threshold
    assert ev['thresholdType'] == threshold
    stacked = torch.cat(diffs, dim=0)
    pred = eng.cc_filter((stacked > float(thr)).to(torch.float32), 7).cpu().numpy() > 0
    assert ev['DiceScore'] == Metrics.dice(pred, ll)
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(2):
            sub, g = pred[44 * k:44 * (k + 1)], ll[44 * k:44 * (k + 1)]
            assert ev['DiceScorePerPatient'][k] == Metrics.dice(sub, g) and ev['PrecisionPerPatient'][k] == Metrics.precision(sub, g)
            assert ev['RecallPerPatient'][k] == Metrics.recall(sub, g)
    assert ev['Dice'] == ev['DiceScorePerPatient']
    # every new key, recomputed on the host from the downloaded residuals: compute_prc, scipy labelling, compute_detection_rate
    dd = stacked.cpu()
    t70 = host_threshold(dd.numpy().flatten(), ll.flatten(), 0.7)
    assert t70_dev == t70
    host_pred = Evaluation.filter_3d_connected_components((dd > float(thr)).numpy()) > 0
    assert np.array_equal(host_pred, pred)
    pred70 = Evaluation.filter_3d_connected_components((dd > float(t70)).numpy()) > 0 if threshold == 'bestdice' else host_pred
    want = np.zeros(3, np.int64)
    for k in range(2):
        want += Evaluation.compute_detection_rate(pred70[44 * k:44 * (k + 1)], ll[44 * k:44 * (k + 1)])
    print('lesion-wise counts', want, 'thr70', t70)
    assert (ev['TPCC'], ev['FPCC'], ev['FNCC']) == tuple(int(v) for v in want)
    assert want[0] > 0 and want[1] + want[2] > 0
    assert ev['TPRCC'] == want[0] / (want[0] + want[2]) and ev['PrecisionCC'] == want[0] / (want[0] + want[1])
    assert (ev['TP'], ev['FP'], ev['TN'], ev['FN']) == tuple(int(v) for v in Metrics.confusion_matrix(host_pred, ll))
    assert ev['TPR'] == Metrics.tpr(host_pred, ll) and ev['FPR'] == Metrics.tpr(host_pred, ll)               # FPR through tpr: sic (:490)
    assert ev['VD'] == Metrics.vd(host_pred, ll)
    for key in ('DiceScore', 'Precision', 'Recall'):
        assert ev[key + 'PerPatientMean'] == np.mean(ev[key + 'PerPatient']) and ev[key + 'PerPatientStd'] == np.std(ev[key + 'PerPatient'])
