"""Inputs and the exact host model for the size / value / label edges of the device scoring sort (uad_scores_*, csrc/uad_eval.hip).
Shared by tests/test_gpu_scoring_edges.py (device against this model) and tests/test_scoring_edges_host.py (this model against
oracle.scoring and trainers/Metrics.py on the CPU, so that the device test cannot pass against a wrong reference).

The exact probe.  With the scores sorted descending and tp = cumulative sum of the labels in that order, a threshold t with exactly
`c` scores above it has  dice(score > t, label) = 2 * tp[c - 1] / (c + P).  Both sides compute it from the same integers with one
correctly rounded fp64 division, so the comparison is `==`, and a Dice value at count c pins the sorted order's label prefix sum at c.
"""
import functools
import types

import numpy as np

from oracle import scoring as osc
from unsupervised_anomaly_detection_brain_mri_amd.trainers import Metrics

# the kernels' constants (csrc/uad_eval.hip); the sizes below are built around them
RS_TILE, RS_THREADS, SC_BLOCK, SCAN_CHUNK, WAVE, DICE_CAP = 4096, 256, 2048, 1024, 64, 64
CARRY = SC_BLOCK * SCAN_CHUNK                       # items one pass of scan_single_block_kernel's loop covers: 2 097 152

SMALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
BIG_N = 2 * CARRY + 4097                            # 4 198 401: three passes of the carry loop for the label and the flag scans
PRECISIONS = (0.7, 0.75, 0.6, 0.55, 0.999, 0.01)    # the levels of tests/test_gpu_lesionwise.py
REL = 1e-12                                         # the project's bar for the fp64 scalar metrics

F32 = np.float32
VALUE_SET = np.array([-np.inf, -3.4e38, -1.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 0.25, 1.0, 3.4e38, np.inf], F32)


def host_threshold(p, y, precision):
    _, prec, _, thr = Metrics.compute_prc(np.asarray(p, np.float64), np.asarray(y).astype(bool))
    return float(thr[np.argmax(prec <= precision)])


def same(a, b, rel=0.0):
    """a == b (within rel when given), nan equal to nan."""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a == b if rel == 0.0 or np.isinf(a) or np.isinf(b) else abs(a - b) <= rel * abs(b)


class SortedModel:
    """The host statement of what uad_scores_create holds: fp32 scores widened to fp64 and sorted descending, the labels in that order,
    their 64-bit cumulative sum."""

    def __init__(self, p, y):
        p = np.asarray(p).reshape(-1)
        assert p.dtype == F32 and not np.isnan(p).any()
        self.p = p.astype(np.float64)
        self.y = np.asarray(y).reshape(-1).astype(bool)
        self.n = self.p.size
        order = np.argsort(-self.p, kind='stable')
        self.ps, self.ys = self.p[order], self.y[order]
        self.ctp = np.cumsum(self.ys, dtype=np.int64)
        self.P = int(self.ctp[-1])

    def dice_at_counts(self, counts, ctp=None):
        """2 * tp[c - 1] / (c + P) for every count c of scores above the threshold; `ctp`: another prefix sum (the mutation checks)."""
        c = np.asarray(counts, np.int64)
        ctp = self.ctp if ctp is None else ctp
        tp = np.where(c > 0, ctp[np.maximum(c, 1) - 1], 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            return 2.0 * tp / (c + self.P)

    def counts_above(self, thresholds):
        return self.n - np.searchsorted(self.ps[::-1], np.asarray(thresholds, np.float64), side='right')

    def dice(self, thresholds):
        return self.dice_at_counts(self.counts_above(thresholds))

    def thresholds_for_counts(self, counts):
        """DISTINCT scores only: an fp64 threshold with exactly c scores above it -- the midpoint of the neighbours, one beyond the ends."""
        c = np.asarray(counts, np.int64)
        assert ((c >= 0) & (c <= self.n)).all()
        hi = np.where(c > 0, self.ps[np.maximum(c, 1) - 1], self.ps[0] + 2.0)
        lo = np.where(c < self.n, self.ps[np.minimum(c, self.n - 1)], self.ps[-1] - 2.0)
        t = 0.5 * (hi + lo)
        assert ((lo < t) & (t < hi)).all(), 'a midpoint does not separate its neighbours in fp64'
        return t


def desc_key(p):
    """The sort key of csrc/uad_eval.hip restated: ascending unsigned order of the key = descending order of the fp32 score."""
    u = np.asarray(p, F32).view(np.uint32)
    asc = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))
    return ~asc


def partial_wave_has_digit0(p):
    """The first scatter pass reads the keys in input order.  True when the last tile ends inside a wave (so that wave holds invalid lanes,
    which carry digit 0) and a real key of that wave has a zero low byte too."""
    n = p.size
    if n % WAVE == 0:
        return False
    low = desc_key(p[n - n % WAVE:]) & np.uint32(255)
    return bool((low == 0).any())


def labels_for(p, rng):
    """Labels correlated with the score, so the prefix sums carry structure: 98 % positive below 0.6, 50 % above (the scheme of
    tests/test_gpu_lesionwise.py).  The precision falls from the prevalence at the lowest threshold to ~0.5 at the highest, so the levels of
    PRECISIONS are crossed mid-curve and threshold_at_precision has more than the trivial answer.  Both classes present from n = 2 on."""
    y = rng.random(p.size) < np.where(p < 0.6, 0.98, 0.5)
    if p.size >= 2:
        y[np.argmax(p)], y[np.argmin(p)] = True, False
    return y


def distinct_case(n, seed=None):
    """p = permutation(n) / n in fp32: n distinct scores in [0, 1).  Where one exists, a score whose key has a zero low byte is moved to
    the last input position (partial_wave_has_digit0)."""
    assert 0 < n < 2 ** 24
    rng = np.random.default_rng(n if seed is None else seed)
    p = (rng.permutation(n) / n).astype(F32)
    if n % WAVE:
        zero = np.nonzero(desc_key(p) & np.uint32(255) == 0)[0]
        if zero.size:
            j = zero[0]
            p[j], p[n - 1] = p[n - 1], p[j]
    s = np.sort(p)
    assert (np.diff(s) > 0).all(), 'scores are not distinct in fp32'
    y = labels_for(p, rng)
    return types.SimpleNamespace(p=p, y=y, model=SortedModel(p, y))


def big_counts(n=BIG_N):
    """The probe counts of the large distinct case: the first scan blocks, both sides of every carry boundary, the end, ~2000 seeded ones."""
    fixed = [1, SC_BLOCK - 1, SC_BLOCK, SC_BLOCK + 1, n - 2, n - 1, n] + [CARRY * j + d for j in (1, 2) for d in (-1, 0, 1)]
    rnd = np.random.default_rng(2000).integers(0, n + 1, 2000)
    return np.unique(np.r_[fixed, rnd]).astype(np.int64)


def _with_oracle(case):
    with np.errstate(divide='ignore', invalid='ignore'):
        case.auroc, case.auprc = osc.auroc(case.p, case.y), osc.average_precision(case.p, case.y)
    return case


@functools.lru_cache(maxsize=None)
def big_distinct():
    """n = 2 * 2048 * 1024 + 4097 distinct scores; the oracle's AUROC / AUPRC are computed once per process."""
    return _with_oracle(distinct_case(BIG_N))


@functools.lru_cache(maxsize=None)
def big_ties():
    """The same n with heavy ties: half the scores exactly 0, the rest on a 1/4096 grid over [-1, 1].  Sorted, ~4096 runs of ~256 equal
    scores come first, the 2.1 M zeros lie across the first carry boundary, and ~4096 more runs follow them across the second one: the flag
    scan carries a non-zero count into flags that are set irregularly."""
    rng = np.random.default_rng(4096)
    p = (np.round((2.0 * rng.random(BIG_N) - 1.0) * 4096) / 4096).astype(F32)
    p[rng.random(BIG_N) < 0.5] = 0.0
    y = labels_for(p, rng)
    case = types.SimpleNamespace(p=p, y=y, model=SortedModel(p, y))
    v = np.unique(case.model.ps)                                # ascending distinct values
    # thresholds at every value (count = the end of the next higher run) and between neighbours (the same count: both must agree)
    case.thresholds = np.r_[v, 0.5 * (v[1:] + v[:-1]), v[0] - 1.0, v[-1] + 1.0]
    return _with_oracle(case)


def values_case(n):
    """Scores drawn from VALUE_SET with many repeats.  The positive rate falls as the score rises, so the precision levels of PRECISIONS
    are crossed at different thresholds; +0.0 is mostly positive and -0.0 mostly negative, so the pair's merge into one threshold shows in
    AUPRC; the last input element is -inf (key low bytes 0, next to the invalid lanes of the last round)."""
    rng = np.random.default_rng(n)
    idx = rng.integers(0, VALUE_SET.size, n)
    p = VALUE_SET[idx]
    p[-1] = -np.inf
    y = rng.random(n) < 0.95 - 0.06 * idx
    pz, nz = (p == 0) & ~np.signbit(p), (p == 0) & np.signbit(p)
    y[pz] = rng.random(int(pz.sum())) < 0.9
    y[nz] = rng.random(int(nz.sum())) < 0.1
    assert all((p.view(np.uint32) == v.view(np.uint32)).sum() > n // 40 for v in VALUE_SET)       # bit patterns: -0.0 and +0.0 counted apart
    v = np.unique(p.astype(np.float64))
    finite = v[np.isfinite(v)]
    case = types.SimpleNamespace(p=p, y=y, model=SortedModel(p, y))
    case.thresholds = np.r_[v, 0.5 * finite[1:] + 0.5 * finite[:-1], -np.inf, np.inf, -0.0, 0.0]
    # the same scores with -0.0 moved to a value of its own between +0.0 and the next lower score: what a sort that split the pair would see
    case.p_split = np.where(nz, F32(-1e-43), p).astype(F32)
    return _with_oracle(case)


def single_class_cases():
    """(name, scores, labels): all-negative and all-positive labels at n = 10 and 4097, all scores equal with mixed labels."""
    out = []
    for n in (10, 4097):
        rng = np.random.default_rng(n)
        p = np.round(rng.random(n) * 64).astype(F32) / F32(64)                       # ties too
        out += [(f'neg{n}', p, np.zeros(n, bool)), (f'pos{n}', p, np.ones(n, bool)),
                (f'equal{n}', np.full(n, 0.25, F32), rng.random(n) < 0.3)]
    return out


def host_metrics(p, y):
    """(auroc, auprc) of the oracle and of trainers/Metrics.py, quietly (single-class labels divide 0 by 0; infinities subtract to nan)."""
    p64, y = np.asarray(p, np.float64), np.asarray(y).astype(bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (osc.auroc(p64, y), osc.average_precision(p64, y)), (Metrics.compute_roc(p64, y)[0], Metrics.compute_prc(p64, y)[0])


def healthy_patients(positive=False):
    """Two small patients for Evaluation._score_diffs whose labels hold one class only (a healthy-only test set; or every voxel a lesion)."""
    rng = np.random.default_rng(7)
    diffs, labels = [], []
    for k in range(2):
        d = (np.round(rng.random((24, 32, 32)) * 32) / 64 * (rng.random((24, 32, 32)) < 0.05)).astype(F32)
        d[5:9, 8:14, 8:14] += F32(0.125)                          # a false blob of more than 7 voxels; every score stays below 0.7
        diffs.append(d)
        labels.append(np.full(d.shape, int(positive), np.int64))
    return diffs, labels
