"""The evaluation histograms of the reference (utils/Evaluation.py:399-411 -> utils/utils.py:44-71, plot_histogram_with_labels): the
histogram of the residual volume -- with Monte-Carlo sampling also of the epistemic variances -- split by ground-truth class, and each
class's mean and variance.

`labelled_histograms` is the host statement in plain numpy: the path of an engine without the device ops and the reference of their tests.
  * classes = np.unique(labels); more than four raise (the reference indexes its four COLORS);
  * class i is counted by np.histogram(data[labels == classes[i]], bins, range) -- what pyplot.hist does for one data set, with the counts cast
    to float64 -- and `bins` is REASSIGNED by the loop: class 0 fixes the edge array (from 'auto' or an integer), every later class is counted
    on it and its own `range` is ignored;
  * mean / var are over all values of the class, not only those in range.  Stated deviation: they are float64 here (np.mean / np.var with
    dtype=float64; the device sums are fp64), the reference's are numpy's in the data's dtype.
`write_labelled_histograms` writes `<stem>.{i}.npy` (a pickle, utils.py:52-53) and `<stem>.pdf.{i}.csv` (csv.DictWriter, utils.py:55-60) per
class.  Stated deviations: no PDF is written (matplotlib is not a dependency), and the .npy name is always formed inside eval_dir (the
reference splits the whole path at its first dot).

The host half of bins='auto' restates numpy.lib._histograms_impl (_get_bin_edges, _hist_bin_auto, _hist_bin_fd, _hist_bin_sturges of numpy
2.2) over FIVE numbers of the values in range -- m, min, max and the brackets of the 25 % and 75 % order statistics, which is what one masked
device select returns (include/uad_hip.h: uad_select_quantiles_masked with q = {0, 0.25, 0.75, 1})."""
import csv
import os
import pickle

import numpy as np

from .order_stats import finish_linear, percentile_fractions

MAX_CLASSES = 4            # utils/utils.py:13 COLORS; include/uad_hip.h: UAD_HISTOGRAM_MAX_CLASSES
AUTO_Q = (0.0, 0.25, 0.75, 1.0)
MAX_DEVICE_BINS = 65536    # longer tables are left to the host statement (64 chunks of UAD_HISTOGRAM_MAX_BINS: 64 passes over the data)


class TooManyBins(ValueError):
    """engine.labelled_histogram: the edge table is longer than MAX_DEVICE_BINS; the caller takes labelled_histograms."""


def labelled_histograms(data, labels, bins, range):
    """[{'class', 'n' (float64 [bins]), 'bins' (edges), 'mean', 'var'}] per class of np.unique(labels), as plot_histogram_with_labels
    computes them.  data, labels: arrays of one shape; bins: 'auto', an integer or an edge array; range: (first, last)."""
    data, labels = np.asarray(data), np.asarray(labels)
    if data.shape != labels.shape:
        raise ValueError(f'data {data.shape} and labels {labels.shape} must have one shape')
    classes = np.unique(labels)
    if classes.size > MAX_CLASSES:
        raise ValueError(f'at most {MAX_CLASSES} classes, got {classes.size}')
    out = []
    for c in classes:
        d = data[labels == c]
        n, bins = np.histogram(d.flatten(), bins=bins, range=range)
        out.append({'class': c, 'n': n.astype(np.float64), 'bins': bins, 'mean': np.mean(d, dtype=np.float64), 'var': np.var(d, dtype=np.float64)})
    return out


def outer_edges(range):
    """numpy's _get_outer_edges for a given range."""
    first, last = range
    if first > last:
        raise ValueError('max must be larger than min in range parameter.')
    if not (np.isfinite(first) and np.isfinite(last)):
        raise ValueError(f'supplied range of [{first}, {last}] is not finite')
    if first == last:
        first, last = first - 0.5, last + 0.5
    return first, last


def range_to_float32(first, last, dtype):
    """(lo32, hi32): float32 bounds with lo32 <= v <= hi32 exactly where numpy's `(a >= first) & (a <= last)` holds for a float32-representable
    value v of an array of `dtype`.  numpy compares in result_type(bound, a): in float32 the bound itself is rounded to float32; in float64 the
    lower bound becomes the smallest float32 at or above it and the upper the largest at or below (order_stats.edges_to_float32's rule)."""
    def one(b, up):
        if np.result_type(b, np.empty(0, dtype)) == np.float32:
            return np.float32(b)
        b = np.float64(b)
        f = np.float32(b)
        if up and np.float64(f) < b:
            f = np.nextafter(f, np.float32(np.inf))
        if not up and np.float64(f) > b:
            f = np.nextafter(f, np.float32(-np.inf))
        return f
    return one(first, True), one(last, False)


def auto_bin_count(m, vmin, vmax, q25, q75, range, dtype):
    """The number of equal bins np.histogram_bin_edges(x, 'auto', range) takes for the m values x (of `dtype`) that lie in the range, from
    their extremes vmin / vmax and the brackets q25 = (lo, hi), q75 = (lo, hi) of the order statistics around the virtual indices (m - 1) *
    0.25 and (m - 1) * 0.75 (float64 indices: np.percentile(x, [75, 25]) takes an array q)."""
    dtype = np.dtype(dtype)
    first, last = outer_edges(range)
    m = int(m)
    if m == 0:
        return 1
    q = percentile_fractions([75, 25], dtype)
    p75 = finish_linear([m], [q75[0]], [q75[1]], q[0], dtype)[0]
    p25 = finish_linear([m], [q25[0]], [q25[1]], q[1], dtype)[0]
    iqr = np.subtract(p75, p25)
    fd_bw = 2.0 * iqr * m ** (-1.0 / 3.0)
    sturges_bw = np.subtract(dtype.type(vmax), dtype.type(vmin), dtype=dtype) / (np.log2(m) + 1.0)
    width = min(fd_bw, sturges_bw) if fd_bw else sturges_bw
    if not width:
        return 1
    return int(np.ceil(np.subtract(last, first, dtype=np.result_type(last, first)) / width))


def equal_bin_edges(n_bins, range, dtype):
    """np.histogram_bin_edges(x, n_bins, range) for any x of `dtype` (the data enter through their dtype only)."""
    return np.histogram_bin_edges(np.empty(0, np.dtype(dtype)), int(n_bins), range)


def auto_bin_edges(m, vmin, vmax, q25, q75, range, dtype):
    """np.histogram_bin_edges(x, 'auto', range) from the five numbers (see auto_bin_count)."""
    return equal_bin_edges(auto_bin_count(m, vmin, vmax, q25, q75, range, dtype), range, dtype)


def auto_numbers(x, range):
    """(m, min, max, (p25 lo, p25 hi), (p75 lo, p75 hi)) of the values of x inside the range, by a sort: the host model of the masked
    device select, for cross-checks against numpy."""
    x = np.asarray(x).reshape(-1)
    first, last = outer_edges(range)
    s = np.sort(x[(x >= first) & (x <= last)])
    m = s.size
    if m == 0:
        nan = np.float32(np.nan)
        return 0, nan, nan, (nan, nan), (nan, nan)

    def bracket(q):
        v = (m - 1) * q
        lo = int(np.floor(v)) if v < m - 1 else m - 1
        return s[lo], s[min(lo + 1, m - 1)]
    return m, s[0], s[-1], bracket(0.25), bracket(0.75)


def class_ids(labels):
    """(classes, ids): np.unique(labels) and the uint8 index of every label in it; ValueError above MAX_CLASSES classes.  Integer and
    boolean label maps are not sorted for this (np.unique's sort of a 21.6 M-voxel label map would cost more than the device histogram):
    the classes are found by repeated minima above the last one, at most MAX_CLASSES + 1 passes, and the index is the number of classes
    at or below the label."""
    lab = np.asarray(labels).reshape(-1)
    if lab.dtype.kind not in 'iub' or lab.size == 0:
        classes, ids = np.unique(lab, return_inverse=True)
        if classes.size > MAX_CLASSES:
            raise ValueError(f'at most {MAX_CLASSES} classes, got {classes.size}')
        return classes, np.ascontiguousarray(ids.reshape(-1), dtype=np.uint8)
    c, hi = lab.min(), lab.max()
    classes = [c]
    while c < hi:
        c = np.min(lab, where=lab > c, initial=hi)
        classes.append(c)
        if len(classes) > MAX_CLASSES:
            raise ValueError(f'at most {MAX_CLASSES} classes, got more')
    classes = np.array(classes, dtype=lab.dtype)
    ids = np.zeros(lab.size, np.uint8)
    for c in classes[1:]:
        np.add(ids, lab >= c, out=ids, casting='unsafe')
    return classes, ids


def write_labelled_histograms(result, eval_dir, stem):
    """<eval_dir>/<stem>.{i}.npy (pickle.dump of n / bins / mean / var) and <eval_dir>/<stem>.pdf.{i}.csv (csv.DictWriter on a text file
    opened with mode="w", header Bin,Count, one row of the left edge and the count per bin) for every class i of `result`
    (labelled_histograms' list).  Returns the files written."""
    files = []
    for i, r in enumerate(result):
        files.append(os.path.join(eval_dir, f'{stem}.{i}.npy'))
        with open(files[-1], 'wb') as file:
            pickle.dump({'n': r['n'], 'bins': r['bins'], 'mean': r['mean'], 'var': r['var']}, file)
        files.append(os.path.join(eval_dir, f'{stem}.pdf.{i}.csv'))
        with open(files[-1], mode="w") as csv_file:
            writer = csv.DictWriter(csv_file, fieldnames=["Bin", "Count"])
            writer.writeheader()
            for k in range(len(r['n'])):
                writer.writerow({"Bin": r['bins'][k], "Count": r['n'][k]})
    return files
