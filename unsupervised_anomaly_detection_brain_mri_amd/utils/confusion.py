"""The voxel-wise operating-point metrics of the evaluation as functions of four integers per patient.

utils/Evaluation.py:452-500 of the reference thresholds the filtered residual volume and hands the boolean prediction and label arrays to
trainers/Metrics.py: dice, precision and recall per patient and overall, confusion_matrix, tpr (twice, once as "FPR", sic) and vd.  Every one of
them is a function of TP, FP, FN, TN of `pred > thr` against `gt != 0`.  This module states both halves in numpy:

    confusion_counts(pred, gt, lengths, thr)   {TP, FP, FN, TN} per contiguous segment (patient) -- the statement csrc/uad_confusion.hip is held to,
                                               and the route of an engine without the device op
    metrics_from_counts(counts)                the reference's scalars from one row of counts (or from the column sums: the overall values)

metrics_from_counts is BIT-equal to trainers/Metrics.py on the boolean arrays: the same int64 operands in the same expressions, on numpy scalars
under np.errstate, so that 0 / 0 is nan exactly where the reference's division gives nan (a Python-int division would raise instead)."""
import numpy as np

TP, FP, FN, TN = 0, 1, 2, 3                        # the columns of a counts row


def segment_offsets(lengths, n=None):
    """int64 [P + 1] offsets of P contiguous segments of the given lengths, the first at 0.  lengths: a 1-D sequence of non-negative integers;
    with n, their sum must be n.  ValueError otherwise."""
    lens = np.asarray(lengths)
    if lens.ndim != 1 or (lens.size and not np.issubdtype(lens.dtype, np.integer)):
        raise ValueError(f'lengths must be a 1-D sequence of integers, got {lens.dtype} {lens.shape}')
    lens = lens.astype(np.int64)
    if (lens < 0).any():
        raise ValueError(f'segment {int(np.argmax(lens < 0))} has the negative length {int(lens[lens < 0][0])}')
    offsets = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    if n is not None and int(offsets[-1]) != int(n):
        raise ValueError(f'the segment lengths add up to {int(offsets[-1])}, the arrays hold {int(n)} voxels')
    return offsets


def confusion_counts(pred, gt, lengths, thr=0.0):
    """int64 [P, 4] = {TP, FP, FN, TN} per segment of `pred > float32(thr)` (an ordered comparison: a NaN is not a prediction) against
    `gt != 0`.  pred: any array of sum(lengths) values (taken flat, as float32); gt: as many labels of an integer or bool dtype."""
    p = np.asarray(pred, np.float32).reshape(-1)
    g = np.asarray(gt).reshape(-1)
    if g.size != p.size:
        raise ValueError(f'{g.size} labels for {p.size} values')
    offsets = segment_offsets(lengths, p.size)
    with np.errstate(invalid='ignore'):
        p = p > np.float32(thr)
    g = g != 0
    counts = np.zeros((offsets.size - 1, 4), np.int64)
    for s in range(offsets.size - 1):
        ps, gs = p[offsets[s]:offsets[s + 1]], g[offsets[s]:offsets[s + 1]]
        counts[s] = (np.count_nonzero(ps & gs), np.count_nonzero(ps & ~gs), np.count_nonzero(~ps & gs), np.count_nonzero(~ps & ~gs))
    return counts


def metrics_from_counts(counts):
    """One row {TP, FP, FN, TN} -> the scalars trainers/Metrics.py gives on the boolean arrays P, G the row was counted on, bit for bit:
    'dice' = Metrics.dice(P, G), 'precision', 'recall', 'tpr' (= recall), 'vd' (numpy float64, nan where the reference divides 0 by 0) and
    'confusion' = Metrics.confusion_matrix(P, G), numpy int64 in ITS order (TP, FP, TN, FN)."""
    c = np.asarray(counts)
    if c.shape != (4,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f'counts must be four integers {{TP, FP, FN, TN}}, got {c.dtype} {c.shape}')
    tp, fp, fn, tn = (np.int64(v) for v in c)
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'dice': (2 * tp) / ((tp + fp) + (tp + fn)),          # Metrics.dice: (2 * sum(P * G)) / (sum(P) + sum(G))
                'precision': tp / (tp + fp),
                'recall': tp / (tp + fn),
                'tpr': tp / (tp + fn),
                'vd': fn / (tp + fn),                                # Metrics.vd: sum(xor(P & G, G)) / sum(G)
                'confusion': (tp, fp, tn, fn)}
