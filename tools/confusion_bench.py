"""Host numpy against the device per-patient confusion counts (uad_confusion_by_segment through engine.confusion_counts) on the voxel-wise tail of
Evaluation._score_diffs / _lesionwise_keys (utils/Evaluation.py:452-500).

    python tools/confusion_bench.py [--out profiles/r22_confusion.json] [--host-reps 3] [--reps 20]

One stacked, filtered prediction of five 110 x 256 x 256 patients (36 M voxels, fp32 0 / 1 on the device, as uad_cc_filter leaves it) with 2 % of
the voxels foreground, and the patients' label maps (bool, host) with 2 % lesion, overlapping the prediction in part.
`host` = the route of an engine without the op: the download of the prediction, `> 0`, and the trainers/Metrics.py calls of _score_diffs and
_lesionwise_keys on the boolean arrays (dice overall, dice / precision / recall per patient, confusion_matrix, tpr twice, vd), host clock;
`device` = engine.confusion_counts on the resident prediction with the patients' bool label maps stacked on the host, viewed as bytes and uploaded
(what _score_diffs does), the one small download and
utils.confusion.metrics_from_counts for the same scalars included (host clock around a call that ends in a synchronising download);
`device_resident` = the same with the labels already resident as uint8.  Every timed shape is warmed up first; median / min / max over the
repetitions.  `equal`: the counts equal the host statement's and every scalar equals Metrics' bit for bit.  The bound reported is the HBM read
traffic of the launch, 4 + 1 B per voxel.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.select_bench import timed  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.trainers import Metrics  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils import confusion  # noqa: E402

PATIENTS, S, NH, NW = 5, 110, 256, 256


def volumes(seed=0):
    rng = np.random.default_rng(seed)
    shape = (PATIENTS * S, NH, NW)
    gt = rng.random(shape, dtype=np.float32) < 0.02
    pred = (rng.random(shape, dtype=np.float32) < 0.01) | (gt & (rng.random(shape, dtype=np.float32) < 0.5))     # 2 % foreground, half of it on lesions
    return pred.astype(np.float32), gt


def host_route(pred_dev, gts):
    """the statements of _score_diffs / _lesionwise_keys behind the download"""
    pred = pred_dev.cpu().numpy() > 0
    gt_all = np.concatenate(gts, axis=0)
    out = [Metrics.dice(pred, gt_all)]
    with np.errstate(divide='ignore', invalid='ignore'):
        for k, g in enumerate(gts):
            sub = pred[k * S:(k + 1) * S]
            out += [Metrics.dice(sub, g), Metrics.precision(sub, g), Metrics.recall(sub, g)]
        out += [*Metrics.confusion_matrix(pred, gt_all), Metrics.tpr(pred, gt_all), Metrics.tpr(pred, gt_all), Metrics.vd(pred, gt_all)]
    return out


def device_route(eng, pred_dev, labels, lengths):
    counts = eng.confusion_counts(pred_dev, labels, lengths, 0.0)
    overall = confusion.metrics_from_counts(counts.sum(axis=0))
    out = [overall['dice']]
    for row in counts:
        m = confusion.metrics_from_counts(row)
        out += [m['dice'], m['precision'], m['recall']]
    return out + [*overall['confusion'], overall['tpr'], overall['tpr'], overall['vd']], counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    eng = DeviceOps()
    sync = lambda: torch.cuda.synchronize(eng.device)
    pred, gt = volumes()
    gts = [gt[k * S:(k + 1) * S] for k in range(PATIENTS)]
    lengths = [S * NH * NW] * PATIENTS
    pred_dev = eng._dev(pred)
    gt_flat = gt.reshape(-1)
    gt_dev = torch.from_numpy(gt_flat.view(np.uint8)).to(eng.device)
    want = host_route(pred_dev, gts)
    stacked = lambda: np.concatenate([g.reshape(-1) for g in gts]).view(np.uint8)
    got, counts = device_route(eng, pred_dev, stacked(), lengths)
    got_resident, counts_resident = device_route(eng, pred_dev, gt_dev, lengths)
    statement = confusion.confusion_counts(pred, gt_flat, lengths, 0.0)
    same = lambda x, y: len(x) == len(y) and all(type(g) is type(w) and np.array_equal(g, w, equal_nan=True) for g, w in zip(x, y))
    res = {'gpu': torch.cuda.get_device_name(eng.device), 'numpy': np.__version__, 'voxels': int(pred.size), 'patients': PATIENTS,
           'counts': counts.tolist(),
           'equal': bool(np.array_equal(counts, statement) and np.array_equal(counts_resident, statement) and same(got, want) and same(got_resident, want)),
           'host': timed(lambda: host_route(pred_dev, gts), a.host_reps, 1),
           'device': timed(lambda: device_route(eng, pred_dev, stacked(), lengths), a.reps, 2, sync),
           'device_resident': timed(lambda: device_route(eng, pred_dev, gt_dev, lengths), a.reps, 2, sync),
           'read_bound_bytes': int(pred.size) * 5}
    eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
