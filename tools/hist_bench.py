"""Host numpy against the device per-class histograms (uad_select_quantiles_masked, uad_histogram_by_class through
engine.labelled_histogram) on the residual histograms of evaluate() (utils/Evaluation.py:399-402 -> utils/utils.py:44-71).

    python tools/hist_bench.py [--out profiles/r15_hist.json] [--host-reps 3] [--reps 20]

One 110 x 256 x 256 residual volume (7.2 M voxels): about half of it exact zeros (outside the eroded brain mask), the rest a skewed positive
residual, 2 % of the voxels labelled as lesion with larger residuals there; bins='auto' on the range 0.01 .. 0.075.
`host` = the host statement utils/histograms.labelled_histograms on this machine's CPU (host clock); `device` = engine.labelled_histogram on
a host array, the upload of values and class ids and the one small download included (host clock around a call that ends in a synchronising
download); `device_resident` = the same on a device-resident tensor (the class ids are still formed on the host and uploaded: the label maps
are host arrays in evaluate()).  Every timed shape is warmed up first; median / min / max over the repetitions.  The device result is also
compared with the statement's (`equal`: counts and edges exactly; `moments_rel`: the largest relative difference of a mean or variance).
The bound reported is the HBM read traffic of the launches: the masked select reads 4 x (4 + 1) B per voxel, each of the two histogram
launches 4 + 1 B per voxel per chunk of 1024 bins.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.select_bench import timed  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd import _lib  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils import histograms  # noqa: E402

S, NH, NW = 110, 256, 256
RANGE = (0.01, 0.075)


def volume(seed=0):
    rng = np.random.default_rng(seed)
    n = S * NH * NW
    lab = (rng.random(n) < 0.02).astype(np.int64)
    v = (rng.random(n, dtype=np.float32) ** 3 * np.float32(0.12)).astype(np.float32)
    v[lab == 1] += np.float32(0.03)
    v[rng.random(n) < 0.5] = 0.0
    return v, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    eng = DeviceOps()
    sync = lambda: torch.cuda.synchronize(eng.device)
    v, lab = volume()
    vd = eng._dev(v)
    want = histograms.labelled_histograms(v, lab, 'auto', RANGE)
    got = eng.labelled_histogram(vd, lab, 'auto', RANGE)
    bins = int(want[0]['n'].size)
    chunks = -(-bins // _lib.HISTOGRAM_MAX_BINS)
    rel = max(abs(g[k] - w[k]) / abs(w[k]) for g, w in zip(got, want) for k in ('mean', 'var'))
    res = {'device': torch.cuda.get_device_name(eng.device), 'numpy': np.__version__, 'voxels': int(v.size), 'classes': len(want), 'bins': bins,
           'equal': bool(all(np.array_equal(g['n'], w['n']) and np.array_equal(g['bins'], w['bins']) for g, w in zip(got, want))),
           'moments_rel': float(rel),
           'host': timed(lambda: histograms.labelled_histograms(v, lab, 'auto', RANGE), a.host_reps, 1),
           'device': timed(lambda: eng.labelled_histogram(v, lab, 'auto', RANGE), a.reps, 2, sync),
           'device_resident': timed(lambda: eng.labelled_histogram(vd, lab, 'auto', RANGE), a.reps, 2, sync),
           'read_bound_bytes': int(v.size) * 5 * (4 + 1 + chunks)}
    eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
