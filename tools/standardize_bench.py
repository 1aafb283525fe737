"""Host statement against the device route of NII.normalize(method='standardization') (utils/standardize.py; uad_select_quantiles,
uad_shifted_sums, uad_clamp_standardize) on one 110 x 217 x 181 skull-stripped volume, in the shape of tools/select_bench.py.

    python tools/standardize_bench.py [--out profiles/r21_standardize.json] [--host-reps 3] [--reps 20]

`host` = nifti.normalize_standardization without an engine (numpy on this machine's CPU, host clock); `numpy_float32` = the reference's own
expression (np.percentile clamps, v - v.mean(), c / c.std()) for comparison; `device` = the engine route on a host array, upload and download
of the volume included; `device_resident` = the same on a device-resident tensor, the result left there (one select call with its small
download, three ordered-sum launches with a 16-byte download each, one map pass); `shifted_sums_resident` = ONE shifted_sums call alone, against
its 4 B x n of reads.  Host clock around calls that end in a synchronising download; every timed shape is warmed up first; median / min / max
over the repetitions.  The device result is compared with the host statement's (`equal`: same bytes).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.select_bench import timed, volume  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti  # noqa: E402


def numpy_float32(v):
    v = v.astype(np.float32)
    q = np.percentile(v, 0); v[v < q] = q
    q = np.percentile(v, 99.8); v[v > q] = q
    c = v - np.mean(v)
    return c / np.std(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    eng = DeviceOps()
    sync = lambda: torch.cuda.synchronize(eng.device)
    v = volume()
    vd = eng._dev(v)
    n = v.size
    host = nifti.normalize_standardization(v)
    dev = nifti._normalize_standardization_on(eng, vd, 0, 99.8)
    mean32, std32 = eng.last_moments                              # (of the call above)
    sums = timed(lambda: eng.shifted_sums(vd, None, None, mean32, 0.0), a.reps, 2, sync)
    res = {'gpu': torch.cuda.get_device_name(eng.device), 'numpy': np.__version__, 'voxels': n,
           'equal': bool(dev.cpu().numpy().tobytes() == host.tobytes()),
           'max_abs_diff_to_numpy_float32': float(np.max(np.abs(host - numpy_float32(v)))),
           'mean32': float(mean32), 'std32': float(std32),
           'host': timed(lambda: nifti.normalize_standardization(v), a.host_reps, 1),
           'numpy_float32': timed(lambda: numpy_float32(v), a.host_reps, 1),
           'device': timed(lambda: nifti.normalize_standardization(v, engine=eng), a.reps, 2, sync),
           'device_resident': timed(lambda: nifti._normalize_standardization_on(eng, vd, 0, 99.8), a.reps, 2, sync),
           'select_only_resident': timed(lambda: eng.select_quantiles(vd, [0.0, 0.998, 1.0], [True, True, False]), a.reps, 2, sync),
           'shifted_sums_resident': sums,
           'shifted_sums_read_bytes': 4 * n,
           'shifted_sums_gb_per_s_at_median': 4 * n / (sums['median_ms'] * 1e-3) / 1e9,
           'bytes_per_voxel': {'select': 16, 'sums': 12, 'map': 8}}
    eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
