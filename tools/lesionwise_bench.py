"""Times the lesion-wise evaluation ops on one seeded [110,256,256] prediction / ground-truth pair at about 2 % foreground: the device
labelling (DeviceOps.cc_label) and DeviceOps.detection_rate with HIP events after a warm-up, and the host path they replace
(Evaluation.compute_detection_rate on the downloaded volumes: three scipy labellings per 20-slice chunk), download included.
For cc_label the algorithmic minimum traffic (one read of the volume, one write of the labels: 8 bytes per voxel) over its time is
reported as a fraction of what a plain device copy of the same 8 bytes per voxel reaches in the same run.

    python tools/lesionwise_bench.py [--out profiles/r07_lesionwise.json] [--reps 20]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import scipy.ndimage
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps               # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation                   # noqa: E402

SHAPE = (110, 256, 256)


def blobs(rng, shape, fill):
    f = scipy.ndimage.uniform_filter(rng.random(shape).astype(np.float32), 3, mode='constant')
    return f > np.quantile(f, 1.0 - fill)


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r07_lesionwise.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lesionwise_bench needs a GPU: nothing is measured without one')
    eng = DeviceOps()
    rng = np.random.default_rng(7)
    gt = blobs(rng, SHAPE, 0.02)
    lab, n = scipy.ndimage.label(gt, structure=np.ones((3, 3, 3), bool))
    keep = np.zeros(n + 1, bool)
    keep[1:] = rng.random(n) < 0.5
    pred = np.roll(keep[lab], (1, 2, -1), axis=(0, 1, 2)) | blobs(rng, SHAPE, 0.01) | (rng.random(SHAPE) < 2e-4)
    dp = torch.from_numpy(pred.astype(np.float32)).to(eng.device)
    dg = torch.from_numpy(gt.astype(np.float32)).to(eng.device)
    voxels = int(np.prod(SHAPE))

    res = {'shape': list(SHAPE), 'foreground_pred': float(pred.mean()), 'foreground_gt': float(gt.mean()), 'reps': args.reps}
    res['cc_label_ms'], res['cc_label_ms_min'], res['cc_label_ms_max'] = event_ms(lambda: eng.cc_label(dp), args.reps)
    res['detection_rate_ms'], res['detection_rate_ms_min'], res['detection_rate_ms_max'] = event_ms(lambda: eng.detection_rate(dp, dg), args.reps)
    res['device_counts'] = list(eng.detection_rate(dp, dg))
    # a plain copy that moves the same 8 bytes per voxel (4 read + 4 written)
    src, dst = torch.empty(voxels, device=eng.device, dtype=torch.int32), torch.empty(voxels, device=eng.device, dtype=torch.int32)
    res['copy_ms'] = event_ms(lambda: dst.copy_(src), args.reps)[0]
    res['cc_label_GBps_algorithmic'] = 8.0 * voxels / (res['cc_label_ms'] * 1e-3) / 1e9
    res['copy_GBps'] = 8.0 * voxels / (res['copy_ms'] * 1e-3) / 1e9
    res['cc_label_fraction_of_copy'] = res['cc_label_GBps_algorithmic'] / res['copy_GBps']

    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hp, hg = dp.cpu().numpy(), dg.cpu().numpy()            # the download the host path needs
        counts = Evaluation.compute_detection_rate(hp, hg)
        host.append((time.perf_counter() - t0) * 1e3)
    res['host_detection_rate_ms'] = float(np.median(host))
    res['host_counts'] = [int(c) for c in counts]
    res['counts_equal'] = res['host_counts'] == res['device_counts']
    res['host_over_device'] = res['host_detection_rate_ms'] / res['detection_rate_ms']
    res['box'] = {'host': socket.gethostname(), 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hip': torch.version.hip}
    try:
        res['commit'] = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res['commit'] = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == '__main__':
    main()
