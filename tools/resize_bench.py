"""The host resize statement (utils/resize.py) against the device resize op (uad_resize2d) on the resize step of the BrainWeb slice ingestion.

    python tools/resize_bench.py [--out profiles/r12_resize.json] [--host-reps 3] [--reps 20]

Workload: one 181 x 217 x 181 volume (BrainWeb's grid), 120 axial slices of 217 x 181 -> 128 x 128 (dataloaders/BRAINWEB.py:140-142) -- the
image (bilinear) and the lesion map (nearest), gathered out of the slice-major volume by a kept-slice list.
  host             utils/resize.py on the kept slices of the host volume (vectorised numpy, one call per map); host clock.
  device           engine.resize(index=kept) on the host volumes, results downloaded to host arrays: H2D of both volumes + two launches + D2H;
                   host clock around calls that end in the download (which synchronises).
  device_resident  the same two calls on the device-resident volumes (what nifti.volume_to_slices(loader='brainweb') does after the
                   normalisation), ending in one download of the resized images and labels; host clock.
The method is tools/rotate_bench.py's: every timed variant is warmed up first; median / min / max over the repetitions are reported.  No
threshold is set here.  Needs the GPU: there is no fallback (--host-only times the host statement alone and says so in the result)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unsupervised_anomaly_detection_brain_mri_amd.utils.resize import resize_linear, resize_nearest  # noqa: E402

NZ, NY, NX = 181, 217, 181
KEPT = list(range(30, 150))
R = 128


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def host_resize(vol, lab):
    return resize_linear(vol[KEPT], (R, R)), resize_nearest(lab[KEPT], (R, R))


def device_resize(eng, vol, lab):
    import torch
    return torch.stack([eng.resize(vol, (R, R), mode='linear', index=KEPT), eng.resize(lab, (R, R), mode='nearest', index=KEPT)]).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r12_resize.json'))
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-only', action='store_true', help='time the host statement alone (no GPU needed); the result records that nothing ran on a device')
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    vol = rng.random((NZ, NY, NX), dtype=np.float32)
    lab = (rng.random((NZ, NY, NX), dtype=np.float32) > 0.97).astype(np.float32)
    res = {'workload': f'{NZ}x{NY}x{NX} volume, {len(KEPT)} axial slices of {NY}x{NX} -> {R}x{R}: image (linear) + label map (nearest), gathered by index',
           'numpy': np.__version__}
    res['host'] = stats(timed(lambda: host_resize(vol, lab), a.host_reps, 1))
    # bytes one image + label call pair must move at least: the kept input slices read once, the output written once (fp32 both)
    res['bytes_model'] = {'read': 2 * len(KEPT) * NY * NX * 4, 'write': 2 * len(KEPT) * R * R * 4}
    if a.host_only:
        res['device'] = None
        res['note'] = 'host statement only: not measured on the GPU'
    else:
        import torch
        from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
        assert torch.cuda.is_available(), 'resize_bench needs the GPU (or --host-only)'
        eng = DeviceOps()
        res['device'] = torch.cuda.get_device_name(0)
        res['device_with_upload'] = stats(timed(lambda: device_resize(eng, vol, lab), a.reps, 3))
        vd, ld = torch.from_numpy(vol).to(eng.device), torch.from_numpy(lab).to(eng.device)
        res['device_resident'] = stats(timed(lambda: device_resize(eng, vd, ld), a.reps, 3))
        # agreement at the timed size (the GPU tests hold the bar, bit equality; this is the record beside the timing)
        got, want = device_resize(eng, vd, ld), host_resize(vol, lab)
        res['agreement'] = {'image_bits_differ': int(np.count_nonzero(got[0].view(np.uint32) != want[0].view(np.uint32))),
                            'label_bits_differ': int(np.count_nonzero(got[1].view(np.uint32) != want[1].view(np.uint32)))}
        res['speedup_with_upload'] = res['host']['median_ms'] / res['device_with_upload']['median_ms']
        res['speedup_resident'] = res['host']['median_ms'] / res['device_resident']['median_ms']
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
