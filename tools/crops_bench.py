"""The host statement of the lesion-centred crops (utils/crops.py) against the device ops (uad_cc_label + uad_cc_props + uad_crop2d) on the crop
step of the slice ingestion.

    python tools/crops_bench.py [--out profiles/r13_crops.json] [--host-reps 3] [--reps 20]

Workload: one 110 x 128 x 128 label batch at about 2 % foreground (smooth random blobs) and its image batch; cropType 'lesions' with 64 x 64
windows (dataloaders/MSLUB.py:200-222): per-slice components of the label batch, one window per component, cut out of the image batch and
the label batch.
  host             component_props(slab=1), lesion_crop_origins and two crop_windows calls on the host batches; host clock.
  device           engine.region_props(slab=1) and two engine.crop calls on the HOST batches, crops downloaded: H2D of both batches + the
                   labelling + the measurements + two gathers + D2H; host clock around calls that end in the download (which synchronises).
  device_resident  the same calls on the device-resident batches (what nifti.volume_to_slices(crops=('lesions', ...)) does after the
                   resampling), ending in one download of the image and label crops; host clock.
The method is tools/resize_bench.py's: every timed variant is warmed up first; median / min / max over the repetitions are reported.  No
threshold is set here.  Needs the GPU: there is no fallback (--host-only times the host statement alone and says so in the result)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unsupervised_anomaly_detection_brain_mri_amd.utils.crops import component_props, crop_windows, lesion_crop_origins  # noqa: E402

D, H, W = 110, 128, 128
CROP = 64
FILL = 0.02


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


def host_crops(img, lab):
    origins = lesion_crop_origins(component_props(lab, slab=1), H, W, CROP, CROP)
    return crop_windows(img, origins, CROP, CROP), crop_windows(lab, origins, CROP, CROP)


def device_crops(eng, img, lab):
    import torch
    origins = lesion_crop_origins(eng.region_props(lab, slab=1), H, W, CROP, CROP)
    return torch.stack([eng.crop(img, origins, (CROP, CROP)), eng.crop(lab, origins, (CROP, CROP))]).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r13_crops.json'))
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-only', action='store_true', help='time the host statement alone (no GPU needed); the result records that nothing ran on a device')
    a = ap.parse_args()
    from scipy.ndimage import uniform_filter
    rng = np.random.default_rng(13)
    f = uniform_filter(rng.random((D, H, W)).astype(np.float32), 3, mode='constant')
    lab = (f > np.quantile(f, 1.0 - FILL)).astype(np.float32)
    img = rng.random((D, H, W), dtype=np.float32)
    want = host_crops(img, lab)
    k = int(want[0].shape[0])
    res = {'workload': f'{D}x{H}x{W} label batch at {100 * float(lab.mean()):.2f} % foreground, cropType lesions {CROP}x{CROP}: {k} components = crops, image + label',
           'numpy': np.__version__, 'components': k}
    res['host'] = stats(timed(lambda: host_crops(img, lab), a.host_reps, 1))
    # bytes the device path must move at least: the labelling reads the mask and writes and re-reads the labels, the
    # measurements read the labels three times and write one rank word per root; the gather reads and writes every window word once, twice over
    res['bytes_model'] = {'cc_label_min': D * H * W * (4 + 4 + 4 + 4), 'cc_props_min': D * H * W * 3 * 4, 'crop2d': 2 * 2 * k * CROP * CROP * 4}
    if a.host_only:
        res['device'] = None
        res['note'] = 'host statement only: not measured on the GPU'
    else:
        import torch
        from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
        assert torch.cuda.is_available(), 'crops_bench needs the GPU (or --host-only)'
        eng = DeviceOps()
        res['device'] = torch.cuda.get_device_name(0)
        res['device_with_upload'] = stats(timed(lambda: device_crops(eng, img, lab), a.reps, 3))
        imd, lbd = torch.from_numpy(img).to(eng.device), torch.from_numpy(lab).to(eng.device)
        res['device_resident'] = stats(timed(lambda: device_crops(eng, imd, lbd), a.reps, 3))
        # the steps of the resident path one by one, each ending in a synchronisation
        sync = lambda: torch.cuda.synchronize(eng.device)
        origins = lesion_crop_origins(eng.region_props(lbd, slab=1), H, W, CROP, CROP)
        res['steps_resident'] = {'region_props': stats(timed(lambda: eng.region_props(lbd, slab=1), a.reps, 3)),
                                 'crop_one_batch': stats(timed(lambda: (eng.crop(imd, origins, (CROP, CROP)), sync()), a.reps, 3)),
                                 'download_both': stats(timed(lambda: torch.empty((2, k, CROP, CROP), device=eng.device).cpu(), a.reps, 3))}
        # agreement at the timed size (the GPU tests hold the bar, equality; this is the record beside the timing)
        got = device_crops(eng, imd, lbd)
        res['agreement'] = {'props_equal': bool(np.array_equal(eng.region_props(lbd, slab=1), component_props(lab, slab=1))),
                            'image_bits_differ': int(np.count_nonzero(got[0].view(np.uint32) != want[0].view(np.uint32))) if got[0].shape == want[0].shape else -1,
                            'label_bits_differ': int(np.count_nonzero(got[1].view(np.uint32) != want[1].view(np.uint32))) if got[1].shape == want[1].shape else -1}
        res['speedup_with_upload'] = res['host']['median_ms'] / res['device_with_upload']['median_ms']
        res['speedup_resident'] = res['host']['median_ms'] / res['device_resident']['median_ms']
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
