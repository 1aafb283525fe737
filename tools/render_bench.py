"""The host statement of the sample-image renderings (utils/render.py) against the device ops (uad_render_minmax_u8 / uad_render_heatmap /
uad_render_overlay) on one patient's images of evaluate()'s options['exportSamples'].

    python tools/render_bench.py [--out profiles/r14_render.json] [--host-reps 3] [--reps 20]

Workload: 110 slices of 128 x 128 and all six image kinds of a slice -- four grey images from fp32 stacks (input, reconstruction, residual
before and after the median), the label image, the heat map (RGBA) and the TP / FP / FN overlay (RGB): 110 x 128 x 128 x 12 bytes of images.
  host             utils/render.py on host arrays; host clock.
  device           the engine's render ops on HOST arrays, ending in the download of the uint8 images: H2D of the fp32 stacks + seven
                   launches + D2H; host clock around calls that end in the download (which synchronises).
  device_resident  the same calls on device-resident stacks (what _evaluate holds when evaluate_volume returns), ending in the same download.
  png              utils/png.py's write_png of all 110 x 7 images into a scratch directory, timed apart: deflate is the host work left.
The method is tools/resize_bench.py's: every timed variant is warmed up first; median / min / max over the repetitions are reported.  No
threshold is set here.  Needs the GPU: there is no fallback (--host-only times the host statement and the PNG encoding alone and says so)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unsupervised_anomaly_detection_brain_mri_amd.utils import png, render  # noqa: E402

S, R = 110, 128
GREY = ('x', 'rec', 'diff', 'diff_filtered')


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


def workload():
    rng = np.random.default_rng(14)
    w = {'x': rng.random((S, R, R), dtype=np.float32)}
    w['rec'] = np.clip(w['x'] + rng.normal(0, 0.05, (S, R, R)).astype(np.float32), 0, 1)
    lesion = rng.random((S, R, R)) < 0.02
    w['diff'] = np.where(lesion, rng.random((S, R, R), dtype=np.float32) * np.float32(0.05), np.float32(0)).astype(np.float32)
    w['diff_filtered'] = np.where(rng.random((S, R, R)) < 0.5, w['diff'], np.float32(0)).astype(np.float32)
    w['gt'] = lesion.astype(np.float32)
    w['pred'] = (w['diff_filtered'] > 0.02).astype(np.float32)
    return w


def host_render(w):
    grey = np.concatenate([render.minmax_u8(w[k]) for k in GREY] + [render.label_u8(w['gt'])])
    return grey, render.heatmap_rgba(w['diff_filtered']), render.overlay_rgb(w['x'], w['pred'], w['gt'])


def device_render(eng, w):
    import torch
    grey = torch.cat([eng.render_gray(w[k]) for k in GREY] + [eng.render_gray(w['gt'])]).cpu().numpy()
    return grey, eng.render_heatmap(w['diff_filtered']).cpu().numpy(), eng.render_overlay(w['x'], w['pred'], w['gt']).cpu().numpy()


def write_all(images, directory):
    grey, heat, vis = images
    for k in range(S):
        for j in range(5):
            png.write_png(os.path.join(directory, f'0_{k}_{j}.png'), grey[j * S + k])
        png.write_png(os.path.join(directory, f'0_{k}_heatmap.png'), heat[k])
        png.write_png(os.path.join(directory, f'0_{k}_vis.png'), vis[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r14_render.json'))
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-only', action='store_true', help='time the host statement and the PNG encoding alone (no GPU needed); the result records that nothing ran on a device')
    a = ap.parse_args()
    w = workload()
    res = {'workload': f'{S} slices of {R}x{R}: 4 grey images + label image (1 B/pixel each), heat map (4 B/pixel), overlay (3 B/pixel)', 'numpy': np.__version__}
    res['host'] = stats(timed(lambda: host_render(w), a.host_reps, 1))
    want = host_render(w)
    with tempfile.TemporaryDirectory() as d:
        res['png_encode_770_files'] = stats(timed(lambda: write_all(want, d), a.host_reps, 1))
    # bytes the seven render calls must move at least: grey 4 + 1 per pixel (five images), heat map 4 + 4, overlay 4 + 4 + 1 + 3
    res['bytes_model'] = {'read': S * R * R * (5 * 4 + 4 + 9), 'write': S * R * R * (5 + 4 + 3)}
    if a.host_only:
        res['device'] = None
        res['note'] = 'host statement and PNG encoding only: not measured on the GPU'
    else:
        import torch
        from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
        assert torch.cuda.is_available(), 'render_bench needs the GPU (or --host-only)'
        eng = DeviceOps()
        res['device'] = torch.cuda.get_device_name(0)
        res['device_with_upload'] = stats(timed(lambda: device_render(eng, w), a.reps, 3))
        wd = {k: torch.from_numpy(v).to(eng.device) for k, v in w.items()}
        res['device_resident'] = stats(timed(lambda: device_render(eng, wd), a.reps, 3))

        def launches():
            device_ops = [eng.render_gray(wd[k]) for k in GREY] + [eng.render_gray(wd['gt']), eng.render_heatmap(wd['diff_filtered']),
                                                                  eng.render_overlay(wd['x'], wd['pred'], wd['gt'])]
            torch.cuda.synchronize()
            return device_ops
        res['device_resident_without_download'] = stats(timed(launches, a.reps, 3))
        # agreement at the timed size (the GPU tests hold the bar; this is the record beside the timing)
        got = device_render(eng, wd)
        res['agreement'] = {'grey_bytes_differ': int(np.count_nonzero(got[0] != want[0])), 'overlay_bytes_differ': int(np.count_nonzero(got[2] != want[2])),
                            'heatmap_pixels_differ': int(np.count_nonzero((got[1] != want[1]).any(axis=3))), 'heatmap_pixels': S * R * R}
        res['speedup_with_upload'] = res['host']['median_ms'] / res['device_with_upload']['median_ms']
        res['speedup_resident'] = res['host']['median_ms'] / res['device_resident']['median_ms']
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
