"""Host scipy against the device spline resampler (uad_zoom_spline3) on the slice-ingestion step of the evaluation path.

    python tools/resample_bench.py [--out profiles/r08_resample.json] [--host-reps 3] [--reps 20]

Workload: one 110 x 217 x 181 patient -- the image ('constant', fp32 out) and two integer maps ('nearest', int32 out) -> 128 x 128 per slice
(utils/Evaluation.py:223-232), then the exportVolumes de-zoom of the 110 x 128 x 128 residual sub-volume back to 217 x 181 (:323-334).
  host    scipy.ndimage.zoom, three calls per slice as the reference's loop makes them, and the 3-D de-zoom; host clock.
  device  engine.zoom on host arrays, results downloaded to host arrays: H2D + three kernels per call + D2H, host clock around a call that
          ends in the download (which synchronises).  `device_resident_ms` is the same work on device-resident inputs between two events.
Every timed shape is warmed up first; median / min / max over the repetitions are reported.  The tool also records the difference the two
ingestion paths make to diff_AUC / diff_AUPRC / bestDiceScore of Evaluation.evaluate on the synthetic 80^2 -> 64^2 patients (a blur stand-in
model scored by the device ops).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import scipy.ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils.default_config_setup import get_options  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import SyntheticPatientDataset, synthetic_slices  # noqa: E402

S, NH, NW, R = 110, 217, 181, 128


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def host_ingest(x, seg, skull):
    zf = (R / NH, R / NW)
    for k in range(S):
        scipy.ndimage.zoom(x[k], zf)
        scipy.ndimage.zoom(seg[k], zf, mode='nearest')
        scipy.ndimage.zoom(skull[k], zf, mode='nearest')


def device_ingest(eng, x, seg, skull):
    a = eng.zoom(x, (R, R), mode='constant')
    b = eng.zoom(seg, (R, R), mode='nearest', integer=True)
    c = eng.zoom(skull, (R, R), mode='nearest', integer=True)
    return a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


class BlurModel:
    def __init__(self, engine):
        self.engine = engine
        self.config = types.SimpleNamespace(batchsize=16)
        self.network = types.SimpleNamespace(__name__='blur_network')
        self.model_dir = 'Blur_dSynthetic'

    def reconstruct(self, x, dropout=False, eps=None):
        x = np.asarray(x, np.float32)
        rec = scipy.ndimage.uniform_filter(x, size=(1, 9, 9, 1))
        return {'reconstruction': rec, 'l1err': np.abs(x - rec).sum(), 'l2err': np.abs(x - rec).sum()}


def metric_differences(eng):
    with tempfile.TemporaryDirectory() as tmp:
        def opts(**kw):
            o = get_options(batchsize=16, learningrate=1e-4, numEpochs=1, zDim=64, outputWidth=64, outputHeight=64, slices_start=0, slices_end=16,
                            config={'CHECKPOINTDIR': os.path.join(tmp, 'ck'), 'SAMPLEDIR': os.path.join(tmp, 'smp')})
            o.update(kw)
            return o
        ds = SyntheticPatientDataset(n_val=1, n_test=4, slices=16, native=80, h=64, w=64, seed=1, slice_start=0, slice_end=16)
        host = Evaluation.evaluate(ds, BlurModel(eng), opts(), epoch='bench', description='host')
        dev = Evaluation.evaluate(ds, BlurModel(eng), opts(resampleOnDevice=True), epoch='bench', description='device')
    return {k: {'host': float(host[k]), 'device': float(dev[k]), 'difference': float(dev[k]) - float(host[k])} for k in ('diff_AUC', 'diff_AUPRC', 'bestDiceScore')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r08_resample.json'))
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'resample_bench needs the GPU'
    eng = DeviceOps()
    x4, lab, msk = synthetic_slices(S, NH, NW, seed=7, lesions=True)
    x, seg, skull = x4[..., 0].astype(np.float64), lab.astype(int), msk.astype(int)
    sub = np.clip(scipy.ndimage.gaussian_filter(np.random.default_rng(3).random((S, R, R)), 1.0) - 0.45, 0, None).astype(np.float32)
    dezoom = (1, NH / R, NW / R)

    res = {'workload': f'{S}x{NH}x{NW} patient: image + 2 integer maps -> {R}x{R}; de-zoom {S}x{R}x{R} -> {NH}x{NW}', 'scipy': scipy.__version__,
           'device': torch.cuda.get_device_name(0)}
    res['host_ingest'] = stats(timed(lambda: host_ingest(x, seg, skull), a.host_reps, 1))
    res['host_dezoom'] = stats(timed(lambda: scipy.ndimage.zoom(sub.astype(np.float64), dezoom), a.host_reps, 1))
    res['device_ingest_with_copies'] = stats(timed(lambda: device_ingest(eng, x, seg, skull), a.reps, 3))
    res['device_dezoom_with_copies'] = stats(timed(lambda: eng.zoom(sub, (NH, NW)).cpu().numpy(), a.reps, 3))
    xd, sd, kd, subd = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(eng.device) for v in (x, seg, skull, sub))

    def resident():
        eng.zoom(xd, (R, R)); eng.zoom(sd, (R, R), mode='nearest', integer=True); eng.zoom(kd, (R, R), mode='nearest', integer=True)
    res['device_ingest_resident'] = stats(event_timed(resident, a.reps, 3))
    res['device_dezoom_resident'] = stats(event_timed(lambda: eng.zoom(subd, (NH, NW)), a.reps, 3))
    # agreement at the timed size (the GPU tests hold the bars; this is the record beside the timing)
    got = device_ingest(eng, x, seg, skull)
    zf = (R / NH, R / NW)
    res['agreement'] = {
        'image_max_abs_err': float(max(np.abs(got[0][k] - scipy.ndimage.zoom(x[k], zf)).max() for k in range(0, S, 10))),
        'label_voxels_differing': int(sum(np.count_nonzero(got[1][k] != scipy.ndimage.zoom(seg[k], zf, mode='nearest')) for k in range(0, S, 10))),
        'skull_voxels_differing': int(sum(np.count_nonzero(got[2][k] != scipy.ndimage.zoom(skull[k], zf, mode='nearest')) for k in range(0, S, 10))),
        'slices_checked': len(range(0, S, 10))}
    res['speedup_ingest_with_copies'] = res['host_ingest']['median_ms'] / res['device_ingest_with_copies']['median_ms']
    res['speedup_dezoom_with_copies'] = res['host_dezoom']['median_ms'] / res['device_dezoom_with_copies']['median_ms']
    # bytes the three kernels must move per call (fp32 in, fp64 coefficients written + read + rewritten per axis, read by the taps, 4-byte out)
    coef = S * NH * NW * 8
    res['bytes_model_image_call'] = S * NH * NW * 4 + 7 * coef + S * R * R * 4
    res['evaluate_metric_differences'] = metric_differences(eng)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
