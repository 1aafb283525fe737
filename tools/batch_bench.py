"""The context-encoder masking of a ceVAE step on its two routes -- the host round trip of retrieve_masked_batch against the device route of
trainers/CE.py: masked_shard -- and the device time of uad_assemble_batch in its four forms.

    python tools/batch_bench.py [--out profiles/r16_batch.json] [--epochs 5] [--slices 512] [--reps 50]

Workload: a synthetic DeviceDataset of `--slices` 128 x 128 TRAIN slices with a tissue-class map (a brain ellipse per slice), a ceVAE trainer
(zDim 128, intermediate resolution 8 x 8) at batch 64 and at batch 16.
  steps    wall time per step of one ceVAE process(TRAIN) epoch with trainer.host_context_mask = True (the batch and the brain masks are
           downloaded, the boxes come from np.nonzero, the product is formed on the host and uploaded again) and = False (boxes from the
           dataset's host table, squares drawn on the host, 48 bytes a sample uploaded, engine.context_mask on the device); the same
           trainer and dataset, the host route first, each after one warm-up epoch, `--epochs` (>= 5) timed epochs each; host clock around
           process(), which ends in the epoch's synchronisation; median / min / max over the epochs, divided by the steps of an epoch.
  assemble device time of DeviceOps.assemble_batch over the dataset's store for a batch of 64 and of 16: gather / gather + noise / gather + mask /
           all three; HIP events around `--reps` back-to-back calls, after a warm-up, so the figure is the time per call in a full queue: the
           kernel's time, or the host's time to issue a call where that is longer; next to the bytes the form must move (every source word
           read once, every output word written once) and the HBM rate that implies (a lower bound of the kernel's own rate).
The method is tools/resize_bench.py's; no threshold is set here.  Needs the GPU: there is no fallback."""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = W = 128


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': len(v)}


def labelled_slices(n, seed=0):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import synthetic_slices
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    cy, cx = rng.integers(H // 2 - 8, H // 2 + 9, (2, n, 1, 1))
    ry, rx = rng.integers(H // 4, H // 2 - 10, (2, n, 1, 1))
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    labels = np.where(inside, rng.integers(1, 4, (n, H, W)), 0).astype(np.uint8)
    return synthetic_slices(n, H, W, seed=seed), labels


def epoch_ms(model, ds, epochs):
    from unsupervised_anomaly_detection_brain_mri_amd.trainers import Phase
    out = []
    for e in range(epochs + 1):                                     # the first one is the warm-up
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            model.process(ds, e, Phase.TRAIN)
        if e:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r16_batch.json'))
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--slices', type=int, default=512)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    if a.epochs < 5:
        raise SystemExit('at least 5 timed epochs')
    import torch
    from unsupervised_anomaly_detection_brain_mri_amd.models import context_encoder_variational_autoencoder
    from unsupervised_anomaly_detection_brain_mri_amd.trainers import ceVAE
    from unsupervised_anomaly_detection_brain_mri_amd.utils.default_config_setup import get_config, get_options
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import DeviceDataset
    assert torch.cuda.is_available(), 'batch_bench needs the GPU'
    imgs, labels = labelled_slices(a.slices)
    res = {'workload': f'{a.slices} synthetic {H}x{W} slices with labels, ceVAE zDim 128, process(TRAIN)', 'device': torch.cuda.get_device_name(0),
           'steps': {}, 'assemble': {}}
    tmp = tempfile.mkdtemp()
    for bs in (64, 16):
        ds = DeviceDataset(imgs, np.zeros(a.slices, int), labels, seed=1)
        opt = get_options(batchsize=bs, learningrate=1e-4, numEpochs=1, zDim=128, outputWidth=W, outputHeight=H,
                          config={'CHECKPOINTDIR': os.path.join(tmp, 'ck'), 'SAMPLEDIR': os.path.join(tmp, 'smp')})
        cfg = get_config(ceVAE, opt, 'ADAM', [8, 8], 0.2, ds)
        model = ceVAE(None, cfg, network=context_encoder_variational_autoencoder, seed=3)
        model.mask_rng = random.Random(7)
        steps = ds.num_batches(bs)
        row = {'steps_per_epoch': steps}
        for name, host in (('host_route', True), ('device_route', False)):
            model.host_context_mask = host
            row[name + '_ms_per_step'] = stats([ms / steps for ms in epoch_ms(model, ds, a.epochs)])
        row['host_over_device'] = row['host_route_ms_per_step']['median'] / row['device_route_ms_per_step']['median']
        res['steps'][f'batch{bs}'] = row
        # the four forms of the assemble launch on this dataset's store
        eng = model.engine
        rng = np.random.default_rng(2)
        idx = ds.upload_int32(rng.integers(0, a.slices, bs).astype(np.int32)).clone()
        rects = np.zeros((bs, 3, 4), np.int32)
        rects[:, :2] = [(30, 40, 20, 20), (60, 50, 20, 20)]
        rects = torch.from_numpy(rects).to(eng.device)
        noise = (0.01, 1, 0, 0, DeviceDataset.NOISE_STREAM)
        words = bs * H * W
        forms = {'gather': (dict(index=idx), 2), 'gather_noise': (dict(index=idx, noise=noise), 2), 'gather_mask': (dict(index=idx, rects=rects), 3),
                 'gather_noise_mask': (dict(index=idx, rects=rects, noise=noise), 3)}
        table = {}
        for form, (kw, moved) in forms.items():
            for _ in range(5):
                eng.assemble_batch(ds._images, **kw)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            times = []
            for _ in range(5):
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(a.reps):
                    eng.assemble_batch(ds._images, **kw)
                ev1.record()
                ev1.synchronize()
                times.append(ev0.elapsed_time(ev1) * 1e3 / a.reps)
            us = statistics.median(times)
            nbytes = moved * words * 4
            table[form] = {'us_per_call': us, 'bytes': nbytes, 'GBps': nbytes / us * 1e-3}
        res['assemble'][f'batch{bs}'] = table
        model.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
