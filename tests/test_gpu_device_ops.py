"""GPU: the device ops need no model handle.  A fresh child interpreter -- the rest of the suite always has handles alive, so only a fresh
process shows that the ops' first launch needs nothing from uad_create -- builds a bare device_ops.DeviceOps, calls one op per kernel source
file at the smallest input that exercises it, and only then creates an AE handle and a GAN handle and repeats the calls on them: the three
objects must return the same bits.  The bits themselves are held to the host statements by the op tests (test_gpu_resize.py, ...)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[1])
from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
from unsupervised_anomaly_detection_brain_mri_amd.engine import Engine
from unsupervised_anomaly_detection_brain_mri_amd.gan_engine import GanEngine

rng = np.random.default_rng(7)
MASK55 = (rng.random((1, 5, 5)) < 0.8).astype(np.float32)
BLOBS = (rng.random((2, 4, 4)) < 0.4).astype(np.float32)
IMG44 = rng.random((1, 4, 4)).astype(np.float32)
IMG55 = rng.random((1, 5, 5)).astype(np.float32)
IMG234 = rng.random((2, 3, 4)).astype(np.float32)
VOL333 = rng.standard_normal((3, 3, 3))
IMG244 = rng.random((2, 4, 4)).astype(np.float32)
IMG157 = rng.standard_normal((1, 5, 7)).astype(np.float32)
NINE = rng.random(9).astype(np.float32)
SIXTEEN = rng.random(16).astype(np.float32)
CLASSES = (np.arange(16) % 2).astype(np.int64)
PRED, GT = rng.random(8).astype(np.float32), np.array([0, 1, 0, 0, 1, 1, 0, 1])


def run(o):
    r = {'erode_cross': o.erode_cross(MASK55, iterations=1),
         'cc_label': o.cc_label(BLOBS),
         'region_props': o.region_props(BLOBS),
         'zoom': o.zoom(IMG44, (6, 6)),
         'rotate': o.rotate(IMG55, 30.0),
         'resize_linear': o.resize(IMG234, (5, 7), mode='linear'),
         'resize_nearest': o.resize(IMG234, (5, 7), mode='nearest'),
         'curvature_flow': o.curvature_flow(VOL333, iterations=2),                    # two iterations: the workspace path
         'crop': o.crop(IMG244, np.array([[0, 0, 0], [1, 2, 1]]), (2, 2)),
         'render_gray': o.render_gray(IMG157),
         'render_heatmap': o.render_heatmap(IMG157),
         'quantile': o.quantile(NINE, 0.9)}
    for h in o.labelled_histogram(SIXTEEN, CLASSES, 4, (0.0, 1.0)):
        for k in ('n', 'bins', 'mean', 'var'):
            r[f"hist{h['class']}_{k}"] = h[k]
    r['auroc'] = o.scores(PRED, GT).auroc
    torch.cuda.synchronize()
    return r


def same(a, b):
    if isinstance(a, torch.Tensor):
        ints = {torch.float32: torch.int32, torch.float64: torch.int64}
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b) and \
            (a.dtype not in ints or torch.equal(a.view(ints[a.dtype]), b.view(ints[b.dtype])))
    if isinstance(a, np.ndarray):
        if not (isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape):
            return False
        if a.dtype.kind == 'f':
            a, b = a.view(f'u{a.dtype.itemsize}'), b.view(f'u{b.dtype.itemsize}')
        return np.array_equal(a, b)
    return struct.pack('<d', float(a)) == struct.pack('<d', float(b))              # host scalars: their 8 bytes


ops = DeviceOps()
assert not hasattr(ops, 'handle')
bare = run(ops)                                                                     # no handle exists in this process yet
assert len(bare) == 21 and bare['region_props'].shape[1] == 5 and bare['zoom'].shape == (1, 6, 6) and bare['rotate'].shape == (1, 1, 5, 5)
assert bare['curvature_flow'].dtype == torch.float64 and bare['render_heatmap'].shape == (1, 5, 7, 4) and bare['crop'].shape == (2, 2, 2)
ae = Engine('AE', 32, 32, 1, 8, 16, max_batch=1)
gan = GanEngine(32, 32, 1, 8, zdim=16, max_batch=2, variant='aae', aae_kind='aae')
for name, eng in (('Engine', ae), ('GanEngine', gan)):
    got = run(eng)
    assert got.keys() == bare.keys()
    for k in bare:
        assert same(bare[k], got[k]), (name, k, bare[k], got[k])
ae.close()
gan.close()
ops.close()
print('OK')
'''


def test_ops_need_no_handle_and_every_owner_returns_the_same_bits():
    p = subprocess.run([sys.executable, '-c', SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == 'OK', p.stdout + p.stderr
