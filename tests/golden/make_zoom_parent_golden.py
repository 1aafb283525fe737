"""Records tests/golden/zoom_parent_golden.npz: what engine.zoom returned on one case of tests/test_gpu_resample.py's list (100x60 -> 50x90,
three slices, both modes, fp32 and int32 output) with the library of the commit BEFORE the prefilter kernels of csrc/uad_resample.hip got their
boundary parameter (the commit that added uad_affine_spline3).  tests/test_gpu_rotate.py holds the current library to these bits.

    UAD_LIB=<libuad_hip.so built from that parent commit> python tests/golden/make_zoom_parent_golden.py [out.npz]

Needs the GPU.  The file was recorded once and is not meant to be regenerated from a later library: that would compare the code with itself."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEED, N, CASE = 11, 3, (100, 60, 50, 90)


def main():
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    assert os.environ.get('UAD_LIB') and _lib.LIB_PATH == os.environ['UAD_LIB'], 'point UAD_LIB at the parent commit\'s library'
    import ctypes
    import torch  # noqa: F401  (before the library: _lib.load)
    parent = ctypes.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib.SYMBOLS if not hasattr(parent, k)]:     # entries newer than the parent: not bound for this recording
        del _lib.SYMBOLS[name]
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'zoom_parent_golden.npz')
    h, w, H, W = CASE
    a = np.random.default_rng(SEED).random((N, h, w)).astype(np.float32)
    m = (a * 3).astype(np.int64)
    eng = DeviceOps()
    rec = {'seed': np.int64(SEED), 'input': a}
    for mode in ('constant', 'nearest'):
        rec[f'f32_{mode}'] = eng.zoom(a, (H, W), mode=mode).cpu().numpy()
        rec[f'i32_{mode}'] = eng.zoom(m, (H, W), mode=mode, integer=True).cpu().numpy()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(out, {k: (v.shape, str(v.dtype)) for k, v in rec.items()})


if __name__ == '__main__':
    main()
