"""Shared by tests/test_resize_host.py (CPU, the host statement), tests/test_resize_kernels_host.py (CPU, the kernel source compiled for the
host) and tests/test_gpu_resize.py (the device): the shapes and inputs the resize op is held on, the reference -- always the host statement
utils/resize.py, which tests/test_resize_host.py pins against torch and a scalar restatement -- and the BrainWeb phantom of the ingestion
tests with the literal per-slice loop it is compared against.  Computed once per case and cached; callers must not write into what they get.

CASES (h, w) -> (H, W): the smallest downscale, a size-1 axis, small odd sizes, the nearest-neighbour quirk down and up (22 -> 18 and
14 -> 18), an upscale that takes both edge clamps, sizes one off a power of two, the workload's slice (217 x 181 -> 128 x 128: 16 row tiles),
and the workgroup tile of csrc/uad_resize.hip at -1, 0, +1: RS_TW = 128 output columns (127, 128, 129: the last is two column tiles and a
width that is no multiple of four, i.e. single-float stores) and RS_TH = 8 output rows (7, 8, 9)."""
import functools

import numpy as np

from unsupervised_anomaly_detection_brain_mri_amd.utils.resize import resize_linear, resize_nearest

RS_TW, RS_TH = 128, 8                # csrc/uad_resize.hip
BASE_CASES = [((2, 2), (1, 1)), ((1, 9), (1, 4)), ((3, 5), (2, 3)), ((7, 7), (3, 5)), ((22, 14), (18, 18)), ((64, 64), (128, 128)),
              ((65, 33), (64, 32)), ((129, 130), (128, 128)), ((217, 181), (128, 128))]
TILE_CASES = [((40, 150), (RS_TH - 1, RS_TW - 1)), ((40, 150), (RS_TH, RS_TW)), ((12, 100), (RS_TH + 1, RS_TW + 1))]
CASES = BASE_CASES + TILE_CASES
QUIRK_AXES = {(22, 18), (14, 18)}    # (src, dst) axes on which the fp64 nearest index differs from d * src // dst
MODES = ('linear', 'nearest')
KINDS = ('uniform', 'ramp', 'special')
INDEX = [3, 0, 6, 3, 5]              # non-monotone, one entry twice, into a 7-slice batch
N_RESIDENT = 7


def case_id(c):
    return '%dx%d-%dx%d' % (c[0] + c[1])


@functools.lru_cache(maxsize=None)
def batch(hw, kind, n=1):
    """[n, h, w] float32.  uniform: seeded [0, 1); ramp: 0, 1, 2, ... row-major, slice k shifted by 1000 k; special: +-0, denormals, +-1e30
    and ordinary values, shuffled."""
    h, w = hw
    rng = np.random.default_rng(7919 * h + 31 * w + n)
    if kind == 'uniform':
        a = rng.random((n, h, w), dtype=np.float32)
    elif kind == 'ramp':
        a = (np.arange(h * w, dtype=np.float32).reshape(1, h, w) + np.float32(1000) * np.arange(n, dtype=np.float32).reshape(n, 1, 1))
    else:
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-41, 1e30, -1e30, 1.0, -2.5, 0.3], np.float32)
        a = pool[rng.integers(0, pool.size, (n, h, w))]
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(hw, out_hw, mode, kind, n=1):
    with np.errstate(over='ignore', invalid='ignore'):          # the 1e30 entries may overflow to inf in a sum: the kernel must do the same
        r = (resize_linear if mode == 'linear' else resize_nearest)(batch(hw, kind, n), out_hw)
    r.setflags(write=False)
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- the BrainWeb phantom
SKULL_CLASSES = (4, 5, 6, 7, 9)      # FAT, MUSCLE, SKIN, SKULL, CONNECTIVE (dataloaders/BRAINWEB.py LABELS, :273-277)


@functools.lru_cache(maxsize=None)
def phantom(seed=0, shape=(12, 40, 36)):
    """(vol float64 with NaNs, tissue uint8 0..10 with all 11 classes).  Slice 0 is all background (constant 0 after background removal, not
    before), slice 1 is zero everywhere (constant whatever the flags), slice 2 is constant and non-zero under one kept class (it stays constant
    after the mask and the scaling); every other slice has structure."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing='ij')
    r = np.sqrt(x ** 2 + y ** 2)
    tissue = np.zeros(shape, np.uint8)
    tissue[r < 0.95] = 6                                                    # skin
    tissue[r < 0.9] = 7                                                     # skull
    tissue[r < 0.85] = 4                                                    # fat
    tissue[r < 0.8] = 1                                                     # CSF
    tissue[r < 0.7] = 2                                                     # GM
    tissue[r < 0.5] = 3                                                     # WM
    tissue[(r < 0.3) & (z % 2 == 0)] = 8                                    # glial matter
    tissue[(np.abs(x - 0.4) < 0.1) & (np.abs(y) < 0.15)] = 10               # lesion
    tissue[(np.abs(x + 0.6) < 0.05) & (np.abs(y) < 0.3)] = 5                # muscle
    tissue[(np.abs(y + 0.75) < 0.04) & (np.abs(x) < 0.3)] = 9               # connective
    vol = 300.0 + 200.0 * x + 80.0 * rng.standard_normal(shape) + 40.0 * (tissue == 10)
    vol[tissue == 0] = 25.0 * rng.random(shape)[tissue == 0]
    tissue[0] = 0
    vol[1] = 0.0
    tissue[2], vol[2] = 2, 120.0
    vol[5, 3, 4] = vol[7, 20, 18] = vol[9, 30, 30] = np.nan
    assert set(np.unique(tissue)) == set(range(11))
    vol.setflags(write=False); tissue.setflags(write=False)
    return vol, tissue


def brainweb_loop(vol, tissue, slice_start, slice_end, slice_resolution, skull_removal=True, background_removal=True, rotations=(0,),
                  center_crop=None):
    """dataloaders/BRAINWEB.py:125-185 and :266-292 slice by slice on an axial [z,y,x] volume, with utils/resize.py in the place of cv2.resize
    and the project's normalize_scaling in the place of NII.normalize.  -> (images, labels, kept)."""
    from scipy.ndimage import rotate

    from unsupervised_anomaly_detection_brain_mri_amd.utils.nifti import crop_center, normalize_scaling
    data = np.array(vol, np.float64)
    data[np.isnan(data)] = 0                                                # NII.py:12-16
    skullmap = tissue * 0.0 + 1.0                                           # :267
    if skull_removal:
        for c in SKULL_CLASSES:                                             # :272-277
            skullmap[tissue == c] = 0
    if background_removal:
        skullmap[tissue == 0] = 0                                           # :279-280
    seg = (tissue == 10).astype(np.float64)                                 # :283-286
    if skull_removal or background_removal:
        data = data * skullmap                                              # :288-289 (a masked negative voxel becomes -0, which compares equal to the package's +0)
    data = normalize_scaling(data, 0, 99.8)                                 # :292
    images, labels, kept = [], [], []
    for s in range(slice_start, min(slice_end, data.shape[0])):             # :125
        sd, ss = data[s], seg[s]
        if np.unique(sd).size == 1:                                         # :133
            continue
        if slice_resolution is not None:
            R = tuple(slice_resolution)
            if sd.shape[0] > R[0] or sd.shape[1] > R[1]:                    # :140-142: cv2 takes (width, height) = R
                sd = resize_linear(np.asarray(sd, np.float32), (R[1], R[0]))
                ss = resize_nearest(np.asarray(ss, np.float32), (R[1], R[0]))
            else:                                                           # :144-154
                tmp, tmp_seg = np.zeros(R), np.zeros(R)
                sx, sy = (R[1] - sd.shape[1]) // 2, (R[0] - sd.shape[0]) // 2
                tmp[sy:sy + sd.shape[0], sx:sx + sd.shape[1]] = sd
                tmp_seg[sy:sy + sd.shape[0], sx:sx + sd.shape[1]] = ss
                sd, ss = tmp.astype(np.float32), tmp_seg.astype(np.float32)
        for angle in rotations:                                             # :156-162
            sdr, ssr = (sd, ss) if angle == 0 else (rotate(sd, angle, reshape=False), rotate(ss, angle, reshape=False, mode='nearest'))
            if center_crop is not None:                                     # :175-177
                sdr, ssr = crop_center(sdr, center_crop[0], center_crop[1]), crop_center(ssr, center_crop[0], center_crop[1])
            images.append(np.asarray(sdr, np.float32)); labels.append(np.asarray(ssr, np.float32)); kept.append(s)
    return np.stack(images), np.stack(labels), kept
