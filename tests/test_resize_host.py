"""CPU: the host statement of the BrainWeb loader's two cv2.resize calls (utils/resize.py; dataloaders/BRAINWEB.py:140-142) and
nifti.volume_to_slices(loader='brainweb') on it (BRAINWEB.py:125-185, 266-292).  OpenCV is not a dependency, so the statement is held to what
can be had without it:

bilinear against torch.nn.functional.interpolate(fp64, mode='bilinear', align_corners=False), the same half-pixel coordinate rule in exact
    coordinates.  Bound per case: 1/2 (ulp32(h - 1) + ulp32(w - 1)) (max - min) + 8 * 2^-24 * max|a|.  The first term is the ONE rounding of
    each axis coordinate to fp32 that OpenCV's statement makes and the fp64 oracle does not -- a coordinate below src - 1 moves by at most
    half an ulp of src - 1, the interpolant's slope along an axis is at most max - min per sample; the second is the eight fp32 roundings of
    the weights (two) and the two passes (three each), each at most 2^-24 relative to a value no larger than max|a|.  Every case prints its
    error beside its bound; seen with the uniform input: <= 5.2e-7 on the nine base shapes (bounds 1.8e-7 .. 1.6e-5) and 4.7e-6 on the tile
    shapes, whose 150-sample axis has the coarsest coordinate ulp (bound 1.0e-5).
nearest against torch mode='nearest' (floor(d * src / dst) in its own arithmetic) on the cases whose fp64 index equals d * src // dst -- all
    but the 22 -> 18 and 14 -> 18 axes, which is asserted -- with the two quirk indices pinned literally.
both against a scalar, loop-written restatement, bit for bit.
volume_to_slices(loader='brainweb') against the literal per-slice loop of tests/resize_cases.py on a 12 x 40 x 36 phantom."""
import math

import numpy as np
import pytest
import torch

from tests import resize_cases as rc
from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti
from unsupervised_anomaly_detection_brain_mri_amd.utils.resize import linear_table, nearest_table, resize_linear, resize_nearest


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_bilinear_against_torch_fp64(case):
    (h, w), (H, W) = case
    for kind in ('uniform', 'ramp'):
        a = rc.batch((h, w), kind)
        want = torch.nn.functional.interpolate(torch.from_numpy(a.astype(np.float64))[None], size=(H, W), mode='bilinear', align_corners=False)[0].numpy()
        got = rc.reference((h, w), (H, W), 'linear', kind)
        bound = 0.5 * (_ulp32(h - 1) + _ulp32(w - 1)) * float(a.max() - a.min()) + 8 * 2.0 ** -24 * float(np.abs(a).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f'resize_linear {rc.case_id(case)} {kind}: max-abs err {err:.3e}, bound {bound:.3e}')
        assert got.dtype == np.float32 and got.shape == (1, H, W)
        assert err <= bound


def _nearest_is_integer_rule(src, dst):
    return np.array_equal(nearest_table(src, dst), np.arange(dst) * src // dst)


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_nearest_against_torch_where_the_index_rules_agree(case):
    (h, w), (H, W) = case
    agree = _nearest_is_integer_rule(h, H) and _nearest_is_integer_rule(w, W)
    # the split: only the 22 -> 18 and 14 -> 18 axes leave the integer rule
    assert agree == (not ({(h, H), (w, W)} & rc.QUIRK_AXES))
    for kind in rc.KINDS:
        a = rc.batch((h, w), kind)
        got = rc.reference((h, w), (H, W), 'nearest', kind)
        assert got.dtype == np.float32 and got.shape == (1, H, W)
        if agree:
            want = torch.nn.functional.interpolate(torch.from_numpy(a.copy())[None], size=(H, W), mode='nearest')[0].numpy()
            assert rc.same_bits(got, want), kind
        else:
            assert rc.same_bits(got, a[:, nearest_table(h, H)][:, :, nearest_table(w, W)])


def test_the_nearest_quirk_is_pinned():
    down, up = nearest_table(22, 18), nearest_table(14, 18)
    assert down[9] == 10 and 9 * 22 // 18 == 11                 # 9 * (1 / (18 / 22)) = 10.999999999999998
    assert up[9] == 6 and 9 * 14 // 18 == 7                     # 9 * (1 / (18 / 14)) = 6.999999999999999
    assert np.count_nonzero(down != np.arange(18) * 22 // 18) == 1 and np.count_nonzero(up != np.arange(18) * 14 // 18) == 1
    a = np.arange(22 * 14, dtype=np.float32).reshape(22, 14)
    out = resize_nearest(a, (18, 18))
    assert out[9, 9] == a[10, 6] and out[9, 0] == a[10, 0] and out[0, 9] == a[0, 6]


def test_the_edge_clamps_of_the_linear_table():
    s0, s1, w0, w1 = linear_table(64, 128)                      # upscale: d = 0 lies left of sample 0, d = 127 right of sample 63
    assert (s0[0], s1[0], w0[0], w1[0]) == (0, 1, 1.0, 0.0) and (s0[-1], s1[-1], w0[-1], w1[-1]) == (63, 63, 1.0, 0.0)
    assert (s0[1], s1[1], w0[1], w1[1]) == (0, 1, 0.75, 0.25)
    s0, s1, w0, w1 = linear_table(1, 4)                         # a size-1 axis: every tap is sample 0
    assert not s0.any() and not s1.any() and np.all(w0 == 1) and np.all(w1 == 0)
    s0, s1, w0, w1 = linear_table(2, 1)
    assert (s0[0], s1[0], w0[0], w1[0]) == (0, 1, 0.5, 0.5)
    assert w0.dtype == np.float32 and w1.dtype == np.float32


def _scalar_linear(a, H, W):
    h, w = a.shape
    f32 = np.float32

    def axis(d, src, dst):
        scale = 1.0 / (float(dst) / float(src))
        f = f32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = f32(f - f32(s))
        if s < 0:
            s, f = 0, f32(0)
        if s >= src - 1:
            s, f = src - 1, f32(0)
        return s, min(s + 1, src - 1), f32(f32(1) - f), f
    out = np.empty((H, W), f32)
    for Y in range(H):
        y0, y1, wy0, wy1 = axis(Y, h, H)
        for X in range(W):
            x0, x1, wx0, wx1 = axis(X, w, W)
            t0 = f32(f32(a[y0, x0] * wx0) + f32(a[y0, x1] * wx1))
            t1 = f32(f32(a[y1, x0] * wx0) + f32(a[y1, x1] * wx1))
            out[Y, X] = f32(f32(t0 * wy0) + f32(t1 * wy1))
    return out


def _scalar_nearest(a, H, W):
    h, w = a.shape
    out = np.empty((H, W), np.float32)
    for Y in range(H):
        y = min(math.floor(Y * (1.0 / (float(H) / float(h)))), h - 1)
        for X in range(W):
            out[Y, X] = a[y, min(math.floor(X * (1.0 / (float(W) / float(w)))), w - 1)]
    return out


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_a_scalar_restatement_gives_the_same_bits(case):
    """Every case; the outputs of more than 2048 pixels (the 128 x 128 ones, the workload's slice and the upscale that takes both edge clamps
    among them) on the input with +-0, denormals and 1e30 alone, which keeps the Python loops to a second or two."""
    (h, w), (H, W) = case
    for kind in (rc.KINDS if H * W <= 2048 else ('special',)):
        a = rc.batch((h, w), kind)[0]
        with np.errstate(over='ignore', invalid='ignore'):
            assert rc.same_bits(_scalar_linear(a, H, W), rc.reference((h, w), (H, W), 'linear', kind)[0]), kind
        assert rc.same_bits(_scalar_nearest(a, H, W), rc.reference((h, w), (H, W), 'nearest', kind)[0]), kind


def test_leading_axes_and_refusals():
    a = rc.batch((7, 7), 'uniform', 5)
    assert rc.same_bits(resize_linear(a.reshape(5, 1, 7, 7), (3, 5))[:, 0], resize_linear(a, (3, 5)))
    assert rc.same_bits(resize_linear(a[2], (3, 5)), resize_linear(a, (3, 5))[2])
    assert rc.same_bits(resize_nearest(a[2], (3, 5)), resize_nearest(a, (3, 5))[2])
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            resize_linear(a, bad)
    with pytest.raises(ValueError):
        resize_nearest(np.zeros(5, np.float32), (2, 2))


# ---------------------------------------------------------------------------------------------------------------- the BrainWeb loader
KW = dict(slice_start=0, slice_end=155)


@pytest.mark.parametrize('res', [(32, 32), (24, 30), (64, 64), (45, 41), (40, 36), (41, 30)], ids=lambda r: '%dx%d' % r)
def test_volume_to_slices_brainweb_against_the_literal_loop(res):
    """(32,32): resize; (24,30): resize, non-square -> output (30, 24), the shape quirk; (64,64): pad, even differences; (45,41): pad, odd
    differences; (40,36): the slice's own size, a pad of nothing; (41,30): larger on one axis only -> still a resize, to (30, 41)."""
    vol, tissue = rc.phantom()
    for skull, back in ((True, True), (True, False), (False, True), (False, False)):
        im, lb, kept = nifti.volume_to_slices(vol, tissue, loader='brainweb', slice_resolution=res, skull_removal=skull, background_removal=back, **KW)
        want = rc.brainweb_loop(vol, tissue, 0, 155, res, skull, back)
        assert kept == want[2] and im.dtype == np.float32 and lb.dtype == np.float32
        assert np.array_equal(im, want[0]) and np.array_equal(lb, want[1]), (skull, back)
        # slice 1 (all zero) and slice 2 (constant, non-zero) never survive; slice 0 is constant only once the background is removed
        assert 1 not in kept and 2 not in kept and (0 in kept) == (not back) and len(kept) == (9 if back else 10)
        resized = 40 > res[0] or 36 > res[1]
        assert im.shape[1:] == ((res[1], res[0]) if resized else res)
        assert set(np.unique(lb)) == {0.0, 1.0} and float(im.max()) <= 1.0
    assert not np.isnan(im).any()


def test_volume_to_slices_brainweb_rotations_crop_window_and_refusals():
    vol, tissue = rc.phantom()
    im, lb, kept = nifti.volume_to_slices(vol, tissue, loader='brainweb', slice_resolution=(32, 32), rotations=(0, 10), center_crop=(24, 20), slice_start=3,
                                          slice_end=8)
    want = rc.brainweb_loop(vol, tissue, 3, 8, (32, 32), rotations=(0, 10), center_crop=(24, 20))
    assert kept == want[2] == [3, 3, 4, 4, 5, 5, 6, 6, 7, 7] and im.shape == (10, 20, 24)
    assert np.array_equal(im, want[0]) and np.array_equal(lb, want[1])
    # no resolution: the kept slices as they are
    raw = nifti.volume_to_slices(vol, tissue, loader='brainweb', slice_resolution=None, **KW)
    want = rc.brainweb_loop(vol, tissue, 0, 155, None)
    assert raw[2] == want[2] and np.array_equal(raw[0], want[0]) and np.array_equal(raw[1], want[1])
    # a window with nothing but constant slices
    assert nifti.volume_to_slices(vol, tissue, loader='brainweb', slice_resolution=(32, 32), slice_start=1, slice_end=3)[2] == []
    with pytest.raises(ValueError):
        nifti.volume_to_slices(vol, tissue, loader='brainweb', curvature_flow=True)
    with pytest.raises(ValueError):
        nifti.volume_to_slices(vol, tissue, np.ones(vol.shape), loader='brainweb')
    with pytest.raises(ValueError):
        nifti.volume_to_slices(vol, None, loader='brainweb')
    with pytest.raises(ValueError):
        nifti.volume_to_slices(vol, tissue + 0.5, loader='brainweb')
    with pytest.raises(ValueError):
        nifti.volume_to_slices(vol, tissue, loader='brainwep')


def test_the_mslub_loader_is_unchanged_by_the_keyword():
    vol, tissue = rc.phantom()
    seg, brain = (tissue == 10).astype(np.float32), (tissue != 0).astype(np.float32)
    kw = dict(slice_start=0, slice_end=155, slice_resolution=(32, 32), rotations=(0, 10))
    a = nifti.volume_to_slices(vol, seg, brain, **kw)
    b = nifti.volume_to_slices(vol, seg, brain, loader='mslub', skull_removal=False, background_removal=False, **kw)
    assert a[2] == b[2] and len(a[2]) > 0
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_build_cache_passes_the_loader_keywords(tmp_path):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    patients = []
    for i in range(2):
        vol, tissue = rc.phantom(seed=40 + i)
        d = tmp_path / f'p{i}'
        d.mkdir()
        nifti.write_nifti(str(d / 't1.nii.gz'), np.nan_to_num(vol))
        nifti.write_nifti(str(d / 'classes.nii.gz'), tissue, dtype='u1')
        patients.append({'name': f'p{i}', 'volume': str(d / 't1.nii.gz'), 'groundtruth': str(d / 'classes.nii.gz'), 'skullmap': str(d / 'classes.nii.gz')})
    nifti.build_cache(str(tmp_path / 'bw'), patients, partition={'TRAIN': 0.5, 'VAL': 0.5}, seed=0, loader='brainweb', background_removal=False,
                      slice_resolution=(24, 30))
    images, labels, info = read_cache(str(tmp_path / 'bw'))
    order = [int(n[1:]) for n in dict.fromkeys(info['patients'])]
    want = [nifti.volume_to_slices(*(nifti.read_nifti(p[k])[0] for k in ('volume', 'groundtruth')), loader='brainweb', background_removal=False,
                                   slice_resolution=(24, 30)) for p in patients]
    w = np.concatenate([want[i][0] for i in order])
    assert images.shape == w.shape + (1,) and w.shape[1:] == (30, 24) and np.array_equal(images[..., 0], w)
    # the cache's label map (nifti.build_cache): 10 on the lesion map, 2 on every other non-zero pixel of the image, else 0
    lw = np.concatenate([want[i][1] for i in order])
    assert labels.dtype == np.uint8 and np.array_equal(labels, np.where(lw > 0, 10, np.where(w > 0, 2, 0)))
    assert (labels == 10).any() and (labels == 2).any() and (labels == 0).any()
