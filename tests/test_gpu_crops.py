"""GPU: the device component measurements (uad_cc_props behind device_ops.DeviceOps.region_props), the window gather (uad_crop2d behind
device_ops.DeviceOps.crop) and the crop modes of the slice ingestion on them (nifti.volume_to_slices(crops=..., engine=...),
nifti.build_cache).

The reference is always the host statement utils/crops.py (pinned by tests/test_crops_host.py against literal restatements of the reference
lines), never the code under test; volumes, batches, windows and references come from tests/crops_cases.py, computed once and shared.  The
measurements are integers accumulated with integer atomics and the gather copies words, so every comparison is EQUALITY (the gather's
through uint32 views)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import crops_cases as cc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti
except Exception:
    DeviceOps = None


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def _hold(eng, shape, kind, slab):
    want = cc.props_reference(shape, kind, slab)
    got = eng.region_props(cc.mask(shape, kind).copy(), slab=slab)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 5
    assert np.array_equal(got, want), (shape, kind, slab, got.shape, want.shape)
    return want


@pytest.mark.parametrize('shape', cc.PROPS_SHAPES, ids=cc.shape_id)
def test_region_props_equal_the_host_statement(eng, shape):
    for kind in cc.KINDS:
        for slab in cc.SLABS:
            want = _hold(eng, shape, kind, slab)
            assert len(want) >= 1
    # a device-resident float mask and a label volume give the same table
    m = torch.from_numpy(cc.mask(shape, 'fill30').astype(np.float32)).to(eng.device)
    assert np.array_equal(eng.region_props(m, slab=1), cc.props_reference(shape, 'fill30', 1))
    assert np.array_equal(eng.region_props(eng.cc_label(m, slab=2)), cc.props_reference(shape, 'fill30', 2))
    assert np.array_equal(eng.region_props(cc.labels_model(shape, 'fill2', 0).copy()), cc.props_reference(shape, 'fill2', 0))


def test_region_props_structured_volumes(eng):
    for slab in cc.SLABS:
        want = _hold(eng, cc.SPAN_SHAPE, 'span', slab)            # one component through every tile
        assert len(want) == {0: 1, 1: 5, 2: 3}[slab]
        got = _hold(eng, cc.SPAN_SHAPE, 'empty', slab)
        assert got.shape == (0, 5)
        _hold(eng, (3, 9, 9), 'corner', slab)
        _hold(eng, (3, 9, 33), 'full', slab)
    assert eng.region_props(np.zeros(cc.SPAN_SHAPE, np.int32)).shape == (0, 5)          # an empty LABEL volume


def test_region_props_twice_and_beyond_the_first_table(eng):
    shape = (4, 128, 128)
    m = torch.from_numpy(cc.mask(shape, 'fill30').astype(np.float32)).to(eng.device)
    a, b = eng.region_props(m, slab=1), eng.region_props(m, slab=1)
    assert np.array_equal(a, b) and np.array_equal(a, cc.props_reference(shape, 'fill30', 1))
    # a label volume with more components than the 4096 rows tried first: isolated voxels on a 2-pixel grid
    iso = np.zeros((2, 128, 128), bool)
    iso[:, ::2, ::2] = True
    lab = eng.cc_label(iso, slab=1)
    got = eng.region_props(lab)
    assert got.shape == (8192, 5) and np.array_equal(got, cc.crops.component_props(iso, slab=1))


def test_cc_props_abi_cap_and_refusals(eng):
    shape, kind = (9, 16, 70), 'fill2'
    want = cc.props_reference(shape, kind, 1)
    assert len(want) > 8
    lab = torch.from_numpy(cc.labels_model(shape, kind, 1).copy()).to(eng.device)
    lib, st = eng.lib, eng._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    D, H, W = shape
    nbytes = int(lib.uad_cc_props_workspace(D, H, W))
    assert nbytes >= 4 * D * H * W
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=eng.device)
    n = torch.full((3,), -777, dtype=torch.int32, device=eng.device)
    guard = 0x5a5a5a5a5a5a5a5a
    for cap in (1, 7, len(want) - 1, len(want), len(want) + 5):
        rows = torch.full((len(want) + 8, 5), guard, dtype=torch.int64, device=eng.device)
        assert lib.uad_cc_props(p(lab), D, H, W, p(rows), cap, p(n[1:]), p(ws), st) == _lib.UAD_OK
        torch.cuda.synchronize()
        assert n.cpu().tolist() == [-777, len(want), -777], cap                       # the true count, whatever the cap
        k = min(cap, len(want))
        assert np.array_equal(rows[:k].cpu().numpy(), want[:k]), cap
        assert bool((rows[k:] == guard).all()), cap                                   # nothing past the cap (or the count) is written
    ok = (p(lab), D, H, W, p(rows), 4, p(n[1:]), p(ws), st)
    for pos, val in ((0, None), (1, 0), (2, -1), (3, 0), (4, None), (5, 0), (5, -3), (6, None), (7, None)):
        args = list(ok)
        args[pos] = val
        assert lib.uad_cc_props(*args) == 1, (pos, val)
    assert b'cc_props' in lib.uad_last_error()
    args = list(ok)
    args[1:4] = 2048, 1024, 1024                                                      # 2^31 voxels: refused before anything is launched
    assert lib.uad_cc_props(*args) == 1
    assert lib.uad_cc_props_workspace(2048, 1024, 1024) == 0 and lib.uad_cc_props_workspace(0, 4, 4) == 0
    torch.cuda.synchronize()
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'uad_hip.h')).read()
    for name in ('uad_cc_props_workspace', 'uad_cc_props', 'uad_crop2d'):
        assert name in _lib.SYMBOLS and name + '(' in header and hasattr(lib, name)


@pytest.mark.parametrize('size', cc.CROP_SIZES, ids=lambda s: '%dx%d' % s)
def test_crop_copies_the_words(eng, size):
    batch, origins, want = cc.crop_batch(), cc.crop_origins(size), cc.crop_reference(size)
    assert sorted(set((origins[:, 2] % 4).tolist())) == ([0, 1, 2, 3] if size[1] <= 64 else [0])
    resident = torch.from_numpy(batch.copy()).to(eng.device)
    before = resident.clone()
    got = eng.crop(resident, origins, size)                       # k = 7: repeated, non-monotone slices
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (7,) + size
    assert cc.same_bits(got.cpu().numpy(), want)
    for j in range(7):                                            # k = 1: the same window alone
        assert cc.same_bits(eng.crop(resident, origins[j:j + 1], size).cpu().numpy(), want[j:j + 1]), j
    assert cc.same_bits(eng.crop(batch.copy(), origins.tolist(), size).cpu().numpy(), want)           # from the host, origins as a list
    # an output that is not 16-byte aligned takes the single-word stores
    lib, st = eng.lib, eng._stream()
    od = torch.from_numpy(origins.copy()).to(eng.device)
    flat = torch.full((7 * size[0] * size[1] + 2,), -777.0, device=eng.device)
    assert lib.uad_crop2d(C.c_void_p(resident.data_ptr()), 7, 66, 72, C.c_void_p(od.data_ptr()), 7, size[0], size[1], C.c_void_p(flat.data_ptr() + 4), st) == _lib.UAD_OK
    torch.cuda.synchronize()
    flat = flat.cpu().numpy()
    assert flat[0] == -777.0 and flat[-1] == -777.0 and cc.same_bits(flat[1:-1].reshape(want.shape), want)
    assert torch.equal(resident.view(torch.int32), before.view(torch.int32))


def test_crop_refusals_and_the_abi(eng):
    a = torch.from_numpy(cc.crop_batch().copy()).to(eng.device)
    empty = eng.crop(a, np.zeros((0, 3), np.int32), (3, 5))
    assert tuple(empty.shape) == (0, 3, 5) and empty.dtype == torch.float32
    assert tuple(eng.crop(a, [], (3, 5)).shape) == (0, 3, 5)
    for bad in ([[7, 0, 0]], [[-1, 0, 0]], [[0, -1, 0]], [[0, 0, -1]], [[0, 64, 0]], [[0, 0, 68]], [[0, 0]], [[0.5, 0, 0]]):
        with pytest.raises(ValueError):
            eng.crop(a, bad, (3, 5))
    for bad_hw in ((0, 5), (3, 0), (67, 5), (3, 73)):
        with pytest.raises(ValueError):
            eng.crop(a, [[0, 0, 0]], bad_hw)
    with pytest.raises(ValueError):
        eng.crop(a[0], [[0, 0, 0]], (3, 5))
    lib, st = eng.lib, eng._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    od = torch.zeros((4, 3), dtype=torch.int32, device=eng.device)
    out = torch.empty((4, 3, 5), device=eng.device)
    ok = (p(a), 7, 66, 72, p(od), 4, 3, 5, p(out), st)
    assert lib.uad_crop2d(*ok) == _lib.UAD_OK
    for pos, val in ((0, None), (1, 0), (2, 0), (3, -1), (4, None), (5, 0), (6, 0), (7, 0), (6, 67), (7, 73), (8, None), (8, p(a))):
        args = list(ok)
        args[pos] = val
        assert lib.uad_crop2d(*args) == 1, (pos, val)
    assert b'crop2d' in lib.uad_last_error()
    args = list(ok)
    args[5] = 65536                                               # one grid holds 65535 windows: UAD_ERR_UNSUPPORTED (3), nothing is launched
    assert lib.uad_crop2d(*args) == 3
    torch.cuda.synchronize()


SPECS = [('center', 20, 16), ('lesions', 16, 12), ('lesions', 15, 11), ('random', 16, 12, 3)]


@pytest.mark.parametrize('loader', ['mslub', 'brainweb'])
def test_volume_to_slices_crops_on_the_device_against_the_host_call(eng, loader):
    args, kw = cc.loader_inputs(loader)
    for res in ((None,) if loader == 'mslub' else (None, (32, 32))):                  # (32, 32): the resized BrainWeb slices, bit-equal on the device
        for spec in SPECS:
            im_h, lb_h, kept_h = nifti.volume_to_slices(*args, crops=spec, rng=np.random.RandomState(7), slice_resolution=res, **kw)
            im_d, lb_d, kept_d = nifti.volume_to_slices(*args, crops=spec, rng=np.random.RandomState(7), slice_resolution=res, engine=eng, **kw)
            assert kept_d == kept_h and len(kept_h) >= 11, (spec, res)
            assert im_d.dtype == im_h.dtype == np.float32 and lb_d.dtype == lb_h.dtype == np.float32
            assert im_d.shape == im_h.shape == (len(kept_h), spec[2], spec[1])
            assert cc.same_bits(im_d, im_h) and cc.same_bits(lb_d, lb_h), (spec, res)
            if spec[0] == 'lesions':
                assert lb_h.any(axis=(1, 2)).all()                # every lesion crop holds its lesion
    # the refusals hold with an engine too; a window without a kept slice gives no crop
    with pytest.raises(ValueError):
        nifti.volume_to_slices(*args, crops=('lesions', 16, 12), rotations=(0, 10), engine=eng, **kw)
    with pytest.raises(ValueError):
        nifti.volume_to_slices(*args, crops=('random', 44, 12, 2), engine=eng, **kw)
    none = nifti.volume_to_slices(*args, crops=('lesions', 16, 12), engine=eng, **{**kw, 'slice_start': 11, 'slice_end': 12})
    assert none[0].shape == (0, 12, 16) and none[2] == []
    none = nifti.volume_to_slices(*args, crops=('lesions', 16, 12), engine=eng, **{**kw, 'slice_start': 0, 'slice_end': 2})      # slices without a lesion
    assert none[0].shape == (0, 12, 16) and none[2] == []


def test_volume_to_slices_random_crops_of_rotated_slices(eng):
    """The rotated batch stays on the device and is cropped there; the origins are the host's, the rotated values are held to the fp32
    rounding of the device spline as in tests/test_gpu_rotate.py (1.2e-7), the angle-0 crops to equality."""
    args, kw = cc.loader_inputs('brainweb')
    spec = ('random', 16, 12, 2)
    kw = {**kw, 'slice_start': 3, 'slice_end': 7, 'rotations': (0, 10), 'crops': spec}
    im_h, lb_h, kept_h = nifti.volume_to_slices(*args, rng=np.random.RandomState(3), **kw)
    im_d, lb_d, kept_d = nifti.volume_to_slices(*args, rng=np.random.RandomState(3), engine=eng, **kw)
    assert kept_d == kept_h == [s for s in (3, 4, 5, 6) for _ in range(4)] and im_d.shape == im_h.shape == (16, 12, 16)
    err = float(np.abs(im_d.astype(np.float64) - im_h.astype(np.float64)).max())
    lerr = float(np.abs(lb_d.astype(np.float64) - lb_h.astype(np.float64)).max())
    print(f'random crops of rotated slices: images max-abs err {err:.3e}, labels {lerr:.3e}')
    assert err <= 1.2e-7 and lerr <= 1.2e-7
    unrotated = [i for i in range(16) if (i // 2) % 2 == 0]
    assert cc.same_bits(im_d[unrotated], im_h[unrotated]) and cc.same_bits(lb_d[unrotated], lb_h[unrotated])


def test_build_cache_with_crops(eng, tmp_path):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    patients = []
    for i in range(2):
        vol, seg, brainmask, _ = cc.phantom(seed=40 + i)
        d = tmp_path / f'p{i}'
        d.mkdir()
        nifti.write_nifti(str(d / 'flair.nii.gz'), vol)
        nifti.write_nifti(str(d / 'gt.nii.gz'), seg, dtype='u1')
        nifti.write_nifti(str(d / 'mask.nii.gz'), brainmask, dtype='u1')
        patients.append({'name': f'p{i}', 'volume': str(d / 'flair.nii.gz'), 'groundtruth': str(d / 'gt.nii.gz'), 'skullmap': str(d / 'mask.nii.gz')})
    for spec in (('lesions', 16, 12), ('random', 16, 12, 2)):
        kw = dict(slice_start=0, slice_end=155, slice_resolution=None, crops=spec)
        where = str(tmp_path / spec[0])
        nifti.build_cache(where, patients, partition={'TRAIN': 0.5, 'VAL': 0.5}, seed=0, engine=eng, rng=np.random.RandomState(11), **kw)
        images, labels, info = read_cache(where)
        order = [int(n[1:]) for n in dict.fromkeys(info['patients'])]
        rng = np.random.RandomState(11)                           # one stream serves the patients in the order they are visited: 0, 1
        want = [nifti.volume_to_slices(*(nifti.read_nifti(p[k])[0] for k in ('volume', 'groundtruth', 'skullmap')), rng=rng, **kw) for p in patients]
        w = np.concatenate([want[i][0] for i in order])
        lw = np.concatenate([want[i][1] for i in order])
        assert images.shape == w.shape + (1,) and len(order) == 2 and w.shape[1:] == (12, 16)
        assert np.array_equal(images[..., 0], w)
        assert labels.dtype == np.uint8 and np.array_equal(labels, np.where(lw > 0, 10, np.where(w > 0, 2, 0)))
        assert (labels == 10).any() and info['options']['crops'] == list(spec) and 'rng' not in info['options']
