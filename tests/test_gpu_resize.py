"""GPU: the device resize op (uad_resize2d through device_ops.DeviceOps.resize), the tissue-class masking (uad_mask_by_label through
device_ops.DeviceOps.mask_by_label) and the BrainWeb ingestion on them (nifti.volume_to_slices(loader='brainweb', engine=...), nifti.build_cache).

The reference is always the host statement utils/resize.py (pinned by tests/test_resize_host.py) or numpy, never the code under test; shapes,
inputs and references come from tests/resize_cases.py, computed once and shared.  The kernel performs the host statement's IEEE operations
in the same order with contraction off and hipcc's correctly rounded fp64 division, so the bar of the ops is BIT EQUALITY; so is the bar of
the ingestion without rotations (the same kept slices, array_equal images and labels).  Rotated outputs are held to the 1.2e-7 of
tests/test_gpu_rotate.py, the final fp32 rounding of the device spline."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import resize_cases as rc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti
except Exception:
    DeviceOps = None

F32_BAR = 1.2e-7            # tests/test_gpu_rotate.py


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def _differ(got, ref):
    return int(np.count_nonzero(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32)))


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_device_result_has_the_bits_of_the_host_statement(eng, case):
    hw, out_hw = case
    for mode in rc.MODES:
        for kind in rc.KINDS:
            for n in (1, 5):
                got = eng.resize(rc.batch(hw, kind, n).copy(), out_hw, mode=mode)
                assert got.dtype == torch.float32 and tuple(got.shape) == (n,) + out_hw and got.is_cuda
                ref = rc.reference(hw, out_hw, mode, kind, n)
                g = got.cpu().numpy()
                print(f'resize {rc.case_id(case)} {mode} {kind} n={n}: {_differ(g, ref)} pixels differ')
                assert rc.same_bits(g, ref), (mode, kind, n)


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_the_slice_gather_from_a_resident_batch(eng, case):
    hw, out_hw = case
    resident = torch.from_numpy(rc.batch(hw, 'uniform', rc.N_RESIDENT).copy()).to(eng.device)
    before = resident.clone()
    for mode in rc.MODES:
        ref = rc.reference(hw, out_hw, mode, 'uniform', rc.N_RESIDENT)
        got = eng.resize(resident, out_hw, mode=mode, index=rc.INDEX).cpu().numpy()          # non-monotone, one entry twice
        assert rc.same_bits(got, ref[rc.INDEX]), mode
        assert rc.same_bits(eng.resize(resident, out_hw, mode=mode).cpu().numpy(), ref)
        # a slice's bits depend on neither n nor its place in the batch
        assert rc.same_bits(eng.resize(resident[4:5], out_hw, mode=mode).cpu().numpy(), ref[4:5])
        assert rc.same_bits(eng.resize(resident, out_hw, mode=mode, index=torch.tensor([4])).cpu().numpy(), ref[4:5])
    assert torch.equal(resident.view(torch.int32), before.view(torch.int32))


def test_resize_refusals_and_the_abi(eng):
    a = torch.from_numpy(rc.batch((7, 7), 'uniform', 5).copy()).to(eng.device)
    assert tuple(eng.resize(a, (3, 5), index=[]).shape) == (0, 3, 5)
    for bad in (dict(index=[5]), dict(index=[-1]), dict(index=[[0, 1]]), dict(index=[0.5]), dict(mode='cubic')):
        with pytest.raises(ValueError):
            eng.resize(a, (3, 5), **bad)
    for bad_hw in ((0, 5), (3, 0)):
        with pytest.raises(ValueError):
            eng.resize(a, bad_hw)
    with pytest.raises(ValueError):
        eng.resize(a[0], (3, 5))
    # the C boundary: UAD_ERR_INVALID (1) for non-positive sizes, an unknown mode, NULL pointers, out aliasing in, NULL index with n != n_in
    lib, st = eng.lib, eng._stream()
    out = torch.empty((5, 3, 5), device=eng.device)
    idx = torch.zeros(5, dtype=torch.int32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = (p(a), 5, 7, 7, p(idx), 5, 3, 5, _lib.RESIZE_LINEAR, p(out), st)
    assert lib.uad_resize2d(*ok) == _lib.UAD_OK
    for pos, val in ((1, 0), (2, 0), (3, -1), (5, 0), (6, 0), (7, 0), (8, 2), (8, -1), (0, None), (9, None), (9, p(a))):
        args = list(ok)
        args[pos] = val
        assert lib.uad_resize2d(*args) == 1, (pos, val)
    args = list(ok)
    args[4], args[5] = None, 4
    assert lib.uad_resize2d(*args) == 1
    assert b'resize2d' in lib.uad_last_error()
    args = list(ok)
    args[5] = 65536                                             # one grid holds 65535 slices: UAD_ERR_UNSUPPORTED (3), nothing is launched
    assert lib.uad_resize2d(*args) == 3
    lab = torch.zeros(16, dtype=torch.uint8, device=eng.device)
    lut = torch.ones(256, dtype=torch.uint8, device=eng.device)
    v = torch.ones(16, device=eng.device)
    okm = (p(v), p(lab), 16, p(lut), p(v), None, 10, st)
    assert lib.uad_mask_by_label(*okm) == _lib.UAD_OK
    for pos, val in ((0, None), (1, None), (2, 0), (3, None), (4, None), (5, p(v))):
        args = list(okm)
        args[pos] = val
        assert lib.uad_mask_by_label(*args) == 1, (pos, val)
    torch.cuda.synchronize()
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'uad_hip.h')).read()
    for name in ('uad_resize2d', 'uad_mask_by_label'):
        assert name in _lib.SYMBOLS and name + '(' in header and hasattr(lib, name)


def test_mask_by_label_against_numpy(eng):
    from tests.test_resize_kernels_host import mask_inputs
    vol, labels, lut = mask_inputs()                            # 4099 values, all 256 label bytes
    assert set(labels.tolist()) == set(range(256))
    keep = np.flatnonzero(lut).tolist()
    want = np.where(lut[labels] != 0, vol, np.float32(0))
    for lesion_label in (None, 10):
        # out of place, from host arrays; the input of a device call stays as it was
        got = eng.mask_by_label(vol.copy(), labels.copy(), keep, lesion_label)
        masked, lesion = got if lesion_label is not None else (got, None)
        assert rc.same_bits(masked.cpu().numpy(), want)
        dv = torch.from_numpy(vol.copy()).to(eng.device)
        dl = torch.from_numpy(labels.copy()).to(eng.device)
        got = eng.mask_by_label(dv, dl, keep, lesion_label)
        masked2 = got[0] if lesion_label is not None else got
        assert masked2.data_ptr() != dv.data_ptr() and rc.same_bits(dv.cpu().numpy(), vol) and rc.same_bits(masked2.cpu().numpy(), want)
        # in place
        got = eng.mask_by_label(dv, dl, keep, lesion_label, out=dv)
        masked3 = got[0] if lesion_label is not None else got
        assert masked3.data_ptr() == dv.data_ptr() and rc.same_bits(dv.cpu().numpy(), want)
        if lesion_label is not None:
            assert rc.same_bits(lesion.cpu().numpy(), (labels == 10).astype(np.float32)) and rc.same_bits(got[1].cpu().numpy(), (labels == 10).astype(np.float32))
    # an unaligned view takes the element-wise path
    dv = torch.from_numpy(vol.copy()).to(eng.device)
    dl = torch.from_numpy(labels.copy()).to(eng.device)
    m, les = eng.mask_by_label(dv[1:], dl[1:], keep, 10)
    assert rc.same_bits(m.cpu().numpy(), want[1:]) and rc.same_bits(les.cpu().numpy(), (labels[1:] == 10).astype(np.float32))
    with pytest.raises((TypeError, ValueError)):
        eng.mask_by_label(vol, labels.astype(np.int32), keep)
    with pytest.raises(ValueError):
        eng.mask_by_label(vol, labels[:-1], keep)
    with pytest.raises(ValueError):
        eng.mask_by_label(vol, labels, [256])


@pytest.mark.parametrize('res', [(32, 32), (24, 30), (45, 41)], ids=lambda r: '%dx%d' % r)
def test_volume_to_slices_brainweb_on_the_device_against_the_host_call(eng, res):
    """(32,32): resize; (24,30): resize to the swapped shape (30, 24); (45,41): pad with odd differences."""
    vol, tissue = rc.phantom()
    for skull, back in ((True, True), (False, False), (True, False)):
        kw = dict(loader='brainweb', slice_start=0, slice_end=155, slice_resolution=res, skull_removal=skull, background_removal=back)
        im_h, lb_h, kept_h = nifti.volume_to_slices(vol, tissue, **kw)
        im_d, lb_d, kept_d = nifti.volume_to_slices(vol, tissue, engine=eng, **kw)
        assert kept_d == kept_h and len(kept_h) == (9 if back else 10)
        assert im_d.dtype == im_h.dtype and lb_d.dtype == lb_h.dtype and im_d.shape == im_h.shape
        print(f'volume_to_slices(brainweb, {res}, skull={skull}, background={back}): {_differ(im_d, im_h)} image pixels differ in bits')
        assert np.array_equal(im_d, im_h) and np.array_equal(lb_d, lb_h)
    # a window of constant slices only, and no resolution at all
    assert nifti.volume_to_slices(vol, tissue, loader='brainweb', engine=eng, slice_start=1, slice_end=3, slice_resolution=res)[2] == []
    raw_h = nifti.volume_to_slices(vol, tissue, loader='brainweb', slice_resolution=None)
    raw_d = nifti.volume_to_slices(vol, tissue, loader='brainweb', slice_resolution=None, engine=eng)
    assert raw_d[2] == raw_h[2] and np.array_equal(raw_d[0], raw_h[0]) and np.array_equal(raw_d[1], raw_h[1])


def test_volume_to_slices_brainweb_with_rotations(eng):
    vol, tissue = rc.phantom()
    kw = dict(loader='brainweb', slice_start=3, slice_end=9, slice_resolution=(32, 32), rotations=(0, 10), center_crop=(24, 20))
    im_h, lb_h, kept_h = nifti.volume_to_slices(vol, tissue, **kw)
    im_d, lb_d, kept_d = nifti.volume_to_slices(vol, tissue, engine=eng, **kw)
    assert kept_d == kept_h and im_d.shape == im_h.shape == (12, 20, 24)
    err = float(np.abs(im_d.astype(np.float64) - im_h.astype(np.float64)).max())
    lerr = float(np.abs(lb_d.astype(np.float64) - lb_h.astype(np.float64)).max())
    print(f'volume_to_slices(brainweb, rotations (0, 10)): images max-abs err {err:.3e}, labels {lerr:.3e}')
    assert err <= F32_BAR and lerr <= F32_BAR
    assert np.array_equal(im_d[0::2], im_h[0::2]) and np.array_equal(lb_d[0::2], lb_h[0::2])          # angle 0 passes through


def test_build_cache_with_the_brainweb_loader(eng, tmp_path):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    patients = []
    for i in range(2):
        vol, tissue = rc.phantom(seed=40 + i)
        d = tmp_path / f'p{i}'
        d.mkdir()
        nifti.write_nifti(str(d / 't1.nii.gz'), vol)
        nifti.write_nifti(str(d / 'classes.nii.gz'), tissue, dtype='u1')
        patients.append({'name': f'p{i}', 'volume': str(d / 't1.nii.gz'), 'groundtruth': str(d / 'classes.nii.gz')})
    kw = dict(loader='brainweb', slice_start=0, slice_end=155, slice_resolution=(32, 32))
    nifti.build_cache(str(tmp_path / 'bw'), patients, partition={'TRAIN': 0.5, 'VAL': 0.5}, seed=0, engine=eng, **kw)
    images, labels, info = read_cache(str(tmp_path / 'bw'))
    order = [int(n[1:]) for n in dict.fromkeys(info['patients'])]
    want = [nifti.volume_to_slices(*(nifti.read_nifti(p[k])[0] for k in ('volume', 'groundtruth')), **kw) for p in patients]
    w = np.concatenate([want[i][0] for i in order])
    assert images.shape == w.shape + (1,) and len(order) == 2
    assert np.array_equal(images[..., 0], w)
    # the cache's label map (nifti.build_cache): 10 on the lesion map, 2 on every other non-zero pixel of the image, else 0
    lw = np.concatenate([want[i][1] for i in order])
    assert labels.dtype == np.uint8 and np.array_equal(labels, np.where(lw > 0, 10, np.where(w > 0, 2, 0)))
    assert (labels == 10).any() and (labels == 2).any()
