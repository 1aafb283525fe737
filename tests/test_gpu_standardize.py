"""GPU: the ordered sums and the standardization map (csrc/uad_moments.hip: uad_shifted_sums, uad_clamp_standardize) and their wiring
(device_ops.DeviceOps.shifted_sums / standardize, nifti.normalize_standardization, nifti.volume_to_slices(normalization='standardization'))
against the host statement utils/standardize.py: everything is BIT-EQUAL -- the order of summation is a function of n alone.  Sizes sit on
the run (32), tile (UAD_SELECT_TILE) and strided-run (256 tiles) edges."""
import numpy as np
import pytest
import torch

from tests import standardize_cases as sc
from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti
from unsupervised_anomaly_detection_brain_mri_amd.utils import standardize as st

pytestmark = pytest.mark.gpu
KW = dict(slice_start=0, slice_end=155, slice_resolution=(32, 32))


@pytest.fixture(scope='module')
def eng():
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    e = DeviceOps()
    yield e
    e.close()


def check(eng, t, v, lo=None, hi=None):
    """shifted_sums at the three settings of the statement and standardize, of device tensor t against the statement on its host copy v."""
    mean32, std32 = st.standardize_clamped(v, lo, hi, return_moments=True)[1]
    for shift, centre in ((0.0, 0.0), (mean32, 0.0), (mean32, np.float32(3e-6))):
        got, want = eng.shifted_sums(t, lo, hi, shift, centre), st.shifted_sums(v, lo, hi, shift, centre)
        assert np.array(got).tobytes() == np.array(want).tobytes(), (v.size, shift, centre, got, want)
    out, moments = eng.standardize(t, lo, hi, return_moments=True)
    assert out.data_ptr() != t.data_ptr() and out.cpu().numpy().tobytes() == st.standardize_clamped(v, lo, hi).tobytes(), v.size
    assert np.array(moments).tobytes() == np.array(eng.last_moments).tobytes() == np.array([mean32, std32]).tobytes()


@pytest.mark.parametrize('n', sc.GPU_SIZES)
def test_sums_and_standardize_equal_the_statement(eng, n):
    v = sc.values(n)
    check(eng, eng._dev(v), v)
    check(eng, eng._dev(v), v, -100.0, 650.0)


def test_offset_input(eng):
    v = sc.offset_values(13 * 17 * 19)
    check(eng, eng._dev(v), v)
    got = eng.shifted_sums(v, shift=1e4, centre=-1e-4)
    assert np.array(got).tobytes() == np.array(st.shifted_sums(v, shift=1e4, centre=-1e-4)).tobytes()


@pytest.mark.parametrize('start', [1, 2, 3])
def test_a_view_that_is_only_4_byte_aligned(eng, start):
    n = 3 * sc.T + 17
    v = sc.values(n + start)
    t = eng._dev(v)[start:]
    assert t.data_ptr() % 16 == 4 * start
    check(eng, t, v[start:], -100.0, 650.0)
    # in place on the view: the elements in front of it stay
    out = eng.standardize(t, -100.0, 650.0, out=t)
    assert out.data_ptr() == t.data_ptr() and out.cpu().numpy().tobytes() == st.standardize_clamped(v[start:], -100.0, 650.0).tobytes()


def test_two_calls_and_a_second_stream_give_the_same_bits(eng):
    n = 256 * sc.T + 1
    v = sc.values(n)
    t = eng._dev(v)
    first = eng.shifted_sums(t, None, 650.0, 117.0, 0.25)
    assert eng.shifted_sums(t, None, 650.0, 117.0, 0.25) == first == st.shifted_sums(v, None, 650.0, 117.0, 0.25)
    ref = eng.standardize(t).cpu().numpy().tobytes()
    torch.cuda.synchronize(eng.device)
    side = torch.cuda.Stream(eng.device)
    with torch.cuda.stream(side):
        assert eng.shifted_sums(t, None, 650.0, 117.0, 0.25) == first
        assert eng.standardize(t).cpu().numpy().tobytes() == ref
    side.synchronize()


def test_constant_volume_and_the_empty_array(eng):
    v = np.full(sc.T + 5, 0.7310586, np.float32)
    out = eng.standardize(v)
    assert eng.last_moments[1] == 0.0 and torch.isnan(out).all()
    assert eng.shifted_sums(np.zeros(0, np.float32)) == (0.0, 0.0)


def test_a_wrong_out_or_workspace_is_refused_before_any_launch(eng):
    t = eng._dev(sc.values(sc.T + 1))
    for bad in (torch.empty(sc.T, device=eng.device), torch.empty(sc.T + 1, device=eng.device, dtype=torch.float64), torch.empty(sc.T + 1),
                torch.empty(2 * (sc.T + 1), device=eng.device)[::2], np.empty(sc.T + 1, np.float32)):
        with pytest.raises(ValueError, match='out must be'):
            eng.standardize(t, out=bad)
    with pytest.raises(ValueError, match='workspace'):
        eng.shifted_sums(t, workspace=torch.empty(4, dtype=torch.float64))
    with pytest.raises(ValueError, match='workspace'):                      # too short: refused by the entry point, nothing launched
        eng.shifted_sums(t, workspace=torch.empty(2, device=eng.device, dtype=torch.float64))
    out = torch.empty((sc.T + 1, 1), device=eng.device)                        # another shape of the same size is fine
    assert eng.standardize(t, out=out) is out and type(eng).last_moments is None


def test_error_codes(eng):
    import ctypes as C
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import _ptr
    t = eng._dev(sc.values(sc.T + 1))
    sums = torch.empty(2, device=eng.device, dtype=torch.float64)
    ws = eng.shifted_sums_workspace(t.numel())
    call = lambda *a: eng.lib.uad_shifted_sums(*a, eng._stream())
    inf = float('inf')
    assert call(_ptr(t), t.numel(), -inf, inf, 0.0, 0.0, _ptr(sums), _ptr(ws), 32) == 0
    assert call(None, t.numel(), -inf, inf, 0.0, 0.0, _ptr(sums), _ptr(ws), 32) == 1                    # UAD_ERR_INVALID
    assert call(_ptr(t), t.numel(), -inf, inf, 0.0, 0.0, None, _ptr(ws), 32) == 1
    assert call(_ptr(t), -1, -inf, inf, 0.0, 0.0, _ptr(sums), _ptr(ws), 32) == 1
    assert call(_ptr(t), t.numel(), -inf, inf, 0.0, 0.0, _ptr(sums), _ptr(ws), 16) == 1                  # short workspace
    assert call(_ptr(t), t.numel(), -inf, inf, 0.0, 0.0, _ptr(sums), C.c_void_p(ws.data_ptr() + 8), 32) == 1      # misaligned workspace
    assert call(_ptr(t), 2 ** 31, -inf, inf, 0.0, 0.0, _ptr(sums), _ptr(ws), 32) == 3                    # UAD_ERR_UNSUPPORTED, nothing launched
    assert eng.lib.uad_clamp_standardize(None, 4, -inf, inf, 0.0, 1.0, _ptr(t), eng._stream()) == 1
    assert eng.lib.uad_clamp_standardize(_ptr(t), 0, -inf, inf, 0.0, 1.0, _ptr(t), eng._stream()) == 0
    torch.cuda.synchronize(eng.device)


@pytest.mark.parametrize('lower,upper', [(None, None), (0, 99.8), (5, 95)])
def test_normalize_standardization_equals_the_host_route(eng, lower, upper):
    vol, _, mask = sc.mslub_phantom()
    v = np.abs(vol) * mask                                     # no negative value: a zero-valued lower clamp has one sign
    got = nifti.normalize_standardization(v, lower, upper, engine=eng)
    want = nifti.normalize_standardization(v, lower, upper)
    assert got.dtype == np.float32 and got.shape == v.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize('axis', ['axial', 'saggital'])
def test_mslub_pipeline_with_and_without_device_stats(eng, axis):
    """device_stats=False normalises with the host statement and resamples on the device; device_stats=True keeps the volume resident from the
    upload on.  Same kept slices as the engine-less route and the same bits between the two (the resampler is the device spline op in both,
    as in the scaling route's own test, tests/test_gpu_select.py)."""
    vol, seg, mask = sc.mslub_phantom()
    vol = np.abs(vol)
    kw = dict(KW, axis=axis)
    host = nifti.volume_to_slices(vol, seg, mask, normalization='standardization', **kw)
    off = nifti.volume_to_slices(vol, seg, mask, engine=eng, device_stats=False, normalization='standardization', **kw)
    on = nifti.volume_to_slices(vol, seg, mask, engine=eng, device_stats=True, normalization='standardization', **kw)
    auto = nifti.volume_to_slices(vol, seg, mask, engine=eng, normalization='standardization', **kw)
    n_ax = vol.shape[nifti.VIEW_MAPPING[axis]]
    assert on[2] == off[2] == auto[2] == host[2] and 0 < len(host[2]) < n_ax
    for got in (on, auto):
        assert got[0].shape == off[0].shape and got[0].tobytes() == off[0].tobytes() and got[1].tobytes() == off[1].tobytes()
    assert on[0].min() < 0.0


def test_brainweb_pipeline_equals_the_host_route(eng):
    vol, tissue = sc.brainweb_phantom()
    host = nifti.volume_to_slices(vol, tissue, loader='brainweb', normalization='standardization', **KW)
    dev = nifti.volume_to_slices(vol, tissue, loader='brainweb', engine=eng, normalization='standardization', **KW)
    assert dev[2] == host[2] and len(host[2]) > 0
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes()


def test_the_default_method_is_unchanged_on_the_device(eng):
    vol, seg, mask = sc.mslub_phantom()
    vol = np.abs(vol)
    v = vol * mask
    assert nifti.normalize_scaling(v, engine=eng).tobytes() == nifti.normalize_scaling(v).tobytes()
    a = nifti.volume_to_slices(vol, seg, mask, engine=eng, **KW)
    b = nifti.volume_to_slices(vol, seg, mask, engine=eng, normalization='scaling', **KW)
    assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].max() <= 1.2 and a[0].min() >= -0.2
