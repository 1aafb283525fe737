"""GPU: the device order statistics (csrc/uad_select.hip: uad_select_quantiles, uad_histogram_edges, uad_clamp_scale) and their wiring,
held EXACTLY to the installed numpy: np.percentile / np.quantile / np.histogram of the same array, value and dtype (a zero of either
sign is a zero).  Sizes sit on the wave (64), workgroup (256) and tile (UAD_SELECT_TILE) edges, one lies past a full grid of tiles;
inputs cover ties, denormals, signed zeros, infinities away from the brackets, and keys that differ in one byte only.
tests/test_select_host.py checks the host half (the interpolation, the numpy model) without a GPU."""
import types

import numpy as np
import pytest
import torch

from tests import select_cases as sc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, nifti
    from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import SyntheticPatientDataset
    T = _lib.SELECT_TILE
except Exception:
    DeviceOps, T = None, 8192

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1)
BIG = 4198401


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def hold_to_numpy(eng, a, tag):
    qa = np.array([0.0, 0.5, 0.998, 1.0])
    assert same(eng.quantile(a, qa), np.quantile(a, qa)), tag                                  # float64 index, four fractions in one call
    for p in (90, 99.8, 25):                                                                    # float32 index, as numpy forms it for float32 data
        assert same(eng.percentile(a, p), np.percentile(a, p)), (tag, p)
    a64 = a.astype(np.float64)
    assert same(eng.quantile(a64, 0.9), np.quantile(a64, 0.9)), tag                            # float64 data with float32-representable values


@pytest.mark.parametrize('n', SIZES)
def test_select_one_segment(eng, n):
    for kind in sc.GPU_KINDS:
        hold_to_numpy(eng, sc.values(kind, n), (kind, n))
    if n >= 63:                                                     # +-inf: only where no bracket is infinite (numpy's own answer is nan there)
        a = sc.values('inf', n)
        for q in (0.25, 0.5, 0.75):
            want = np.quantile(a, q)
            assert np.isfinite(want) and same(eng.quantile(a, q), want), ('inf', n, q)


@pytest.mark.parametrize('kind', ['random', 'zeros', 'two'])
def test_select_past_one_grid_of_tiles(eng, kind):
    hold_to_numpy(eng, sc.values(kind, BIG), (kind, BIG))


def test_select_takes_a_device_tensor_and_an_unaligned_start(eng):
    a = sc.values('random', 3 * T + 7)
    t = torch.from_numpy(a).to(eng.device)
    for start in (0, 1, 2, 3):                                      # segment starts off the 16-byte grid: the guarded head / tail chunks
        assert same(eng.percentile(t[start:], 90), np.percentile(a[start:], 90)), start
        assert same(eng.quantile(t[start:start + 2 * T], np.array([0.0, 1.0])), np.quantile(a[start:start + 2 * T], np.array([0.0, 1.0]))), start


@pytest.mark.parametrize('per', [257, 4099])
@pytest.mark.parametrize('n_seg', [1, 2, 7, 65])
def test_select_segmented(eng, n_seg, per):
    a = sc.values('random', n_seg * per).reshape(n_seg, per)
    a[n_seg // 2] = sc.values('two', per)                           # a tie-heavy segment among the others
    got = eng.percentile(a, 90, segments=n_seg)
    assert same(got, np.stack([np.percentile(row, 90) for row in a]))                          # every segment on its own
    qa = np.array([0.0, 0.37, 1.0])
    got_q = eng.quantile(a, qa, segments=n_seg)
    assert same(got_q, np.stack([np.quantile(row, qa) for row in a], axis=1))
    # a segment's result does not depend on its neighbours' contents
    s = n_seg - 1
    b = sc.values('distinct', n_seg * per, seed=5).reshape(n_seg, per)
    b[s] = a[s]
    again = eng.percentile(b, 90, segments=n_seg)
    assert again[s].tobytes() == got[s].tobytes()


def test_select_filter(eng):
    base = np.abs(sc.values('random', 2 * T + 1)) + np.float32(0.5)
    none_neg, all_neg = base, -base
    some_neg = base.copy()
    some_neg[::3] *= -1
    some_neg[5] = -0.0                                              # -0 >= 0: it passes the filter, as in numpy
    for a in (none_neg, some_neg):
        pos = a[a >= 0]
        m, lo, hi = eng.select_quantiles(a, [0.998], [True], nonneg_only=True)
        assert int(m[0]) == pos.size
        assert same(eng.percentile(a, 99.8, nonneg_only=True), np.percentile(pos, 99.8))
        assert same(eng.quantile(a, np.array([0.0, 1.0]), nonneg_only=True), np.quantile(pos, np.array([0.0, 1.0])))
    m, lo, hi = eng.select_quantiles(all_neg, [0.998], [True], nonneg_only=True)
    assert int(m[0]) == 0 and np.isnan(lo).all() and np.isnan(hi).all()
    r = eng.percentile(all_neg, 99.8, nonneg_only=True)
    assert r.dtype == np.float32 and np.isnan(r)
    # segment-wise: an empty segment between two populated ones
    three = np.stack([some_neg[:4099], all_neg[:4099], none_neg[:4099]])
    r = eng.percentile(three, 50, segments=3, nonneg_only=True)
    assert np.isnan(r[1]) and same(r[[0, 2]], np.array([np.percentile(three[0][three[0] >= 0], 50), np.percentile(three[2], 50)]))


def test_select_workspace_reuse(eng):
    """Two calls of different size on one workspace, then the first again: bit-identical (the last arrivers leave the counters and tickets
    at zero; whatever else the workspace held does not matter)."""
    ws = eng.select_workspace(7)
    ws.fill_(-1)                                                    # poisoned: the call initialises what it polls
    a = sc.values('random', 7 * 4099).reshape(7, 4099)
    b = sc.values('two', 3 * T + 1)
    qa, f32 = [0.0, 0.9, 0.998, 1.0], [True, False, True, False]
    first = eng.select_quantiles(a, qa, f32, segments=7, workspace=ws)
    other = eng.select_quantiles(b, qa[:2], f32[:2], workspace=ws)
    again = eng.select_quantiles(a, qa, f32, segments=7, workspace=ws)
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    want = sc.model_select(b, qa[:2], f32[:2])
    for x, y in zip(other, want):
        assert same(x, y)
    for x, y in zip(first, sc.model_select(a, qa, f32, segments=7)):
        assert same(x, y)


def _histogram_vector(n_max, bins, seed):
    """Specials first (on every edge, one ulp to either side of it, on the last edge, outside the range), then a skewed random tail."""
    rng = np.random.default_rng(seed)
    tail = rng.random(n_max).astype(np.float32) ** 3 * np.float32(0.02)
    hi = float(np.percentile(tail[tail >= 0], 99.8))
    e = np.histogram_bin_edges(tail, bins=bins, range=(1e-5, hi))
    assert e.dtype == np.float32
    specials = np.concatenate([[e[-1], e[0], np.float32(-1.0), np.float32(1.0), np.float32(0.0)], np.nextafter(e, np.float32(np.inf)),
                               np.nextafter(e, np.float32(-np.inf)), e]).astype(np.float32)
    return np.concatenate([specials, tail])[:max(n_max, specials.size)], hi


@pytest.mark.parametrize('bins', [50, 7])
def test_histogram(eng, bins):
    v, hi = _histogram_vector(2 * T + 1, bins, bins)
    for n in SIZES + (v.size,):
        a = v[:n]
        counts, edges = eng.histogram(a, bins, (1e-5, hi))
        want, want_edges = np.histogram(a, bins=bins, range=(1e-5, hi))
        assert same(edges, want_edges) and same(counts, want), (bins, n)
    t = torch.from_numpy(v).to(eng.device)
    for start in (1, 2, 3):                                         # off the 16-byte grid
        assert same(eng.histogram(t[start:], bins, (1e-5, hi))[0], np.histogram(v[start:], bins=bins, range=(1e-5, hi))[0]), start
    a64 = v.astype(np.float64)                                      # float64 data: float64 edges, folded onto float32 ones that bin alike
    assert same(eng.histogram(a64, bins, (1e-5, hi))[0], np.histogram(a64, bins=bins, range=(1e-5, hi))[0])
    assert same(eng.histogram(v, bins)[0], np.histogram(v, bins=bins)[0])                      # range=None


def test_clamp_scale(eng):
    a = sc.values('random', 2 * T + 3)
    a[:4] = [-0.0, 0.0, -3.0, 3.0]
    t = torch.from_numpy(a).to(eng.device)
    lo, hi, s = np.float32(-0.5), np.float32(0.75), np.float32(1.0) / np.float32(0.75)
    for start in (0, 1):                                            # the 16-byte path and the scalar path
        want = a[start:].copy()
        want[want < lo] = lo
        want[want > hi] = hi
        want = want * s
        assert eng.clamp_scale(t[start:], lo, hi, s).cpu().numpy().tobytes() == want.tobytes(), start
    assert eng.clamp_scale(t, None, None, 1.0).cpu().numpy().tobytes() == a.tobytes()


# ------------------------------------------------------------------------------------------------------------------------ ingestion / evaluation
def test_normalize_scaling_on_the_device_is_bit_equal(eng):
    """(0, 99.8), the pipeline's setting: bit-equal.  A lower percentile that lands on a zero while the volume holds negative values (the
    phantom's noisy rim does) CLAMPS those to the percentile itself, and the sign of that zero is not defined: numpy's comes out of its
    partition order and _lerp (-0 + 0 * t = +0, -0 - 0 * (1 - t) = -0), the op returns +0 for either -- the op's contract, as numpy's own
    comparisons, knows one zero.  There every value must be equal and every non-zero bit-equal."""
    vol, _, mask = sc.phantom()
    v = vol * (mask >= 0.1)
    assert nifti.normalize_scaling(v, 0, 99.8, engine=eng).tobytes() == nifti.normalize_scaling(v, 0, 99.8).tobytes()
    got, want = nifti.normalize_scaling(v, 5, 90, engine=eng), nifti.normalize_scaling(v, 5, 90)
    assert np.percentile(v.astype(np.float32), 5) == 0 and (v < 0).any()
    assert same(got, want)
    nz = want != 0
    assert got[nz].tobytes() == want[nz].tobytes()


@pytest.mark.parametrize('axis', ['axial', 'saggital'])
def test_volume_to_slices_device_stats(eng, axis):
    vol, seg, mask = sc.phantom((12, 37, 29))
    kw = dict(axis=axis, slice_start=0, slice_end=40, slice_resolution=(32, 32))
    on = nifti.volume_to_slices(vol, seg, mask, engine=eng, device_stats=True, **kw)
    off = nifti.volume_to_slices(vol, seg, mask, engine=eng, device_stats=False, **kw)
    n_ax = vol.shape[nifti.VIEW_MAPPING[axis]]
    assert 2 <= len(off[2]) <= n_ax - 2, 'the phantom must have slices on either side of the 0.2 filter'
    assert on[2] == off[2]
    assert on[0].shape == off[0].shape and on[0].tobytes() == off[0].tobytes()
    assert on[1].tobytes() == off[1].tobytes()
    host = nifti.volume_to_slices(vol, seg, mask, **kw)             # and the kept slices are the host path's
    assert host[2] == on[2]


class _Float32Volumes:
    """SyntheticPatientDataset whose image volumes hold float32 numbers (as a float32 NIfTI gives), so the prior quantile runs on the device."""

    def __init__(self, ds):
        self._ds = ds

    def __getattr__(self, k):
        return getattr(self._ds, k)

    def load_volume_and_groundtruth(self, nii_filename, patient):
        x, lab, msk = self._ds.load_volume_and_groundtruth(nii_filename, patient)
        x.data = x.data.astype(np.float32).astype(np.float64)
        return x, lab, msk


def test_collect_patient_volume_prior_quantile(eng, tmp_path):
    ds = _Float32Volumes(SyntheticPatientDataset(n_val=1, n_test=1, slices=14, native=80, h=64, w=64, seed=3, slice_start=2, slice_end=12))
    calls = []
    spy = types.SimpleNamespace(zoom=eng.zoom, quantile=lambda a, q: calls.append(q) or eng.quantile(a, q))
    for k in ds.get_patient_idx('TEST'):
        p = ds.patients[k]
        data = ds.load_volume_and_groundtruth(p['filtered_files'][0], p)[0].data
        got = Evaluation.collect_patient_volume(ds, p, p['filtered_files'][0], {}, engine=spy)
        assert got[3] == float(np.quantile(data, 0.9))
        assert same(Evaluation._prior_quantile(data, eng), np.quantile(data, 0.9))
    assert calls == [0.9]


def test_monte_carlo_tail_uncertainty_histogram(eng):
    rng = np.random.default_rng(11)
    shape = (6, 16, 16)
    lab = np.zeros(shape, np.int64)
    lab[2:4, 4:9, 4:9] = 1
    d = (rng.random(shape) * 0.3 + 0.6 * lab * rng.random(shape)).astype(np.float32)
    var = (rng.random(shape).astype(np.float32) ** 4 * np.float32(3e-3)).astype(np.float32)
    var[0, 0, :4] = [0.0, 1e-5, -0.0, 2e-3]
    ev = Evaluation._score_diffs(types.SimpleNamespace(engine=eng), [torch.from_numpy(d).to(eng.device)], [lab], {}, [var])
    pos = var[var >= 0]
    hi = float(np.percentile(pos, 99.8))
    assert ev['uncertaintyHistogram'] == np.histogram(var, bins=50, range=(1e-5, hi))[0].tolist()
    assert ev['epistemic_variance'] is not None and same(ev['epistemic_variance'], var)
