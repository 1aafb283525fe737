"""GPU: the per-class histogram ops (csrc/uad_select.hip: uad_select_quantiles_masked; csrc/uad_hist.hip: uad_histogram_by_class) and
their wiring (engine.labelled_histogram, options['exportHistograms'] of evaluate()), held to the host statement utils/histograms.py, which
is plain numpy: counts, m, the select's brackets and the edges EXACTLY; mean and variance to the exactly rounded values (math.fsum over
the fp64 values and over (v - mean)^2) at 1e-12 relative to sum |terms| / count -- the project's bar for fp64 reductions, which any
fixed-order sum whose longest chain of dependent additions is at most 8192 holds by construction (8192 * 2^-53 = 9.1e-13); the chain the
header states is asserted to be that short.  Sizes sit on the wave (64) and tile (UAD_SELECT_TILE) edges, bin counts on either side of the
chunk edge (UAD_HISTOGRAM_MAX_BINS).  tests/test_histograms_kernels_host.py runs the same cases on the kernel source compiled for the host."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import hist_cases as hc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, histograms as H
    from unsupervised_anomaly_detection_brain_mri_amd.utils.order_stats import edges_to_float32
except Exception:
    DeviceOps = None

KIND_BINS = tuple(zip(hc.KINDS, (1024, 1025, 2, 1, 50, 2049)))       # every bin count of hc.BINS; the values on the edges meet the chunk edge
assert sorted(b for _, b in KIND_BINS) == sorted(hc.BINS)


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def two_pass(eng, v, lab, k, e32, ws=None):
    """the two launches of labelled_histogram through the raw op -> host arrays (counts, class_count, mean, var)"""
    _, cnt, sums = eng.histogram_by_class(v, lab, k, workspace=ws)
    mean = sums / cnt.to(torch.float64)
    counts, cnt2, sq = eng.histogram_by_class(v, lab, k, edges32=e32, centre=mean, workspace=ws)
    assert torch.equal(cnt, cnt2)
    return counts.cpu().numpy(), cnt.cpu().numpy(), mean.cpu().numpy(), (sq / cnt.to(torch.float64)).cpu().numpy()


def moments_checked(v, lab, k, cnt, mean, var, tag):
    for c, exact in enumerate(hc.exact_moments(v, lab, k)):
        d = v[lab == c].astype(np.float64)
        print(tag, 'class', c, 'count', cnt[c], 'mean', repr(mean[c]), 'var', repr(var[c]), 'exact', exact)
        if exact is not None:
            assert hc.moments_hold(cnt[c], mean[c], var[c], exact), (tag, c, mean[c], var[c], exact)
        elif d.size:                                                   # an infinity in the class: numpy's inf / nan
            with np.errstate(invalid='ignore'):
                assert cnt[c] == d.size and np.array_equal(mean[c], np.mean(d), equal_nan=True) and np.isnan(var[c]), (tag, c)
        else:
            assert cnt[c] == 0


@pytest.mark.parametrize('n', hc.SIZES)
def test_counts_and_moments_per_class(eng, n):
    for k in hc.CLASSES:
        lab = hc.ids(n, k, extra=True)                                 # ids at or above k are dropped
        for kind, bins in KIND_BINS:
            v = hc.values(kind, n, lab, bins)
            e32 = edges_to_float32(hc.edge_table(bins))
            counts, cnt, mean, var = two_pass(eng, v, lab, k, e32)
            assert same(counts, hc.reference_counts(v, lab, k, e32)), (k, kind, bins)
            moments_checked(v, lab, k, cnt, mean, var, (n, k, kind))


@pytest.mark.parametrize('n', hc.SIZES)
def test_masked_select_and_auto_edges(eng, n):
    first, last = H.outer_edges(hc.RANGE)
    for k in hc.CLASSES:
        lab = hc.ids(n, k)
        for kind in hc.KINDS:
            v = hc.values(kind, n, lab)
            for dtype in (np.float32, np.float64):
                x = v.astype(dtype)
                lo32, hi32 = H.range_to_float32(first, last, dtype)
                m, lo, hi = eng.select_quantiles_masked(v, lab, 0, lo32, hi32, H.AUTO_Q, [False] * 4)
                x0 = x[lab == 0]
                s = np.sort(x0[(x0 >= first) & (x0 <= last)]).astype(np.float32)
                assert m == s.size, (k, kind, dtype)
                if m == 0:
                    assert np.isnan(lo).all() and np.isnan(hi).all()
                else:
                    idx = [(m - 1) * q for q in H.AUTO_Q]
                    assert same(lo, s[[int(np.floor(i)) for i in idx]]) and same(hi, s[[min(int(np.floor(i)) + 1, m - 1) for i in idx]]), (k, kind, dtype)
                got = H.auto_bin_edges(m, lo[0], hi[3], (lo[1], hi[1]), (lo[2], hi[2]), hc.RANGE, dtype)
                assert same(got, np.histogram_bin_edges(x0, 'auto', hc.RANGE)), (k, kind, dtype)
    if n > 2:                                                          # another class than 0, off the 16-byte grid
        t = torch.from_numpy(v).to(eng.device)
        m, lo, hi = eng.select_quantiles_masked(t[1:], lab[1:], k - 1, np.float32(0.0), np.float32(1.0), [0.5], [False])
        s = np.sort(v[1:][(lab[1:] == k - 1) & (v[1:] >= 0) & (v[1:] <= 1)])
        assert m == s.size and (m == 0 or (lo[0] == s[(m - 1) // 2] and hi[0] == s[min((m - 1) // 2 + 1, m - 1)]))


@pytest.mark.parametrize('n', hc.SIZES)
def test_labelled_histogram_is_the_statement(eng, n):
    for k in hc.CLASSES:
        ids = hc.ids(n, k)
        labels = ids.astype(np.int64) * 3 - 2                          # class values need not be 0 .. k - 1
        for kind in hc.KINDS:
            v = hc.values(kind, n, ids)
            for values, ref_values, bins in ((torch.from_numpy(v).to(eng.device), v, 'auto'), (v.astype(np.float64), v.astype(np.float64), 'auto'),
                                             (v, v, 50), (torch.from_numpy(v).to(eng.device), v, hc.edge_table(7, dtype=np.float64))):
                got = eng.labelled_histogram(values, labels, bins, hc.RANGE)
                with np.errstate(invalid='ignore'):                    # numpy's own mean / var of a class that holds an infinity
                    want = H.labelled_histograms(ref_values, labels, bins, hc.RANGE)
                assert len(got) == len(want) == np.unique(labels).size
                for g, w in zip(got, want):
                    assert g['class'] == w['class'] and same(g['bins'], w['bins']) and same(g['n'], w['n']), (k, kind, str(bins)[:8])
                    assert type(g['mean']) is np.float64 and type(g['var']) is np.float64
                present = [int(c) for c in np.unique(ids)]
                exact = hc.exact_moments(v, ids, k)
                for g, c in zip(got, present):
                    if exact[c] is not None:
                        assert hc.moments_hold(exact[c][0], g['mean'], g['var'], exact[c]), (k, kind, c, g['mean'], g['var'], exact[c])


def test_nothing_to_do(eng):
    assert eng.labelled_histogram(np.zeros(0, np.float32), np.zeros(0, np.int64), 'auto', hc.RANGE) == []
    lib, st = eng.lib, eng._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    counts = torch.full((2, 5), -1, dtype=torch.int64, device=eng.device)
    cnt = torch.full((2,), -1, dtype=torch.int64, device=eng.device)
    sums = torch.full((2,), np.nan, dtype=torch.float64, device=eng.device)
    edges = torch.linspace(0, 1, 6, device=eng.device)
    assert lib.uad_histogram_by_class(None, None, 0, 2, p(edges), 5, None, p(counts), p(cnt), p(sums), None, 0, st) == _lib.UAD_OK
    torch.cuda.synchronize()
    assert not counts.any() and not cnt.any() and not sums.any()
    assert lib.uad_histogram_by_class_workspace(0) == 0 and lib.uad_histogram_by_class_workspace(hc.T - 3) == 64 and lib.uad_histogram_by_class_workspace(hc.T - 2) == 128


def test_bits_do_not_change_from_run_to_run(eng):
    n, k = 3 * hc.T + 17, 4
    lab = hc.ids(n, k)
    v = hc.values('random', n, lab)
    e32 = edges_to_float32(hc.edge_table(1025))
    ws = eng.histogram_workspace(n)
    ws.fill_(-1)                                                       # poisoned: as int64 pairs all ones, as fp64 a NaN
    first = two_pass(eng, v, lab, k, e32, ws=ws)
    again = two_pass(eng, v, lab, k, e32, ws=ws)                       # the workspace as the first call left it
    other = torch.rand(1 << 20, device=eng.device)                     # an unrelated tensor allocated: other addresses for the temporaries
    smaller = two_pass(eng, v[:hc.T + 5], lab[:hc.T + 5], k, e32, ws=ws)
    third = two_pass(eng, v, lab, k, e32)
    for a, b, c in zip(first, again, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert same(smaller[0], hc.reference_counts(v[:hc.T + 5], lab[:hc.T + 5], k, e32))
    a = eng.labelled_histogram(v, lab, 'auto', hc.RANGE)
    b = eng.labelled_histogram(v, lab, 'auto', hc.RANGE)
    assert pickle.dumps(a) == pickle.dumps(b) and other.numel()


def test_chain_length_refusals_and_the_abi(eng):
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'uad_hip.h')).read()
    chain = int(re.search(r'UAD_HISTOGRAM_SUM_CHAIN\s*=\s*(\d+)', header).group(1))
    assert chain == _lib.HISTOGRAM_SUM_CHAIN and chain <= hc.CHAIN_MAX
    lib, st = eng.lib, eng._stream()
    for name in ('uad_select_quantiles_masked', 'uad_histogram_by_class', 'uad_histogram_by_class_workspace'):
        assert name in _lib.SYMBOLS and name + '(' in header and hasattr(lib, name)
    p = lambda t: C.c_void_p(t.data_ptr())
    n, k, bins = 100, 2, 5
    v = torch.rand(n, device=eng.device)
    lab = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    edges = torch.linspace(0, 1, bins + 1, device=eng.device)
    counts = torch.zeros((k, bins), dtype=torch.int64, device=eng.device)
    cnt = torch.zeros(k, dtype=torch.int64, device=eng.device)
    sums = torch.zeros(k, dtype=torch.float64, device=eng.device)
    ws = eng.histogram_workspace(n)
    ok = (p(v), p(lab), n, k, p(edges), bins, None, p(counts), p(cnt), p(sums), p(ws), ws.numel() * 8, st)
    assert lib.uad_histogram_by_class(*ok) == _lib.UAD_OK
    for pos, val in ((0, None), (1, None), (2, -1), (3, 0), (3, 5), (4, None), (5, -1), (5, _lib.HISTOGRAM_MAX_BINS + 1), (7, None), (8, None), (9, None),
                     (10, None), (11, 8), (10, C.c_void_p(ws.data_ptr() + 8))):
        args = list(ok)
        args[pos] = val
        assert lib.uad_histogram_by_class(*args) == 1, (pos, val)
    assert b'histogram_by_class' in lib.uad_last_error()
    args = list(ok)
    args[2] = 1 << 31
    assert lib.uad_histogram_by_class(*args) == 3                      # unsupported, nothing launched
    m = torch.zeros(1, dtype=torch.int64, device=eng.device)
    br = torch.zeros(8, dtype=torch.float32, device=eng.device)
    sws = eng.select_workspace(1)
    q = (C.c_double * 4)(*H.AUTO_Q)
    oks = (p(v), p(lab), n, 0, 0.0, 1.0, q, 4, 0, p(m), p(br), p(sws), sws.numel() * 8, st)
    assert lib.uad_select_quantiles_masked(*oks) == _lib.UAD_OK
    for pos, val in ((0, None), (1, None), (2, 0), (3, -1), (3, 256), (4, 2.0), (4, float('nan')), (7, 0), (7, 5), (9, None), (10, None), (11, None), (12, 8)):
        args = list(oks)
        args[pos] = val
        assert lib.uad_select_quantiles_masked(*args) == 1, (pos, val)
    torch.cuda.synchronize()
    assert int(m[0]) == n
    with pytest.raises(ValueError):
        eng.labelled_histogram(np.array([0.1], np.float64), np.zeros(1), 'auto', hc.RANGE)          # not a float32 number
    with pytest.raises(ValueError):
        eng.labelled_histogram(np.zeros(10, np.float32), np.arange(10), 'auto', hc.RANGE)          # more than four classes
    with pytest.raises(ValueError):
        eng.labelled_histogram(np.zeros(10, np.float32), np.zeros(9), 'auto', hc.RANGE)


def test_long_tables(eng, capsys):
    """a small inter-quartile range: 'auto' asks for thousands of bins (counted in chunks) -- and, narrower still, for more than
    MAX_DEVICE_BINS, which evaluate()'s helper hands to the host statement with one line on stderr"""
    rng = np.random.default_rng(8)
    lab = (rng.random(30000) < 0.05).astype(np.int64)
    v = (0.04 + 7.5e-5 * rng.standard_normal(30000)).astype(np.float32)
    got, want = eng.labelled_histogram(v, lab, 'auto', hc.RANGE), H.labelled_histograms(v, lab, 'auto', hc.RANGE)
    assert 4 * _lib.HISTOGRAM_MAX_BINS < want[0]['n'].size <= H.MAX_DEVICE_BINS
    for g, w in zip(got, want):
        assert same(g['bins'], w['bins']) and same(g['n'], w['n'])
    v = (0.04 + 7.5e-6 * rng.standard_normal(30000)).astype(np.float32)
    with pytest.raises(H.TooManyBins):
        eng.labelled_histogram(v, lab, 'auto', hc.RANGE)
    Evaluation._told_host_histogram = False
    want = H.labelled_histograms(v, lab, 'auto', hc.RANGE)
    for _ in range(2):
        got = Evaluation._labelled_histograms(eng, v, v, lab, 'auto', hc.RANGE)
        assert all(same(g['n'], w['n']) and same(g['bins'], w['bins']) for g, w in zip(got, want)) and want[0]['n'].size > H.MAX_DEVICE_BINS
    assert capsys.readouterr().err.count('computed on the host') == 1


def test_export_histograms_on_the_engine_writes_the_files_of_the_host_path(eng, tmp_path):
    """evaluate() with exportHistograms for two small patients (6 slices of 32 x 32) and three Monte-Carlo passes: the real engine computes
    the histograms on the device, the same engine with labelled_histogram hidden takes the host statement on the downloaded residuals.
    The .csv files are byte-identical, the pickles hold the same counts and edges and moments that meet the bar; without the key no
    histogram file appears."""
    from tests.test_evaluation_entry import BlurModel, _opts
    from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import SyntheticPatientDataset

    class Hidden:
        """the engine without labelled_histogram"""
        def __init__(self, e):
            self._e = e

        def __getattr__(self, k):
            if k == 'labelled_histogram':
                raise AttributeError(k)
            return getattr(self._e, k)

    class Recording:
        """the engine, remembering what labelled_histogram was given"""
        def __init__(self, e):
            self._e, self.seen = e, []

        def __getattr__(self, k):
            return getattr(self._e, k)

        def labelled_histogram(self, values, labels, bins, range, **kw):
            self.seen.append((values.cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values), np.asarray(labels)))
            return self._e.labelled_histogram(values, labels, bins, range, **kw)

    class Noisy(BlurModel):
        def reconstruct(self, x, dropout=False, eps=None):
            out = super().reconstruct(x)
            if dropout:
                self.k = getattr(self, 'k', 0) + 1
                out['reconstruction'] = out['reconstruction'] * np.float32(1 + 0.05 * np.sin(self.k))
            return out

    ds = SyntheticPatientDataset(n_val=0, n_test=2, slices=6, native=40, h=32, w=32, seed=6, slice_start=0, slice_end=6)
    dirs, evs = [], []
    recording = Recording(eng)
    for engine, tag in ((recording, 'device'), (Hidden(eng), 'host')):
        model = Noisy(tmp_path, bs=4)
        model.engine = engine
        opt = dict(_opts(tmp_path, h=32), exportHistograms=True, erodeBrainmask=False, numMonteCarloSamples=3)
        evs.append(Evaluation.evaluate(ds, model, opt, epoch='1', description=tag))
        dirs.append(evs[-1]['eval_dir'])
    names = sorted(f for f in os.listdir(dirs[0]) if 'histogram' in f)
    stems = ('testing_lesions_diffimages_histogram', 'testing_lesions_epistemic_variances_histogram')
    assert names == sorted(f for f in os.listdir(dirs[1]) if 'histogram' in f)
    assert names == sorted([f'{s}.{i}.npy' for s in stems for i in range(2)] + [f'{s}.pdf.{i}.csv' for s in stems for i in range(2)])
    # the values the histograms are of: the residuals evaluate() scored, and the variances it returned
    assert len(recording.seen) == 2 and recording.seen[0][0].dtype == recording.seen[1][0].dtype == np.float32
    assert np.array_equal(recording.seen[1][0], evs[0]['epistemic_variance']) and np.array_equal(evs[0]['epistemic_variance'], evs[1]['epistemic_variance'])
    exact = {stem: hc.exact_moments(v.reshape(-1), H.class_ids(lab)[1], 2) for stem, (v, lab) in zip(stems, recording.seen)}
    for name in names:
        a, b = (open(os.path.join(d, name), 'rb').read() for d in dirs)
        if name.endswith('.csv'):
            assert a == b and a.count(b'\n') > 1, name
        else:
            ga, gb = pickle.loads(a), pickle.loads(b)
            assert same(ga['n'], gb['n']) and same(ga['bins'], gb['bins']) and ga['n'].sum() > 0, name
            stem, i = name.rsplit('.', 2)[0], int(name.rsplit('.', 2)[1])
            print(name, repr(ga['mean']), repr(gb['mean']), repr(ga['var']), repr(gb['var']), exact[stem][i])
            assert hc.moments_hold(exact[stem][i][0], ga['mean'], ga['var'], exact[stem][i]), name
    model = Noisy(tmp_path, bs=4)
    model.engine = eng
    ev = Evaluation.evaluate(ds, model, dict(_opts(tmp_path, h=32), erodeBrainmask=False), epoch='1', description='plain')
    assert not [f for f in os.listdir(ev['eval_dir']) if 'histogram' in f]
