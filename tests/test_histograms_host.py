"""CPU: the host statement of the evaluation histograms (utils/histograms.py; reference utils/utils.py:44-71 under utils/Evaluation.py:399-411)
against direct numpy calls, the host half of bins='auto' against np.histogram_bin_edges of the installed numpy, the files against
csv.DictWriter / pickle driven as the reference drives them, and options['exportHistograms'] of evaluate() on the host stand-in engine."""
import csv
import os
import pickle

import numpy as np
import pytest

from tests.test_evaluation_entry import BlurModel, _opts
from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, histograms as H
from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import SyntheticPatientDataset

RANGE = (0.01, 0.075)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def data(n, n_classes, dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    v = (rng.random(n) ** 2 * 0.1).astype(np.float32).astype(dtype)
    lab = (rng.integers(0, n_classes, n) * 3 - 2).astype(np.int64)          # class values need not be 0 .. k - 1
    lab[:n_classes] = np.arange(n_classes) * 3 - 2
    return v, lab


@pytest.mark.parametrize('n_classes', [1, 2, 3, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_statement_against_direct_numpy_calls(n_classes, dtype):
    v, lab = data(5000, n_classes, dtype, seed=n_classes)
    classes = np.unique(lab)
    for bins in ('auto', 50):
        got = H.labelled_histograms(v.reshape(50, 100), lab.reshape(50, 100), bins, RANGE)
        assert [r['class'] for r in got] == list(classes) and len(got) == n_classes
        edges = np.histogram_bin_edges(v[lab == classes[0]], bins, RANGE)              # class 0 fixes the edges
        for r, c in zip(got, classes):
            d = v[lab == c]
            assert same(r['bins'], edges)
            assert same(r['n'], np.histogram(d, edges)[0].astype(np.float64))
            assert r['mean'] == np.mean(d.astype(np.float64)) and r['var'] == np.var(d.astype(np.float64))
            assert type(r['mean']) is np.float64 and type(r['var']) is np.float64
    # the moments are over all values of the class, not only those in range
    assert got[0]['n'].sum() < (lab == classes[0]).sum()


def test_more_than_four_classes_raise():
    v, lab = data(100, 5)
    with pytest.raises(ValueError):
        H.labelled_histograms(v, lab, 'auto', RANGE)
    with pytest.raises(ValueError):
        H.class_ids(lab)
    classes, ids = H.class_ids(data(100, 4)[1])
    assert ids.dtype == np.uint8 and np.array_equal(classes[ids], data(100, 4)[1])


def test_class_zero_fixes_the_edges_of_every_class():
    """class 1 is narrow and large: its own 'auto' would take far more bins than class 0's"""
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.random(200) * 0.065 + 0.01, 0.04 + 1e-4 * rng.standard_normal(20000)]).astype(np.float32)
    lab = np.concatenate([np.zeros(200, int), np.ones(20000, int)])
    got = H.labelled_histograms(v, lab, 'auto', RANGE)
    own = np.histogram_bin_edges(v[lab == 1], 'auto', RANGE)
    assert own.size > 4 * got[0]['bins'].size
    assert same(got[1]['bins'], got[0]['bins']) and same(got[0]['bins'], np.histogram_bin_edges(v[lab == 0], 'auto', RANGE))
    assert same(got[1]['n'], np.histogram(v[lab == 1], got[0]['bins'])[0].astype(np.float64))


def auto_cases():
    rng = np.random.default_rng(5)
    lo, hi = np.float32(RANGE[0]), np.float32(RANGE[1])
    rnd = (rng.random(4001) ** 2 * 0.1).astype(np.float32)
    iqr0 = rnd.copy()
    iqr0[rng.random(iqr0.size) < 0.8] = np.float32(0.03125)
    ends = rnd.copy()
    ends[:4] = [lo, hi, np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1))]
    return {'random': rnd, 'iqr0': iqr0, 'all_equal': np.full(300, 0.05, np.float32), 'none_in_range': np.full(300, 0.5, np.float32),
            'one_value': np.array([0.02], np.float32), 'two_values': np.array([0.02, 0.03], np.float32), 'range_ends': ends,
            'small': rnd[:7], 'narrow': (0.04 + 1e-5 * rng.standard_normal(30000)).astype(np.float32)}


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('name', sorted(auto_cases()))
def test_host_half_of_auto_equals_numpy(name, dtype):
    x = auto_cases()[name].astype(dtype)
    for rng_ in (RANGE, (1e-5, 0.0625), (0.05, 0.05)):
        m, vmin, vmax, q25, q75 = H.auto_numbers(x, rng_)
        want = np.histogram_bin_edges(x, 'auto', rng_)
        assert same(H.auto_bin_edges(m, vmin, vmax, q25, q75, rng_, dtype), want), (name, rng_)
        # the float32 bounds select what numpy's own range test selects
        lo32, hi32 = H.range_to_float32(*H.outer_edges(rng_), dtype)
        first, last = H.outer_edges(rng_)
        x32 = x.astype(np.float32)
        assert np.array_equal((x32 >= lo32) & (x32 <= hi32), (x >= first) & (x <= last))
    if name == 'iqr0':
        assert m > 0 and q25 == q75 and want.size > 2                      # fell to Sturges
    if name in ('all_equal', 'none_in_range'):
        assert np.histogram_bin_edges(x, 'auto', RANGE).size == 2           # width 0 / m == 0: one bin


def test_files_are_the_references(tmp_path):
    v, lab = data(3000, 3, np.float64, seed=9)
    res = H.labelled_histograms(v, lab, 'auto', RANGE)
    files = H.write_labelled_histograms(res, str(tmp_path), 'testing_lesions_diffimages_histogram')
    assert sorted(os.path.basename(f) for f in files) == sorted(
        [f'testing_lesions_diffimages_histogram.{i}.npy' for i in range(3)] + [f'testing_lesions_diffimages_histogram.pdf.{i}.csv' for i in range(3)])
    export_pdf = str(tmp_path / 'ref' / 'testing_lesions_diffimages_histogram.pdf')
    os.makedirs(os.path.dirname(export_pdf))
    for i, r in enumerate(res):
        n, bins = r['n'], r['bins']
        with open(export_pdf + ".{}.csv".format(i), mode="w") as csv_file:                    # utils/utils.py:55-60
            fieldnames = ["Bin", "Count"]
            writer = csv.DictWriter(csv_file, fieldnames=fieldnames)
            writer.writeheader()
            for k in range(len(n)):
                writer.writerow({"Bin": bins[k], "Count": n[k]})
        got = open(tmp_path / f'testing_lesions_diffimages_histogram.pdf.{i}.csv', 'rb').read()
        assert got == open(export_pdf + f'.{i}.csv', 'rb').read() and got.startswith(b'Bin,Count\r\n') and got.count(b'\n') == len(n) + 1
        with open(tmp_path / f'testing_lesions_diffimages_histogram.{i}.npy', 'rb') as f:
            back = pickle.load(f)
        assert set(back) == {'n', 'bins', 'mean', 'var'} and same(back['n'], n) and same(back['bins'], bins)
        assert back['mean'] == r['mean'] and back['var'] == r['var']


def test_statement_against_pyplot_hist():
    matplotlib = pytest.importorskip('matplotlib')
    matplotlib.use('Agg')
    from matplotlib import pyplot
    v, lab = data(4000, 3, np.float64, seed=4)
    for bins0 in ('auto', 50):
        res = H.labelled_histograms(v, lab, bins0, RANGE)
        f = pyplot.figure()
        bins = bins0
        for i, c in enumerate(np.unique(lab)):                                                # utils/utils.py:48-50
            n, bins, _ = pyplot.hist(v[lab == c].flatten(), bins=bins, range=RANGE, color=['b', 'r', 'g', 'c'][i])
            assert same(res[i]['n'], n) and same(res[i]['bins'], bins)
        pyplot.close(f)


def _dataset():
    return SyntheticPatientDataset(n_val=0, n_test=2, slices=6, native=40, h=32, w=32, seed=6, slice_start=0, slice_end=6)


HIST_FILES = lambda stem, k: {f'{stem}.{i}.npy' for i in range(k)} | {f'{stem}.pdf.{i}.csv' for i in range(k)}


def test_export_histograms_on_the_host_engine(tmp_path):
    ds = _dataset()
    opt = dict(_opts(tmp_path, h=32), erodeBrainmask=False)
    assert 'exportHistograms' not in opt
    ev0 = Evaluation.evaluate(ds, BlurModel(tmp_path), opt, epoch='2', description='plain')
    assert not [f for f in os.listdir(ev0['eval_dir']) if 'histogram' in f]
    ev1 = Evaluation.evaluate(ds, BlurModel(tmp_path), dict(opt, exportHistograms=True), epoch='2', description='hist')
    names = {f for f in os.listdir(ev1['eval_dir']) if 'histogram' in f}
    assert names == HIST_FILES('testing_lesions_diffimages_histogram', 2)
    # the result and the saved dictionary are those of a run without the switch
    assert set(ev0) == set(ev1)
    for k in ev0:
        if k not in ('time', 'eval_dir', 'reconstructionTimes'):
            np.testing.assert_equal(ev0[k], ev1[k], err_msg=k)
    saved = np.load(os.path.join(ev1['eval_dir'], 'evalPC.npy'), allow_pickle=True).item()
    assert set(saved) == set(ev0) - {'eval_dir'}
    # the files hold the statement of the residuals evaluate() scores
    eval_pc, _ = Evaluation._evaluate(ds, BlurModel(tmp_path), str(tmp_path / 'again'), opt)
    want = H.labelled_histograms(eval_pc['diffs'], eval_pc['labelmaps'], 'auto', Evaluation.HISTOGRAM_RANGE)
    assert len(want) == 2 and want[1]['n'].sum() > 0
    for i, r in enumerate(want):
        with open(os.path.join(ev1['eval_dir'], f'testing_lesions_diffimages_histogram.{i}.npy'), 'rb') as f:
            back = pickle.load(f)
        assert same(back['n'], r['n']) and same(back['bins'], r['bins']) and back['mean'] == r['mean'] and back['var'] == r['var']
        rows = list(csv.DictReader(open(os.path.join(ev1['eval_dir'], f'testing_lesions_diffimages_histogram.pdf.{i}.csv'), newline='')))
        assert [float(x['Bin']) for x in rows] == list(r['bins'][:-1]) and [float(x['Count']) for x in rows] == list(r['n'])


def test_export_histograms_with_monte_carlo_variances(tmp_path):
    class Noisy(BlurModel):
        def reconstruct(self, x, dropout=False, eps=None):
            out = super().reconstruct(x)
            if dropout:
                self.k = getattr(self, 'k', 0) + 1
                out['reconstruction'] = out['reconstruction'] * np.float32(1 + 0.05 * np.sin(self.k))
            return out
    ds = _dataset()
    opt = dict(_opts(tmp_path, h=32), erodeBrainmask=False, exportHistograms=True, numMonteCarloSamples=3)
    ev = Evaluation.evaluate(ds, Noisy(tmp_path), opt, epoch='2', description='mc')
    names = {f for f in os.listdir(ev['eval_dir']) if 'histogram' in f}
    assert names == HIST_FILES('testing_lesions_diffimages_histogram', 2) | HIST_FILES('testing_lesions_epistemic_variances_histogram', 2)
    var = ev['epistemic_variance']
    hi = float(np.percentile(var[var >= 0], 99.8))
    eval_pc, _ = Evaluation._evaluate(ds, Noisy(tmp_path), str(tmp_path / 'again'), opt)
    want = H.labelled_histograms(var, eval_pc['labelmaps'], 50, (1e-5, hi))
    for i, r in enumerate(want):
        with open(os.path.join(ev['eval_dir'], f'testing_lesions_epistemic_variances_histogram.{i}.npy'), 'rb') as f:
            back = pickle.load(f)
        assert same(back['n'], r['n']) and same(back['bins'], r['bins']) and back['n'].size == 50 and back['mean'] == r['mean']
    assert sum(r['n'].sum() for r in want) == sum(ev['uncertaintyHistogram'])
    saved = np.load(os.path.join(ev['eval_dir'], 'evalPC.npy'), allow_pickle=True).item()
    assert not [k for k in saved if 'istogram' in k and k != 'uncertaintyHistogram']
