"""CPU: options['exportSamples'] of utils/Evaluation.evaluate (utils/Evaluation.py:302-321, 501-507: the per-slice PNG images of
samples_test_PC/) on the patient-structured stand-in dataset and a host engine, which takes the host-statement path utils/render.py: the
exact file set -- one patient is shorter than sliceEnd --, every file decoded and compared with the statement's array, and nothing at all
without the switch."""
import os

import numpy as np
import torch

from tests.test_evaluation_entry import BlurModel, _opts
from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, png, render
from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import SyntheticPatientDataset

KINDS = ('', '_rec', '_gt', '_diff', '_diff_filtered', '_heatmap', '_vis')


def dataset():
    """two TEST patients at positions 0 and 1 of the walk: 14 slices (indices 2 .. 13) and 12 slices, shorter than sliceEnd = 14 (2 .. 11)"""
    ds = SyntheticPatientDataset(n_val=0, n_test=2, slices=14, native=80, h=64, w=64, seed=6, slice_start=2, slice_end=14)
    name = ds.patients[1]['name']
    ds._vols[name] = tuple(v[:12] for v in ds._vols[name])
    return ds


def expected_images(ds, model, opt):
    """{file name: array} from the statement, over the existing pieces of the evaluation (collect_patient_volume, evaluate_volume, _score_diffs)"""
    want, xs, diffs, segs, where = {}, [], [], [], []
    for p, k in enumerate(ds.get_patient_idx('TEST')):
        patient = ds.patients[k]
        x, seg, skull, prior, idx = Evaluation.collect_patient_volume(ds, patient, patient['filtered_files'][0], opt)
        got = {}
        d, _ = Evaluation.evaluate_volume(model, x, skull, opt, device_out=True, prior=prior, collector=got)
        assert got['reconstructions'].shape == got['residual'].shape == d.shape == x.shape
        assert not torch.equal(got['residual'], d)                                                    # before / after the median
        grey = {'': render.minmax_u8(x.astype(np.float32)), '_rec': render.minmax_u8(got['reconstructions'].numpy()), '_gt': render.label_u8(seg),
                '_diff': render.minmax_u8(got['residual'].numpy()), '_diff_filtered': render.minmax_u8(d.numpy()),
                '_heatmap': render.heatmap_rgba(d.numpy())}
        for j, s in enumerate(idx):
            for kind, a in grey.items():
                want[f'{p}_{s}{kind}.png'] = a[j]
            where.append((p, s))
        xs.append(x); diffs.append(d); segs.append(seg)
    keep = {}
    Evaluation._score_diffs(model, diffs, segs, opt, keep=keep)
    vis = render.overlay_rgb(np.concatenate(xs).astype(np.float32), keep['pred_dev'].numpy(), np.concatenate(segs))
    for (p, s), a in zip(where, vis):
        want[f'{p}_{s}_vis.png'] = a
    return want


def test_export_samples_writes_the_statements_images(tmp_path):
    ds = dataset()
    opt = dict(_opts(tmp_path), exportSamples=True)
    ev = Evaluation.evaluate(ds, BlurModel(tmp_path), opt, epoch='2', description='samples')
    sample_dir = os.path.join(ev['eval_dir'], 'samples_test_PC')
    names = {f'{p}_{s}{kind}.png' for p, idx in ((0, range(2, 14)), (1, range(2, 12))) for s in idx for kind in KINDS}
    assert set(os.listdir(sample_dir)) == names and len(names) == 22 * 7
    want = expected_images(ds, BlurModel(tmp_path), opt)
    assert set(want) == names
    shapes = {'_heatmap': (64, 64, 4), '_vis': (64, 64, 3)}
    seen = set()
    for name, a in want.items():
        got = png.read_png(os.path.join(sample_dir, name))
        kind = name[:-4].split('_', 2)[2] if name.count('_') > 1 else ''
        assert got.shape == shapes.get("_" + kind, (64, 64)) and np.array_equal(got, a), name
        seen.add(got.tobytes())
    assert len(seen) > 22 * 4                                                                         # real pictures, not one image many times
    # lesions are planted: the overlays carry colour somewhere, and the heat maps their colour bar (jet's last entry bottom right)
    assert any((want[n][..., 0] != want[n][..., 1]).any() for n in names if n.endswith('_vis.png'))
    assert all(np.array_equal(want[n][-1, -1], render.jet_u8()[255]) for n in names if n.endswith('_heatmap.png'))


def test_without_the_switch_nothing_is_written_and_the_result_is_unchanged(tmp_path):
    ds = dataset()
    opt = _opts(tmp_path)
    assert 'exportSamples' not in opt
    ev0 = Evaluation.evaluate(ds, BlurModel(tmp_path), opt, epoch='2', description='plain')
    assert os.listdir(os.path.join(ev0['eval_dir'], 'samples_test_PC')) == []
    ev1 = Evaluation.evaluate(ds, BlurModel(tmp_path), dict(opt, exportSamples=True), epoch='2', description='samples')
    assert set(ev0) == set(ev1) and not [k for k in ev0 if k.startswith('_')]
    for k in ev0:
        if k not in ('time', 'eval_dir', 'reconstructionTimes'):
            np.testing.assert_equal(ev0[k], ev1[k], err_msg=k)
    saved = np.load(os.path.join(ev1['eval_dir'], 'evalPC.npy'), allow_pickle=True).item()
    assert set(saved) == set(ev0) - {'eval_dir'}
    # the array-level entry point is untouched by the collector argument's default
    p = ds.patients[ds.get_patient_idx('TEST')[0]]
    x, seg, skull, prior, idx = Evaluation.collect_patient_volume(ds, p, p['filtered_files'][0], opt)
    a = Evaluation.evaluate_volume(BlurModel(tmp_path), x, skull, opt, prior=prior)
    got = {}
    b = Evaluation.evaluate_volume(BlurModel(tmp_path), x, skull, opt, prior=prior, collector=got)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and set(got) == {'reconstructions', 'residual'}
