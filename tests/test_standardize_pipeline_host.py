"""CPU: normalization='standardization' through the volume -> slice pipeline without an engine (utils/nifti.py: volume_to_slices for both
loaders, build_cache), against the steps spelled out by hand with numpy and scipy; the default method's output stays byte for byte what
normalization='scaling' gives; the two new entry points are declared, bound and exported."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage

from tests import standardize_cases as sc
from unsupervised_anomaly_detection_brain_mri_amd import _lib
from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti, resize
from unsupervised_anomaly_detection_brain_mri_amd.utils.standardize import standardize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(slice_start=0, slice_end=155, slice_resolution=(32, 32))


def same(a, b):
    return a[2] == b[2] and a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_mslub_against_the_steps_by_hand():
    vol, seg, mask = sc.mslub_phantom()
    got = nifti.volume_to_slices(vol, seg, mask, normalization='standardization', **KW)
    v = standardize(np.array(vol, np.float64) * (mask >= 0.1), 0, 99.8)                 # skull stripping, then NII.normalize('standardization', 0, 99.8)
    lab = (seg >= 0.9).astype(np.float64)
    images, labels, kept = [], [], []
    for s in range(vol.shape[0]):
        sd, ss = v[s], lab[s]
        if np.percentile(sd, 90) < 0.2:                                                 # MSLUB.py:161, whatever the method
            continue
        f = 32.0 / sd.shape[0]                                                          # 40 x 36 needs no padding
        images.append(scipy.ndimage.zoom(sd, f).astype(np.float32))
        labels.append((scipy.ndimage.zoom(ss, f, mode='nearest') >= 0.9).astype(np.float32))
        kept.append(s)
    assert 0 < len(kept) < vol.shape[0] and same(got, (np.stack(images), np.stack(labels), kept))
    assert got[0].min() < 0.0 and got[0].max() > 1.0                                    # not in [0, 1] any more
    assert (got[1] > 0).any()


def test_brainweb_against_the_steps_by_hand():
    vol, tissue = sc.brainweb_phantom()
    got = nifti.volume_to_slices(vol, tissue, loader='brainweb', normalization='standardization', **KW)
    v = standardize(np.where(np.isin(tissue, (0, 4, 5, 6, 7, 9)), 0.0, vol), 0, 99.8)
    lesion = (tissue == 10).astype(np.float32)
    images, labels, kept = [], [], []
    for s in range(vol.shape[0]):
        if np.unique(v[s]).size == 1:                                                   # BRAINWEB.py:133
            continue
        images.append(resize.resize_linear(v[s], (32, 32)))
        labels.append(resize.resize_nearest(lesion[s], (32, 32)))
        kept.append(s)
    assert vol.shape[0] - 1 not in kept and len(kept) > 0                               # the constant last slice is dropped
    assert same(got, (np.stack(images).astype(np.float32), np.stack(labels).astype(np.float32), kept))


@pytest.mark.parametrize('loader', ['mslub', 'brainweb'])
def test_the_default_is_scaling_byte_for_byte(loader):
    if loader == 'mslub':
        vol, seg, mask = sc.mslub_phantom()
        args, kw = (vol, seg, mask), dict(KW, rotations=(0, 10))
    else:
        args, kw = sc.brainweb_phantom(), dict(KW, loader='brainweb')
    today = nifti.volume_to_slices(*args, normalization='scaling', **kw)
    assert same(nifti.volume_to_slices(*args, **kw), today) and len(today[2]) > 0
    assert today[0].min() >= -0.2 and today[0].max() <= 1.2                             # (spline overshoot aside) scaled into [0, 1]
    other = nifti.volume_to_slices(*args, normalization='standardization', **kw)
    assert other[0].shape[1:] == today[0].shape[1:] and not same(other, today)


def test_normalize_scaling_is_what_it_was():
    """The clamp bounds moved into a helper the two methods share: the stand-in engine still sees one select and one clamp-and-scale call."""
    from tests.select_cases import ModelEngine
    vol, _, mask = sc.mslub_phantom()
    v = vol * mask
    eng = ModelEngine()
    assert nifti.normalize_scaling(v, engine=eng).tobytes() == nifti.normalize_scaling(v).tobytes()
    assert [c[0] for c in eng.calls] == ['select', 'clamp_scale']
    # the stand-in has no ordered sums: standardization takes the host statement with it
    assert nifti.normalize_standardization(v, engine=eng).tobytes() == standardize(v, 0, 99.8).tobytes()
    got = nifti.volume_to_slices(vol, None, mask, engine=eng, normalization='standardization', **KW)
    assert same(got, nifti.volume_to_slices(vol, None, mask, normalization='standardization', **KW))
    with pytest.raises(ValueError, match='ordered sums'):
        nifti.volume_to_slices(vol, None, mask, engine=eng, device_stats=True, normalization='standardization', **KW)


def test_an_unknown_method_raises():
    vol, seg, mask = sc.mslub_phantom()
    for kw in (dict(), dict(loader='brainweb')):
        with pytest.raises(ValueError, match='normalization'):
            nifti.volume_to_slices(vol, seg, None if kw else mask, normalization='minmax', **KW, **kw)


def write_patients(root, layout):
    """Two phantom patients as NIfTI files; layout(name, kind) -> file name under the patient's directory."""
    patients = []
    for i in range(2):
        vol, seg, mask = sc.phantom((12, 40, 36), seed=50 + i)
        d = root / f'p{i}'
        d.mkdir(parents=True)
        paths = {}
        for kind, a in (('volume', vol), ('groundtruth', seg), ('skullmap', mask)):
            paths[kind] = str(d / layout(f'p{i}', kind))
            nifti.write_nifti(paths[kind], a)
        patients.append({'name': f'p{i}', **paths})
    return patients


def test_build_cache_passes_the_method_through(tmp_path):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    patients = write_patients(tmp_path / 'data', lambda name, kind: kind + '.nii.gz')
    nifti.build_cache(str(tmp_path / 'std'), patients, partition={'TRAIN': 0.5, 'VAL': 0.5}, seed=0, normalization='standardization', **KW)
    images, labels, index = read_cache(str(tmp_path / 'std'))
    assert index['options']['normalization'] == 'standardization'
    order = [int(n[1:]) for n in dict.fromkeys(index['patients'])]
    want = [nifti.volume_to_slices(*(nifti.read_nifti(p[k])[0] for k in ('volume', 'groundtruth', 'skullmap')), normalization='standardization', **KW)
            for p in patients]
    w = np.concatenate([want[i][0] for i in order])
    assert np.array_equal(images[..., 0], w) and w.min() < 0.0
    # the label rule is the one of every cache: 10 = lesion, 2 = image > 0, else 0 (with standardization "> 0" is "above the volume's mean")
    lw = np.concatenate([want[i][1] for i in order])
    assert np.array_equal(labels, np.where(lw > 0, 10, np.where(w > 0, 2, 0)))
    assert (labels == 10).any() and (labels == 2).any() and (labels == 0).any()
    # the default records nothing new
    nifti.build_cache(str(tmp_path / 'scl'), patients, partition={'TRAIN': 0.5, 'VAL': 0.5}, seed=0, **KW)
    assert 'normalization' not in read_cache(str(tmp_path / 'scl'))[2]['options']
    with pytest.raises(ValueError, match='normalization'):
        nifti.build_cache(str(tmp_path / 'bad'), patients, partition={'TRAIN': 1.0}, normalization='zscore', **KW)


def test_padding_and_rotation_corners_stay_background_in_the_cache(tmp_path):
    """Zero padding and the corners a rotation fills are literal zeros whatever the method (the reference pads after normalising): the
    cache's label map must not call them brain."""
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    vol, tissue = sc.brainweb_phantom()
    d = tmp_path / 'p0'
    d.mkdir()
    nifti.write_nifti(str(d / 't1.nii.gz'), vol)
    nifti.write_nifti(str(d / 'classes.nii.gz'), tissue, dtype='u1')
    patients = [{'name': 'p0', 'volume': str(d / 't1.nii.gz'), 'groundtruth': str(d / 'classes.nii.gz')}]
    kw = dict(loader='brainweb', slice_start=0, slice_end=155, slice_resolution=(48, 48), rotations=(0, 20), normalization='standardization')
    nifti.build_cache(str(tmp_path / 'c'), patients, partition={'TRAIN': 1.0}, seed=0, **kw)
    images, labels, index = read_cache(str(tmp_path / 'c'))
    assert images.shape[1:3] == (48, 48) and images.shape[0] % 2 == 0 and index['options']['rotations'] == [0, 20]
    y0, x0 = (48 - 40) // 2, (48 - 36) // 2
    frame = np.ones((48, 48), bool)
    frame[y0:y0 + 40, x0:x0 + 36] = False
    plain, rotated = np.asarray(images[0::2, ..., 0]), np.asarray(images[1::2, ..., 0])
    assert (plain[:, frame] == 0).all() and (np.asarray(labels[0::2])[:, frame] == 0).all()          # the padding frame
    assert (plain[:, ~frame] < 0).any()                                                                # a standardized background inside it
    # filled by the rotation: never brain.  (The LESION class of a rotated slice is `spline-rotated label map > 0` whatever the method, and
    # the cubic spline rings at 1e-12 far from the lesion: a corner may carry 10 in a 'scaling' cache just as well.)
    for corner in ((0, 0), (0, 47), (47, 0), (47, 47)):
        assert (rotated[(slice(None),) + corner] == 0).all() and (np.asarray(labels[1::2])[(slice(None),) + corner] != 2).all()
    assert (labels == 2).any() and (labels == 10).any()


def test_brainweb_with_an_engine_without_the_sums_takes_the_host_route():
    """A stand-in engine with `resize` but no ordered sums: the normalisation falls back to the host statement, as the MS loaders' path does."""
    from tests.select_cases import ModelEngine

    class ResizeOnly(ModelEngine):
        def resize(self, *a, **k):
            raise AssertionError('the device route must not be taken')
    vol, tissue = sc.brainweb_phantom()
    kw = dict(KW, loader='brainweb', normalization='standardization')
    got = nifti.volume_to_slices(vol, tissue, engine=ResizeOnly(), device_rotate=False, **kw)
    assert same(got, nifti.volume_to_slices(vol, tissue, **kw))


def test_the_build_tool_forwards_the_method(tmp_path, monkeypatch, capsys):
    import importlib.util
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    names = {'volume': 'FLAIR', 'groundtruth': 'consensus_gt', 'skullmap': 'brainmask'}
    patients = write_patients(tmp_path / 'data', lambda name, kind: f'{name}_{names[kind]}.nii.gz')
    spec = importlib.util.spec_from_file_location('uad_build_cache_tool', os.path.join(ROOT, 'tools', 'build_cache.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    common = [str(tmp_path / 'data'), None, '--res', '32', '--train', '0.5', '--val', '0.5', '--test', '0']
    for cache, extra in (('std', ['--normalization', 'standardization']), ('scl', [])):
        argv = list(common)
        argv[1] = str(tmp_path / cache)
        monkeypatch.setattr('sys.argv', ['build_cache.py'] + argv + extra)
        tool.main()
    capsys.readouterr()
    std, scl = read_cache(str(tmp_path / 'std')), read_cache(str(tmp_path / 'scl'))
    assert std[2]['options'].get('normalization') == 'standardization' and 'normalization' not in scl[2]['options']
    want = nifti.build_cache(str(tmp_path / 'ref'), patients, partition={'TRAIN': 0.5, 'VAL': 0.5, 'TEST': 0.0}, seed=0, axis='axial', slice_start=0,
                             slice_end=155, slice_resolution=(32, 32), normalization='standardization')
    ref = read_cache(str(tmp_path / 'ref'))
    assert want['slices'] == std[0].shape[0] and np.array_equal(std[0], ref[0]) and np.array_equal(std[1], ref[1])
    assert std[0].min() < 0.0 and scl[0].min() >= -0.2 and not np.array_equal(std[0], scl[0])
    monkeypatch.setattr('sys.argv', ['build_cache.py'] + common[:1] + [str(tmp_path / 'x'), '--normalization', 'zscore'])
    with pytest.raises(SystemExit):
        tool.main()
    capsys.readouterr()


def test_the_two_symbols_are_declared_bound_and_exported():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'uad_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(uad_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('uad_shifted_sums_workspace', 'uad_shifted_sums', 'uad_clamp_standardize'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert len(_lib.SYMBOLS['uad_shifted_sums'][1]) == 10 and len(_lib.SYMBOLS['uad_clamp_standardize'][1]) == 8
    assert declared == set(_lib.SYMBOLS)
    ws = _lib.load().uad_shifted_sums_workspace                     # host arithmetic only
    assert ws(0) == 0 and ws(1) == 16 and ws(sc.T) == 16 and ws(sc.T + 1) == 32 and ws(2 ** 31 - 1) == 262144 * 16 and ws(2 ** 31) == 0
    assert math.isclose(_lib.SHIFTED_SUMS_CHAIN, 1072)
