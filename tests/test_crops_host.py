"""CPU: the host statement of the crop modes (utils/crops.py) and volume_to_slices(crops=...) on it.

component_props against the literal per-component loop of tests/crops_cases.py (np.argwhere per scipy label); lesion_crop_origins against a
restatement of dataloaders/MSLUB.py:203-220 in the reference's own floats (float centroid, float clamps, int(), crop(), the shape check);
random_crop_origins against the reference's two randint lines under RandomState(7); volume_to_slices, for every crop mode, against the
reference's crop step applied slice by slice to the uncropped output.  Everything compared is an integer or a copied value: equality.
skimage is not installed, so nothing here compares with skimage's own label / regionprops."""
import numpy as np
import pytest

from tests import crops_cases as cc
from unsupervised_anomaly_detection_brain_mri_amd.utils import crops, nifti


@pytest.mark.parametrize('shape', cc.PROPS_SHAPES, ids=cc.shape_id)
def test_component_props_against_the_literal_loop(shape):
    for kind in cc.KINDS:
        for slab in cc.SLABS:
            got = cc.props_reference(shape, kind, slab)
            assert got.dtype == np.int64 and np.array_equal(got, cc.props_loop(cc.mask(shape, kind), slab)), (kind, slab)
            assert (np.diff(got[:, 0]) > 0).all()                                     # ordered by the first index
            assert got[:, 1].sum() == cc.mask(shape, kind).sum()
            # the label model of uad_cc_label carries the same components: rows are the roots, in index order
            lab = cc.labels_model(shape, kind, slab)
            assert np.array_equal(np.flatnonzero(lab.ravel() == np.arange(1, lab.size + 1)), got[:, 0])
            assert np.array_equal(crops.component_props(lab, slab), got)


def test_component_props_structured_volumes():
    chain = cc.mask((1, 9, 33), 'chain')
    assert len(cc.props_reference((1, 9, 33), 'chain', 0)) == 1                        # 8-connected ...
    from scipy.ndimage import label
    assert label(chain[0])[1] > 1                                                     # ... but not 4-connected
    p = cc.props_reference((3, 9, 9), 'corner', 1)
    assert np.array_equal(p, cc.props_loop(cc.mask((3, 9, 9), 'corner'), 1))
    assert p[:, 1].tolist() == [13, 2, 1]                                             # the two squares are ONE component; the diagonal pair; the pixel two rows off
    full = cc.props_reference((3, 9, 33), 'full', 0)
    assert full.tolist() == [[9 * 33, 9 * 33, 9 * 33, 33 * 36, 9 * 528]]
    assert cc.props_reference(cc.SPAN_SHAPE, 'empty', 0).shape == (0, 5) and cc.props_reference(cc.SPAN_SHAPE, 'empty', 1).dtype == np.int64
    for slab, n in ((0, 1), (1, 5), (2, 3)):
        assert len(cc.props_reference(cc.SPAN_SHAPE, 'span', slab)) == n
        assert np.array_equal(cc.props_reference(cc.SPAN_SHAPE, 'span', slab), cc.props_loop(cc.mask(cc.SPAN_SHAPE, 'span'), slab))
    with pytest.raises(ValueError):
        crops.component_props(np.zeros((4, 4)))


def test_slab_one_is_every_slice_on_its_own():
    shape = (5, 37, 53)
    m = cc.mask(shape, 'fill30')
    whole = cc.props_reference(shape, 'fill30', 0)
    per_slice = cc.props_reference(shape, 'fill30', 1)
    assert len(per_slice) > len(whole)
    rows = []
    for z in range(shape[0]):
        p = crops.component_props(m[z:z + 1], 0).copy()
        p[:, 0] += z * shape[1] * shape[2]
        p[:, 2] += z * p[:, 1]
        rows.append(p)
    assert np.array_equal(per_slice, np.concatenate(rows))
    assert np.array_equal(crops.component_props(m, shape[0]), whole) and np.array_equal(crops.component_props(m, 99), whole)


def _origins_by_the_reference_lines(labels, crop_w, crop_h):
    out = []
    for s, seg in enumerate(labels):
        out += [(s, y, x) for _, _, (y, x) in cc.reference_lesion_crops(seg, seg, crop_w, crop_h)]
    return np.array(out, np.int32).reshape(-1, 3)


def border_slices():
    """[6,20,24] label batch: a fractional centroid; a component on each border and in two corners; an L whose floored centroid differs from
    its rounded one; two components in one slice in raster order."""
    b = np.zeros((6, 20, 24), np.float32)
    b[0, 8:10, 8:11] = 1; b[0, 10, 8] = 1                          # centroid (8.857.., 8.857..)
    b[1, 0:2, 10:13] = 1                                           # top
    b[1, 18:20, 3:5] = 1                                           # bottom
    b[2, 9:12, 0:2] = 1                                            # left
    b[2, 5:8, 22:24] = 1                                           # right
    b[3, 0, 0] = 1                                                 # corners
    b[3, 19, 23] = 1
    b[4, 4:9, 4] = 1; b[4, 8, 4:12] = 1                            # an L
    b[5, 3, 15] = 1; b[5, 3, 2] = 1; b[5, 2, 20] = 1               # raster order: (2,20), (3,2), (3,15)
    return b


@pytest.mark.parametrize('crop_w,crop_h', [(8, 6), (7, 5), (8, 5), (7, 6), (2, 2), (1, 1), (24, 20), (23, 19), (24, 1)])
def test_lesion_crop_origins_against_the_float_restatement(crop_w, crop_h):
    b = border_slices()
    props = crops.component_props(b, slab=1)
    assert len(props) == 11
    got = crops.lesion_crop_origins(props, 20, 24, crop_w, crop_h)
    want = _origins_by_the_reference_lines(b, crop_w, crop_h)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got.tolist(), want.tolist())
    # the drop rule: never with even sizes; with an odd size exactly the components whose centre sits on the upper bound of that axis
    cy, cx = props[:, 3] // props[:, 1], props[:, 4] // props[:, 1]
    dropped = ((crop_h % 2 == 1) & (cy >= 20 - crop_h // 2)) | ((crop_w % 2 == 1) & (cx >= 24 - crop_w // 2))
    assert len(got) == len(props) - int(dropped.sum())
    if crop_w % 2 == 0 and crop_h % 2 == 0:
        assert len(got) == len(props)
    if (crop_w, crop_h) == (7, 5):
        kept = {tuple(r[:1]) for r in got.tolist()}
        assert dropped.sum() == 3 and (1,) in kept and (2,) in kept                   # bottom, right and the bottom-right corner go; top and left stay
    windows = crops.crop_windows(b, got, crop_h, crop_w)
    assert windows.shape == (len(got), crop_h, crop_w)
    if crop_w > 1 and crop_h > 1 and (crop_w, crop_h) != (2, 2):
        assert windows.any(axis=(1, 2)).all()


def test_lesion_crop_origins_floor_equals_the_clamped_float():
    """int(clamp(c, lo, hi)) == clamp(floor(c), lo, hi) for c >= 0 and integer lo <= hi: on every centroid k / a of small components."""
    for a in range(1, 40):
        for k in range(0, 30 * a, 7):
            for lo, hi in ((0, 29), (3, 26), (14, 15), (15, 15)):
                c = k / a
                f = lo if c < lo else c
                f = hi if f > hi else f
                assert int(f) == min(max(k // a, lo), hi)


def test_lesion_crop_origins_refusals_and_empties():
    props = crops.component_props(border_slices(), slab=1)
    for w, h in ((25, 6), (8, 21), (0, 5), (5, 0)):
        with pytest.raises(ValueError):
            crops.lesion_crop_origins(props, 20, 24, w, h)
    e = crops.lesion_crop_origins(np.zeros((0, 5), np.int64), 20, 24, 8, 6)
    assert e.shape == (0, 3) and e.dtype == np.int32
    assert crops.crop_windows(border_slices(), e, 6, 8).shape == (0, 6, 8)
    full = crops.lesion_crop_origins(props, 20, 24, 24, 20)                           # crop == slice: every component gives the slice itself
    assert np.array_equal(full[:, 1:], np.zeros((11, 2), np.int32))


def test_random_crop_origins_are_the_reference_draws():
    n, H, W, cw, ch, per = 5, 40, 44, 16, 12, 3
    got = crops.random_crop_origins(n, H, W, cw, ch, per, np.random.RandomState(7))
    rs = np.random.RandomState(7)
    want = []
    for s in range(n):
        rx = rs.randint(0, high=(W - cw), size=per)                                   # BRAINWEB.py:167-170
        ry = rs.randint(0, high=(H - ch), size=per)
        want += [(s, ry[r], rx[r]) for r in range(per)]
    assert got.dtype == np.int32 and np.array_equal(got, np.array(want, np.int32))
    assert got[:, 1].max() < H - ch and got[:, 2].max() < W - cw
    np.random.seed(7)                                                                 # the default stream is the numpy.random module, as in the reference
    assert np.array_equal(crops.random_crop_origins(n, H, W, cw, ch, per), got)
    for w, h in ((44, 12), (16, 40), (45, 12), (0, 3)):
        with pytest.raises(ValueError):
            crops.random_crop_origins(n, H, W, w, h, per, np.random.RandomState(7))
    assert crops.random_crop_origins(0, H, W, cw, ch, per, rs).shape == (0, 3)


def test_crop_windows_copy_the_values():
    for size in cc.CROP_SIZES:
        o, want = cc.crop_origins(size), cc.crop_reference(size)
        b = cc.crop_batch()
        for j, (s, t, l) in enumerate(o):
            assert cc.same_bits(want[j], b[s, t:t + size[0], l:l + size[1]])
    for bad in ([[7, 0, 0]], [[0, 64, 0]], [[0, 0, 68]], [[0, -1, 0]], [[0, 0]], [[0.0, 0, 0]]):
        with pytest.raises(ValueError):
            crops.crop_windows(cc.crop_batch(), bad, 3, 5)


SPECS = [('center', 20, 16), ('lesions', 16, 12), ('lesions', 15, 11), ('lesions', 44, 40), ('random', 16, 12, 3)]


@pytest.mark.parametrize('loader', ['mslub', 'brainweb'])
@pytest.mark.parametrize('rotations', [(0,), (0, 10)], ids=['plain', 'rotated'])
def test_volume_to_slices_crops_against_the_per_slice_loop(loader, rotations):
    args, kw = cc.loader_inputs(loader)
    if rotations != (0,):
        kw = {**kw, 'slice_start': 3, 'slice_end': 7}                                 # (scipy's rotate per slice and angle: keep it short)
    base = nifti.volume_to_slices(*args, rotations=rotations, **kw)
    assert base[0].shape[1:] == (40, 44)
    for spec in SPECS:
        if spec[0] == 'lesions' and rotations != (0,):
            with pytest.raises(ValueError):
                nifti.volume_to_slices(*args, rotations=rotations, crops=spec, **kw)
            continue
        got = nifti.volume_to_slices(*args, rotations=rotations, crops=spec, rng=np.random.RandomState(7), **kw)
        want = cc.crops_loop(*base, spec, np.random.RandomState(7))
        assert got[2] == want[2] and got[0].dtype == got[1].dtype == np.float32
        assert cc.same_bits(got[0], want[0]) and cc.same_bits(got[1], want[1]), spec
        assert got[0].shape[1:] == (spec[2], spec[1]) and len(got[2]) >= len(base[2]) // 2
    # ('center', w, h) is center_crop=(w, h)
    a = nifti.volume_to_slices(*args, rotations=rotations, crops=('center', 20, 16), **kw)
    b = nifti.volume_to_slices(*args, rotations=rotations, center_crop=(20, 16), **kw)
    assert a[2] == b[2] and cc.same_bits(a[0], b[0]) and cc.same_bits(a[1], b[1])


def test_volume_to_slices_crop_counts_on_the_phantom():
    args, kw = cc.loader_inputs('mslub')
    even = nifti.volume_to_slices(*args, crops=('lesions', 16, 12), **kw)
    odd = nifti.volume_to_slices(*args, crops=('lesions', 15, 11), **kw)
    seg = cc.phantom()[1]
    assert len(even[2]) == len(crops.component_props(seg[:11], slab=1)) == 21          # one crop per component and slice
    assert even[2] == sorted(even[2]) and 0 not in even[2] and 1 not in even[2]
    assert 0 < len(odd[2]) < len(even[2])                                             # the bottom / right border components are dropped
    assert even[1].any(axis=(1, 2)).all()
    rnd = nifti.volume_to_slices(*args, crops=('random', 16, 12, 3), rng=np.random.RandomState(1), **kw)
    assert rnd[2] == [s for s in range(11) for _ in range(3)]
    empty = nifti.volume_to_slices(*args, crops=('lesions', 16, 12), **{**kw, 'slice_start': 0, 'slice_end': 2})
    assert empty[0].shape == (0, 12, 16) and empty[1].shape == (0, 12, 16) and empty[2] == []


def test_volume_to_slices_crop_refusals():
    args, kw = cc.loader_inputs('mslub')
    for bad in (dict(crops=('center', 20, 16), center_crop=(20, 16)), dict(crops=('lesions', 16, 12), center_crop=(20, 16)),
                dict(crops=('lesions', 16, 12), rotations=(0, 10)), dict(crops=('lesions', 16, 12), rotations=(5,)),
                dict(crops=('patches', 16, 12)), dict(crops=('lesions', 16)), dict(crops=('random', 16, 12)), dict(crops=('random', 16, 12, 0)),
                dict(crops=('lesions', 0, 12)), dict(crops=('lesions', 45, 12)), dict(crops=('lesions', 16, 41)), dict(crops=('random', 44, 12, 2)),
                dict(crops=('random', 16, 40, 2)), dict(crops='lesions')):
        with pytest.raises(ValueError):
            nifti.volume_to_slices(*args, **{**kw, **bad})
    args, kw = cc.loader_inputs('brainweb')
    with pytest.raises(ValueError):
        nifti.volume_to_slices(*args, crops=('lesions', 16, 12), rotations=(0, 10), **kw)
    assert len(nifti.volume_to_slices(*args, crops=('lesions', 16, 12), **kw)[2]) == 21      # 'lesions' with loader='brainweb' is allowed


def test_build_cache_passes_the_crops_through(tmp_path):
    from unsupervised_anomaly_detection_brain_mri_amd.utils.slice_cache import read_cache
    vol, seg, brainmask, _ = cc.phantom()
    nifti.write_nifti(str(tmp_path / 'flair.nii.gz'), vol)
    nifti.write_nifti(str(tmp_path / 'gt.nii.gz'), seg, dtype='u1')
    nifti.write_nifti(str(tmp_path / 'mask.nii.gz'), brainmask, dtype='u1')
    patients = [{'name': 'p0', 'volume': str(tmp_path / 'flair.nii.gz'), 'groundtruth': str(tmp_path / 'gt.nii.gz'), 'skullmap': str(tmp_path / 'mask.nii.gz')}]
    for spec in (('lesions', 16, 12), ('random', 16, 12, 2)):
        kw = dict(slice_start=0, slice_end=155, slice_resolution=None, crops=spec)
        nifti.build_cache(str(tmp_path / spec[0]), patients, partition={'TRAIN': 1.0}, rng=np.random.RandomState(5), **kw)
        images, labels, info = read_cache(str(tmp_path / spec[0]))
        want = nifti.volume_to_slices(*(nifti.read_nifti(patients[0][k])[0] for k in ('volume', 'groundtruth', 'skullmap')), rng=np.random.RandomState(5), **kw)
        assert np.array_equal(images[..., 0], want[0]) and np.array_equal(labels > 5, want[1] > 0)
        assert info['options']['crops'] == list(spec) and 'rng' not in info['options']
