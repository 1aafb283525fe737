"""GPU: the device renderings of the evaluation sample images (uad_render_minmax_u8 / uad_render_heatmap / uad_render_overlay through
device_ops.DeviceOps.render_gray / render_heatmap / render_overlay) and options['exportSamples'] on them.

The reference is always the host statement utils/render.py (pinned by tests/test_render_host.py), never the code under test; shapes, inputs
and references come from tests/render_cases.py, computed once and shared.  Grey, label and overlay images are held to BIT EQUALITY: the
kernels perform the statement's IEEE operations in its order with contraction off.  The heat map is held to INDEX EQUALITY with one
exemption: a pixel may differ by one index where the statement's fp64 q * 256 lies within 1e-9 of an integer -- the device exp() may differ
from the host's by an ulp, which moves q * 256 by about 1e-13 (derived, not measured) -- and such pixels may be at most 0.1 % of a test's
pixels (tests/test_render_kernels_host.py checks on the CPU that a one-ulp nudge of exp stays inside that)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import render_cases as rc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils import Evaluation, png, render
except Exception:
    DeviceOps = None


@pytest.fixture(scope='module')
def eng():
    e = DeviceOps()
    yield e
    e.close()


def _offset_view(eng, a):
    """the batch as a contiguous view one element into a larger buffer: its base is only 4-byte aligned (1-byte for uint8)"""
    flat = torch.empty(a.size + 1, device=eng.device, dtype=torch.from_numpy(a[:0].copy()).dtype)
    flat[1:] = torch.from_numpy(np.array(a)).reshape(-1).to(eng.device)
    v = flat[1:].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _strided(eng, a):
    """the batch as every second column of a wider tensor: not contiguous, the op must make it so"""
    wide = torch.zeros(a.shape[:2] + (2 * a.shape[2],), device=eng.device, dtype=torch.float32)
    wide[..., ::2] = torch.from_numpy(np.array(a, np.float32)).to(eng.device)
    v = wide[..., ::2]
    assert not v.is_contiguous() or a.shape[2] == 1
    return v


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_grey_images_have_the_bytes_of_the_host_statement(eng, case):
    n, hw = case
    for kind in rc.GREY_KINDS if n < rc.N_FOLD else ('uniform',):
        got = eng.render_gray(rc.grey_input(n, hw, kind).copy())
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n,) + hw and got.is_cuda
        g, ref = got.cpu().numpy(), rc.grey_reference(n, hw, kind)
        print(f'render_gray {rc.case_id(case)} {kind}: {int((g != ref).sum())} bytes differ')
        assert np.array_equal(g, ref), kind
    if n <= 3:
        x, ref = rc.grey_input(n, hw, 'uniform'), rc.grey_reference(n, hw, 'uniform')
        assert np.array_equal(eng.render_gray(_offset_view(eng, x)).cpu().numpy(), ref)
        assert np.array_equal(eng.render_gray(_strided(eng, x)).cpu().numpy(), ref)
        # a slice's bytes depend on neither n nor its place in the batch
        assert np.array_equal(eng.render_gray(x[n - 1:n].copy()).cpu().numpy(), ref[n - 1:n])
        # the label map: integers cast to fp32
        lab = (rc.overlay_input(n, hw)[2] * np.int64(10)).astype(np.int64)
        assert np.array_equal(eng.render_gray(lab).cpu().numpy(), render.label_u8(lab))


def test_heat_maps_have_the_indices_of_the_host_statement(eng):
    """One test over every shape, so that the 0.1 % cap on exempt pixels is taken of all its pixels."""
    total = differ_all = 0
    for case in rc.CASES:
        n, hw = case
        for kind in rc.HEAT_KINDS if n < rc.N_FOLD else ('lesions',):
            d, q256 = rc.heat_input(n, hw, kind), rc.heat_q256(n, hw, kind)
            variants = [d.copy()] + ([_offset_view(eng, d), _strided(eng, d)] if n <= 3 and kind == 'lesions' else [])
            for v in variants:
                got = eng.render_heatmap(v, lut=rc.INDEX_LUT)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (n,) + hw + (4,)
                g = got.cpu().numpy()
                assert np.array_equal(g, rc.INDEX_LUT[g[..., 0]])                                    # whole table entries, bytes in order
                differ, uncovered = rc.heat_mismatch(g[..., 0], q256)
                print(f'render_heatmap {rc.case_id(case)} {kind}: {differ} of {g[..., 0].size} indices differ, {uncovered} outside the exemption')
                assert uncovered == 0, (case, kind)
                total += g[..., 0].size
                differ_all += differ
    print(f'render_heatmap: {differ_all} exempt pixels of {total}')
    assert differ_all <= rc.EXEMPT_CAP * total
    # the default table is the package's jet table
    d = rc.heat_input(3, (5, 7), 'zeros')
    assert np.array_equal(eng.render_heatmap(d.copy()).cpu().numpy(), render.heatmap_rgba(d))        # no exp() in a heat map of zeros
    assert np.array_equal(eng.render_heatmap(torch.from_numpy(d.copy()).to(eng.device), lut=torch.from_numpy(render.jet_u8().copy())).cpu().numpy(),
                          render.heatmap_rgba(d))
    with pytest.raises(ValueError):
        eng.render_heatmap(d, lut=np.zeros((256, 3), np.uint8))


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_overlays_have_the_bytes_of_the_host_statement(eng, case):
    n, hw = case
    x, pred, gt = rc.overlay_input(n, hw)
    ref = rc.overlay_reference(n, hw)
    got = eng.render_overlay(x.copy(), pred.copy(), gt.copy())
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n,) + hw + (3,) and got.is_cuda
    print(f'render_overlay {rc.case_id(case)}: {int((got.cpu().numpy() != ref).sum())} bytes differ')
    assert np.array_equal(got.cpu().numpy(), ref)
    if n <= 3:
        dev = lambda a: torch.from_numpy(a.copy()).to(eng.device)
        assert np.array_equal(eng.render_overlay(_offset_view(eng, x), _offset_view(eng, pred), dev(gt)).cpu().numpy(), ref)
        assert np.array_equal(eng.render_overlay(_strided(eng, x), _strided(eng, pred), dev(gt)).cpu().numpy(), ref)
        assert np.array_equal(eng.render_overlay(dev(x), dev(pred) * 0.25, dev(gt).to(torch.int32) * 10).cpu().numpy(), ref)


def test_render_refusals_and_the_abi(eng):
    with pytest.raises(ValueError):
        eng.render_gray(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        eng.render_overlay(np.zeros((1, 4, 4), np.float32), np.zeros((1, 4, 5), np.float32), np.zeros((1, 4, 4), bool))
    with pytest.raises(ValueError):
        eng.render_overlay(np.zeros((1, 4, 4), np.float32), np.zeros((1, 4, 4), np.float32), np.zeros((2, 4, 4), bool))
    assert tuple(eng.render_gray(np.zeros((0, 4, 4), np.float32)).shape) == (0, 4, 4)
    assert tuple(eng.render_heatmap(np.zeros((0, 4, 4), np.float32)).shape) == (0, 4, 4, 4)
    lib, st = eng.lib, eng._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.rand(2, 35, device=eng.device)
    pred = torch.zeros(2, 35, device=eng.device)
    gt = torch.zeros(2, 35, dtype=torch.uint8, device=eng.device)
    lut = torch.from_numpy(render.jet_u8().copy()).to(eng.device)
    out = torch.full((2 * 35 * 4 + 1,), 0xa5, dtype=torch.uint8, device=eng.device)
    ok = (p(x), 2, 35, p(out), st)
    assert lib.uad_render_minmax_u8(*ok) == _lib.UAD_OK
    for pos, val in ((1, -1), (2, 0), (2, -3), (0, None), (3, None), (3, p(x))):
        args = list(ok)
        args[pos] = val
        assert lib.uad_render_minmax_u8(*args) == 1, (pos, val)
    assert b'render_minmax_u8' in lib.uad_last_error()
    okh = (p(x), 2, 5, 7, p(lut), p(out), st)
    assert lib.uad_render_heatmap(*okh) == _lib.UAD_OK
    for pos, val in ((1, -1), (2, 0), (3, 0), (0, None), (4, None), (5, None), (5, p(x)), (5, C.c_void_p(out.data_ptr() + 1))):
        args = list(okh)
        args[pos] = val
        assert lib.uad_render_heatmap(*args) == 1, (pos, val)
    assert lib.uad_render_heatmap(p(x), 1, 65536, 65536, p(lut), p(out), st) == 3                    # 2^32 pixels a slice: unsupported, nothing launched
    oko = (p(x), p(pred), p(gt), 2, 35, p(out), st)
    assert lib.uad_render_overlay(*oko) == _lib.UAD_OK
    for pos, val in ((3, -1), (4, 0), (0, None), (1, None), (2, None), (5, None), (5, p(x)), (5, p(pred)), (5, p(gt))):
        args = list(oko)
        args[pos] = val
        assert lib.uad_render_overlay(*args) == 1, (pos, val)
    # n == 0 is UAD_OK and launches nothing: NULL pointers are not even looked at, the output stays as it was
    out.fill_(0xa5)
    assert lib.uad_render_minmax_u8(None, 0, 35, None, st) == _lib.UAD_OK
    assert lib.uad_render_heatmap(None, 0, 5, 7, None, None, st) == _lib.UAD_OK
    assert lib.uad_render_overlay(None, None, None, 0, 35, None, st) == _lib.UAD_OK
    assert lib.uad_render_minmax_u8(p(x), 0, 35, p(out), st) == _lib.UAD_OK
    torch.cuda.synchronize()
    assert bool((out == 0xa5).all())
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'uad_hip.h')).read()
    for name in ('uad_render_minmax_u8', 'uad_render_heatmap', 'uad_render_overlay'):
        assert name in _lib.SYMBOLS and name + '(' in header and hasattr(lib, name)


def test_export_samples_on_the_engine_writes_the_files_of_the_host_path(eng, tmp_path):
    """evaluate() with exportSamples for one small patient (4 slices of 16 x 16): the real engine renders on the device, the same engine with
    its render ops hidden takes utils/render.py; the files are byte-identical."""
    import types
    from tests.test_evaluation_entry import BlurModel, _opts
    from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import SyntheticPatientDataset

    class Hidden:
        """the engine without its render ops"""
        def __init__(self, e):
            self._e = e

        def __getattr__(self, k):
            if k.startswith('render_'):
                raise AttributeError(k)
            return getattr(self._e, k)

    ds = SyntheticPatientDataset(n_val=0, n_test=1, slices=4, native=16, h=16, w=16, seed=2, slice_start=0, slice_end=4)
    dirs = []
    for engine, tag in ((eng, 'device'), (Hidden(eng), 'host')):
        model = BlurModel(tmp_path, bs=3)
        model.engine = engine
        opt = dict(_opts(tmp_path, h=16), exportSamples=True, erodeBrainmask=False)
        ev = Evaluation.evaluate(ds, model, opt, epoch='1', description=tag)
        dirs.append(os.path.join(ev['eval_dir'], 'samples_test_PC'))
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and len(names) == 4 * 7
    for name in names:
        a, b = (open(os.path.join(d, name), 'rb').read() for d in dirs)
        assert a == b, name
    assert png.read_png(os.path.join(dirs[0], '0_2_heatmap.png')).shape == (16, 16, 4)
