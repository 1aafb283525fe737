"""CPU: the host statement of the 8-bit sample-image renderings (utils/render.py: minmax_u8, label_u8, heatmap_rgba, overlay_rgb) pinned on
hand-derived cases and on a scalar per-pixel restatement, the committed jet table against matplotlib, and the PNG codec (utils/png.py)
against PIL and against itself.  The device ops of csrc/uad_render.hip are held to this statement (tests/test_render_kernels_host.py on the
CPU, tests/test_gpu_render.py on the GPU)."""
import math
import os
import struct
import zlib

import numpy as np
import pytest

from tests import render_cases as rc
from unsupervised_anomaly_detection_brain_mri_amd.utils import png, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- minmax_u8 / label_u8
def test_minmax_u8_on_hand_derived_slices():
    assert render.minmax_u8(np.full((1, 1, 1), 0.7, f32)).tolist() == [[[0]]]                        # 1 x 1: smax == smin -> scale 0
    assert not render.minmax_u8(np.full((2, 3, 5), -4.25, f32)).any()                                # a constant slice gives zeros
    # smin = -1, smax = 3: scale = 63.75, shift = 63.75 (both fp32 numbers): -1 -> 0, 0 -> 63.75 -> 63, 1 -> 127.5 -> 127, 3 -> 255
    assert render.minmax_u8(np.array([[[-1, 0], [1, 3]]], f32)).tolist() == [[[0, 63], [127, 255]]]
    # the grey level of smax is 255, of the midpoint 127 (127.5 truncated)
    assert render.minmax_u8(np.array([[[0, 0.5, 1]]], f32)).tolist() == [[[0, 127, 255]]]
    # all-negative: -3 -> 0, -2 -> 127, -1 -> 255
    assert render.minmax_u8(np.array([[[-3], [-2], [-1]]], f32)).tolist() == [[[0], [127], [255]]]
    # smax - smin = 1e-20 is not zero in fp32 but below DBL_EPSILON: scale 0
    assert not render.minmax_u8(np.array([[[1e-20, 2e-20]]], f32)).any()
    # every slice has its own range
    two = render.minmax_u8(np.array([[[0, 1]], [[0, 2]]], f32))
    assert two.tolist() == [[[0, 255]], [[0, 255]]] and two.dtype == np.uint8
    with pytest.raises(ValueError):
        render.minmax_u8(np.zeros((3, 3), f32))


def test_label_u8_is_minmax_of_the_label_map_cast_to_fp32():
    g = np.array([[[0, 1], [1, 0]], [[0, 0], [0, 0]], [[0, 10], [2, 10]]], np.int64)
    assert render.label_u8(g).tolist() == [[[0, 255], [255, 0]], [[0, 0], [0, 0]], [[0, 255], [51, 255]]]
    assert np.array_equal(render.label_u8(g.astype(bool)), render.minmax_u8(g.astype(bool).astype(f32)))


def _minmax_scalar(s):
    """the statement for one slice, one IEEE operation at a time"""
    flat = [f32(v) for v in s.ravel().tolist()]
    smin, smax = min(flat), max(flat)
    diff = float(smax) - float(smin)
    scale = 255.0 / diff if diff > 2.220446049250313e-16 else 0.0
    shift = -float(smin) * scale
    out = []
    for v in flat:
        t = f32(f32(v * f32(scale)) + f32(shift))
        out.append(min(max(int(math.trunc(float(t))), 0), 255))
    return np.array(out, np.uint8).reshape(s.shape)


def test_minmax_u8_against_a_scalar_restatement():
    for n, hw in ((3, (5, 7)), (1, (33, 31))):
        for kind in rc.GREY_KINDS:
            x = rc.grey_input(n, hw, kind)
            assert np.array_equal(rc.grey_reference(n, hw, kind), np.stack([_minmax_scalar(s) for s in x])), (hw, kind)
    wide = (np.random.default_rng(3).standard_normal((2, 9, 11)) * 1e6).astype(f32)
    assert np.array_equal(render.minmax_u8(wide), np.stack([_minmax_scalar(s) for s in wide]))


# ---------------------------------------------------------------------------------------------------------------- heat map
def test_heatmap_colour_bar_and_the_end_indices():
    # residuals exactly 0: squash(0) = 0 everywhere, the last column is the bar i / H = 0, .25, .5, .75; min 0, max .75:
    # q / max = 0, 1/3, 2/3, 1 -> int(q * 256) = 0, 85, 170, 256 -> 255
    idx = render.heatmap_index(np.zeros((1, 4, 3), f32))
    assert idx.tolist() == [[[0, 0, 0], [0, 0, 85], [0, 0, 170], [0, 0, 255]]]
    # w = 1: the bar overwrites the whole slice, whatever the residuals are
    assert render.heatmap_index(np.full((1, 4, 1), 0.3, f32)).tolist() == [[[0], [85], [170], [255]]]
    # 1 x 1: the bar is 0 / 1 = 0, max 0: no division, index 0
    assert render.heatmap_index(np.full((1, 1, 1), 5.0, f32)).tolist() == [[[0]]]
    # index 255 away from the bar: squash(1.0) = 1 in fp64 (exp(-100) vanishes next to 1) is the maximum, squash(0) = 0 the minimum;
    # the bar 0, .5 lands on 0 and 128
    d = np.array([[[1.0, 0.0, 9.0], [0.0, 1.0, 9.0]]], f32)
    assert render.heatmap_index(d).tolist() == [[[255, 0, 0], [0, 255, 128]]]
    # a negative residual squashes below zero and becomes the minimum: -10 -> q = -1; 0 -> 0; bar 0: (q + 1) / 1 * 256
    assert render.heatmap_index(np.array([[[-10.0, 0.0, 0.0]]], f32)).tolist() == [[[0, 255, 255]]]


def test_heatmap_rgba_looks_the_table_up():
    d = rc.heat_input(3, (5, 7), 'lesions')
    idx = render.heatmap_index(d)
    assert np.array_equal(render.heatmap_rgba(d), render.jet_u8()[idx]) and render.heatmap_rgba(d).shape == (3, 5, 7, 4)
    assert np.array_equal(render.heatmap_rgba(d, rc.INDEX_LUT)[..., 0], idx)                         # any 256-entry map works
    assert np.array_equal(render.heatmap_rgba(np.zeros((1, 4, 3), f32))[0, 3, 2], [127, 0, 0, 255])  # jet's last entry: dark red
    assert np.array_equal(render.heatmap_rgba(np.zeros((1, 4, 3), f32))[0, 0, 0], [0, 0, 127, 255])  # ... and its first: dark blue
    with pytest.raises(ValueError):
        render.heatmap_rgba(d, np.zeros((255, 4), np.uint8))


def _heat_scalar(s):
    h, w = s.shape
    q = [[0.0] * w for _ in range(h)]
    for i in range(h):
        for j in range(w):
            if j == w - 1:
                q[i][j] = i / h
            else:
                q[i][j] = 2.0 * (1.0 / (1.0 + math.exp(-100.0 * float(s[i, j]))) - 0.5)
    lo = min(min(r) for r in q)
    q = [[v - lo for v in r] for r in q]
    hi = max(max(r) for r in q)
    if hi != 0:
        q = [[v / hi for v in r] for r in q]
    return np.array([[min(int(v * 256.0), 255) for v in r] for r in q], np.uint8)


def test_heatmap_index_against_a_scalar_restatement():
    for n, hw in ((3, (5, 7)), (1, (33, 31)), (1, (9, 1))):
        for kind in rc.HEAT_KINDS:
            d = rc.heat_input(n, hw, kind)
            assert np.array_equal(rc.heat_reference_index(n, hw, kind), np.stack([_heat_scalar(s) for s in d])), (hw, kind)
    signed = (np.random.default_rng(4).standard_normal((2, 6, 5)) * 0.02).astype(f32)
    assert np.array_equal(render.heatmap_index(signed), np.stack([_heat_scalar(s) for s in signed]))


def test_the_committed_jet_table():
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'jet_u8.npy'))
    assert golden.shape == (256, 4) and golden.dtype == np.uint8 and np.array_equal(golden, render.jet_u8())
    matplotlib = pytest.importorskip('matplotlib')
    import matplotlib.cm
    assert np.array_equal(np.uint8(matplotlib.cm.jet(np.arange(256)) * 255), golden), matplotlib.__version__


def test_render_needs_no_matplotlib_at_run_time():
    import subprocess
    import sys
    code = ('import sys; sys.modules["matplotlib"] = None\n'
            'import numpy as np\n'
            'from unsupervised_anomaly_detection_brain_mri_amd.utils import render\n'
            'assert render.heatmap_rgba(np.zeros((1, 4, 3), np.float32)).shape == (1, 4, 3, 4)\n')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=ROOT)


# ---------------------------------------------------------------------------------------------------------------- overlay
def test_overlay_classes_and_grey_levels():
    x = np.array([[[0.5, 0.5, 0.5, 0.5], [-0.2, 1.5, 1.0, 0.0]]], f32)
    pred = np.array([[[1, 1, 0, 0], [0, 0, 0, 0]]], f32)
    gt = np.array([[[1, 0, 1, 0], [0, 0, 0, 0]]], bool)
    v = render.overlay_rgb(x, pred, gt)
    assert v.shape == (1, 2, 4, 3) and v.dtype == np.uint8
    assert v[0, 0].tolist() == [[0, 255, 0], [255, 127, 0], [255, 0, 0], [127, 127, 127]]            # TP, FP (0.5 -> 127), FN, grey 0.5 -> 127
    assert v[0, 1].tolist() == [[0, 0, 0], [255, 255, 255], [255, 255, 255], [0, 0, 0]]              # negatives -> 0, above 1 -> 255
    # any non-zero prediction / label counts
    assert np.array_equal(render.overlay_rgb(x, pred * 0.25, gt.astype(np.int64) * 10), v)


def test_overlay_against_a_scalar_restatement():
    x, pred, gt = rc.overlay_input(3, (5, 7))
    want = np.zeros(x.shape + (3,), np.uint8)
    for k in np.ndindex(x.shape):
        p, g = bool(pred[k]), bool(gt[k])
        if p and g:
            c = (f32(0), f32(1), f32(0))
        elif p:
            c = (f32(1), f32(0.5), f32(0))
        elif g:
            c = (f32(1), f32(0), f32(0))
        else:
            c = (max(x[k], f32(0)),) * 3
        want[k] = [int(math.trunc(float(f32(min(max(t, f32(0)), f32(1)) * f32(255))))) for t in c]
    assert np.array_equal(rc.overlay_reference(3, (5, 7)), want)


# ---------------------------------------------------------------------------------------------------------------- PNG
def _images():
    rng = np.random.default_rng(11)
    for hw in ((1, 1), (5, 7), (128, 128)):
        for c in (None, 3, 4):
            yield rng.integers(0, 256, hw + (() if c is None else (c,)), dtype=np.uint8)


def test_write_png_against_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    for k, a in enumerate(_images()):
        path = str(tmp_path / f'{k}.png')
        png.write_png(path, a)
        with Image.open(path) as im:
            assert im.mode == ('L' if a.ndim == 2 else {3: 'RGB', 4: 'RGBA'}[a.shape[2]])
            assert im.size == (a.shape[1], a.shape[0])
            assert np.array_equal(np.asarray(im), a), a.shape


def test_png_round_trip_and_the_file_structure(tmp_path):
    for k, a in enumerate(_images()):
        path = str(tmp_path / f'{k}.png')
        png.write_png(path, a)
        back = png.read_png(path)
        assert back.dtype == np.uint8 and back.shape == a.shape and np.array_equal(back, a)
    data = png.encode_png(np.arange(35, dtype=np.uint8).reshape(5, 7))
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR' and data[-8:-4] == b'IEND'
    assert struct.unpack('>IIBBBBB', data[16:29]) == (7, 5, 8, 0, 0, 0, 0)                           # width, height, depth, colour type 0
    assert struct.unpack('>I', data[29:33])[0] == zlib.crc32(data[12:29])
    n, = struct.unpack('>I', data[33:37])
    raw = zlib.decompress(data[41:41 + n])
    assert len(raw) == 5 * 8 and set(raw[0::8]) == {0}                                               # filter 0 on every row
    assert struct.unpack('>IIBBBBB', png.encode_png(np.zeros((2, 3, 3), np.uint8))[16:29])[3] == 2
    assert struct.unpack('>IIBBBBB', png.encode_png(np.zeros((2, 3, 4), np.uint8))[16:29])[3] == 6
    broken = bytearray(data)
    broken[45] ^= 1
    with pytest.raises(ValueError):
        png.decode_png(bytes(broken))
    for bad in (np.zeros((2, 2), np.float32), np.zeros((2, 2, 2), np.uint8), np.zeros((0, 2), np.uint8)):
        with pytest.raises((TypeError, ValueError)):
            png.encode_png(bad)
