"""Shared by tests/test_rotate_host.py, tests/test_rotate_kernels_host.py and tests/test_gpu_rotate.py: the scipy reference of the device
rotation op (always scipy in fp64 on the fp32-rounded input), the shapes / angles / bars of the three files, the inputs without a rounding tie,
and a numpy RESTATEMENT of what csrc/uad_resample.hip computes for uad_affine_spline3, with switches for the two wrong rules
the restatement must NOT use (mirrored taps beyond the 12-sample padding; the mirror instead of the reflect initial values)."""
import functools

import numpy as np
import scipy.ndimage
import scipy.special

F32_BAR = 1.2e-7             # fp32 output: twice the half-ulp (6e-8) of the final rounding for |v| < 2  (tests/test_gpu_resample.py)
TIE_WINDOW = 1e-9            # int32 output: exact, on inputs with no unrounded value this close to a half-integer
MODES = ('constant', 'nearest')
SHAPES = [(64, 64), (33, 57), (100, 60), (7, 5), (128, 128)]       # ragged 16x16 tiles, non-square offsets, a tiny plane, corners beyond the padding
ANGLES = (15, -10, 37.5, 45, 90, 180)
BATCHES = (1, 7)
PAD = 12                     # scipy.ndimage._interpolation._prepad_for_spline_filter, mode 'nearest'
POLE = np.sqrt(3.0) - 2.0


def rotation_transform(angle, shape):
    """(matrix [2,2], offset [2]) of scipy.ndimage.rotate(a, angle, reshape=False) on a 2-D array, in scipy's own expressions."""
    c, s = scipy.special.cosdg(angle), scipy.special.sindg(angle)
    m = np.array([[c, s], [-s, c]])
    in_center = (np.array(shape, dtype=np.float64) - 1) / 2
    return m, in_center - np.dot(m, in_center)


def scipy_rotate(a, angle, mode):
    return scipy.ndimage.rotate(a, angle, reshape=False, order=3, mode=mode)


def near_ties(unrounded):
    return int(np.count_nonzero(np.abs(np.abs(unrounded - np.floor(unrounded)) - 0.5) < TIE_WINDOW))


def float_batch(n, h, w, seed):
    return np.random.default_rng(seed).random((n, h, w)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def float_reference(n, h, w, mode):
    """-> (input fp32 [n,h,w], scipy fp64 [n, len(ANGLES), h, w]); computed once per process and shared, never written to."""
    a = float_batch(n, h, w, seed=7 * h + 3 * w + n)
    ref = np.stack([np.stack([scipy_rotate(x.astype(np.float64), ang, mode) for ang in ANGLES]) for x in a])
    a.setflags(write=False); ref.setflags(write=False)
    return a, ref


@functools.lru_cache(maxsize=None)
def integer_reference(n, h, w, mode):
    """Blob-shaped integer maps (labels 0..2) without a near-tie voxel under scipy alone at any of ANGLES: the first of a fixed seed sequence
    (the search of tests/test_gpu_resample.py: integer_batch).  -> (maps int [n,h,w], unrounded fp64 [n,A,h,w], scipy's integer result)."""
    for s in range(2000 + h + n, 2000 + h + n + 400):
        rng = np.random.default_rng(s)
        f = scipy.ndimage.gaussian_filter(rng.standard_normal((n, h, w)), (0, min(h, 8) / 4.0, min(w, 8) / 4.0))
        m = (f > np.quantile(f, 0.55)).astype(int) + (f > np.quantile(f, 0.9)).astype(int)
        un = np.stack([np.stack([scipy_rotate(x.astype(np.float64), ang, mode) for ang in ANGLES]) for x in m])
        if near_ties(un) == 0:
            want = np.stack([np.stack([scipy_rotate(x, ang, mode) for ang in ANGLES]) for x in m])
            for arr in (m, un, want):
                arr.setflags(write=False)
            return m, un, want
    raise AssertionError('no tie-free integer input found')


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def coordinates(matrix, offset, out_shape):
    """Input coordinates of every output pixel: the matrix sum first, then the offset (this order is scipy's, bit for bit)."""
    Y, X = np.meshgrid(np.arange(out_shape[0], dtype=np.float64), np.arange(out_shape[1], dtype=np.float64), indexing='ij')
    m = np.asarray(matrix, np.float64)
    return (Y * m[0, 0] + X * m[0, 1]) + offset[0], (Y * m[1, 0] + X * m[1, 1]) + offset[1]


def beyond_padding(matrix, offset, shape, out_shape=None):
    """How many output pixels of a 'nearest' transform have a tap outside the padded plane (where clamping and mirroring differ)."""
    cy, cx = coordinates(matrix, offset, out_shape or shape)
    out = np.zeros(cy.shape, bool)
    for c, ln in ((cy, shape[0]), (cx, shape[1])):
        start = np.floor(c + PAD) - 1
        out |= (start < 0) | (start + 3 > ln + 2 * PAD - 1)
    return int(out.sum())


def prefilter_line(line, init):
    """ni_splines.c for order 3 on one fp64 line: gain 6, causal / anticausal recursion with the 'mirror' or 'reflect' initial values."""
    z = POLE
    c = np.asarray(line, np.float64) * 6.0
    n = len(c)
    zi = z ** np.arange(n)
    if init == 'mirror':
        zn = z ** (n - 1)
        c[0] = (c[0] + zn * c[n - 1] + np.sum(zi[1:n - 1] * (c[1:n - 1] + zn * c[n - 2:0:-1]))) / (1 - zn * zn)
    else:
        zn = z ** n
        c[0] = c[0] + (z / (1 - zn * zn)) * np.sum(zi * (c + zn * c[::-1]))
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1) if init == 'mirror' else c[n - 1] * z / (z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def prefilter_plane(a, init):
    c = np.apply_along_axis(prefilter_line, 0, np.asarray(a, np.float64), init)
    return np.apply_along_axis(prefilter_line, 1, c, init)


def _mirror(idx, ln):
    s2 = 2 * ln - 2
    idx = np.abs(idx) % s2
    return np.where(idx >= ln, s2 - idx, idx)


def _axis(c, ln, fold):
    fl = np.floor(c)
    idx = fl.astype(np.int64)[..., None] - 1 + np.arange(4)
    idx = _mirror(idx, ln) if fold == 'mirror' else np.clip(idx, 0, ln - 1)
    y = c - fl
    zc = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0
    w0 = zc * zc * zc / 6.0
    return idx, np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], -1)


def affine_restated(a, matrix, offset, out_shape=None, mode='constant', nearest_taps='clamp', nearest_init='reflect'):
    """What the device computes for one fp64 [h,w] plane -> unrounded fp64 [H,W].  nearest_taps='mirror' / nearest_init='mirror' are the two
    wrong rules (what the zoom path does), kept so that a test can show they fail."""
    a = np.asarray(a, np.float64)
    h, w = a.shape
    cy, cx = coordinates(matrix, offset, out_shape or a.shape)
    if mode == 'constant':
        coef = prefilter_plane(a, 'mirror')
        inside = ~((cy < 0) | (cy > h - 1) | (cx < 0) | (cx > w - 1))
        fold = 'mirror'
    else:
        coef = prefilter_plane(np.pad(a, PAD, mode='edge'), nearest_init)
        cy, cx = cy + PAD, cx + PAD
        inside = np.ones(cy.shape, bool)
        fold = nearest_taps
    iy, wy = _axis(cy, coef.shape[0], fold)
    ix, wx = _axis(cx, coef.shape[1], fold)
    t = np.zeros(cy.shape)
    for i in range(4):
        for j in range(4):
            t += coef[iy[..., i], ix[..., j]] * wy[..., i] * wx[..., j]
    return np.where(inside, t, 0.0)


def round_half_away(t):
    return np.where(t > 0, (t + 0.5).astype(np.int64), (t - 0.5).astype(np.int64))
