"""Shared cases of tests/test_batch_kernels_host.py (CPU, the kernels behind the host shim) and tests/test_gpu_batch.py (GPU): label stores,
masks and batches from seeded numpy generators, and the scalar numpy statement of the two kernels of csrc/uad_batch.hip -- boxes by
np.argwhere (trainers/CE.py:124-126 of the reference), masking by batch * mask (:139), noise by oracle.rng.normal."""
import numpy as np

from oracle import rng as orng

# H*W below (4), at no multiple of (60, 780) and at a multiple of (4096, 16384) the workgroup size of 256; 6x10 and 26x30 have W % 4 != 0
BOX_SHAPES = [(1, 4), (6, 10), (26, 30), (64, 64), (128, 128)]
# 26x30x1 and 24x28x1: windows start at columns of every residue mod 4; 26x30: a 16-byte vector straddles a row end (30 % 4 != 0)
ASM_SHAPES = [(26, 30, 1), (24, 28, 1), (64, 64, 1), (32, 32, 2)]
NOISE_TOL = 4e-6                                  # tests/test_gpu_rng.py: logf / sincosf differ from libm in the last ulps


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- boxes
def box_patterns(shape, seed=0):
    """{name: bool [H,W]}: a single pixel at each corner and in the centre, the full slice, one row, one column, nothing, random blobs."""
    H, W = shape
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((H, W), bool)
    out = {}
    for name, (r, c) in {'tl': (0, 0), 'tr': (0, W - 1), 'bl': (H - 1, 0), 'br': (H - 1, W - 1), 'centre': (H // 2, W // 2)}.items():
        out[name] = z()
        out[name][r, c] = True
    out['full'] = ~z()
    out['row'] = z()
    out['row'][H // 3] = True
    out['col'] = z()
    out['col'][:, (2 * W) // 3] = True
    out['empty'] = z()
    for k in range(3):
        m = z()
        for _ in range(1 + k):
            r, c = int(rng.integers(0, H)), int(rng.integers(0, W))
            h, w = int(rng.integers(1, max(2, H // 2))), int(rng.integers(1, max(2, W // 2)))
            m[r:r + h, c:c + w] |= rng.random((H, W))[r:r + h, c:c + w] < 0.7
        out[f'blob{k}'] = m
    return out


def mask_stack(shape, seed=0):
    p = box_patterns(shape, seed)
    return list(p), np.stack([p[k] for k in p])


def label_store(shape, lut_kind, seed=0):
    """-> (labels u8 [n,H,W], lut u8 [256] or None, set bool [n,H,W]).  lut_kind None: LUT NULL, a pixel is set where its label is non-zero;
    'brain': utils.slice_cache's brain-mask LUT; 'random': a random 0/1 table under which label 0 is SET and some non-zero labels are not."""
    _, want = mask_stack(shape, seed)
    rng = np.random.default_rng(seed + 1)
    if lut_kind is None:
        lut, eff = None, (np.arange(256) != 0)
    elif lut_kind == 'brain':
        lut = np.ones(256, np.uint8)
        lut[[0, 4, 5, 6, 7, 9]] = 0
        eff = lut != 0
    else:
        lut = (rng.random(256) < 0.5).astype(np.uint8)
        lut[0], lut[1], lut[255] = 1, 0, 1
        eff = lut != 0
    on, off = np.flatnonzero(eff).astype(np.uint8), np.flatnonzero(~eff).astype(np.uint8)
    labels = np.where(want, rng.choice(on, want.shape), rng.choice(off, want.shape)).astype(np.uint8)
    return labels, lut, want


def f32_masks(shape, seed=0):
    """-> (masks fp32 [n,H,W], set bool [n,H,W]): a set pixel is any non-zero word -- 1, a negative, a denormal, inf, NaN; a clear one is +0 or -0."""
    _, want = mask_stack(shape, seed)
    rng = np.random.default_rng(seed + 2)
    on = np.array([1.0, -2.5, 1e-42, np.inf, np.nan, 0.25], np.float32)
    off = np.array([0.0, -0.0], np.float32)
    return np.where(want, rng.choice(on, want.shape), rng.choice(off, want.shape)).astype(np.float32), want


def boxes_reference(set_):
    """int32 [n,4] (row_min, row_max, col_min, col_max) by np.argwhere; (-1,-1,-1,-1) for an empty slice."""
    out = np.full((len(set_), 4), -1, np.int32)
    for i, m in enumerate(set_):
        at = np.argwhere(m)
        if len(at):
            out[i] = (at[:, 0].min(), at[:, 0].max(), at[:, 1].min(), at[:, 1].max())
    return out


# ---------------------------------------------------------------------------------------------------------------- assemble
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, -1e-42, -3.5, 1e30], np.float32)


def source(N, shape, seed=0, special=True):
    """fp32 [N,H,W,C] of N(0,1) values (half of them negative); with special, a fifth of the elements are +-0, +-inf, NaN (one of them with
    a payload), denormals -- spread everywhere, so also under every window."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N,) + tuple(shape)).astype(np.float32)
    if special:
        pick = rng.random(a.shape) < 0.2
        a[pick] = rng.choice(SPECIALS, int(pick.sum()))
        a.reshape(-1).view(np.uint32)[5] = 0x7FC12345               # a quiet NaN with a payload
    return a


def index_case(kind, N, n, seed=0):
    rng = np.random.default_rng(seed + 3)
    if kind is None:
        return None
    if kind == 'perm':
        return rng.permutation(N)[:n].astype(np.int32)
    return rng.integers(0, max(1, N // 2), n).astype(np.int32)      # repeats


def _fixed_windows(H, W):
    """Per-sample window lists that name every edge case: one window at each column residue mod 4, three windows with an overlap, windows
    flush with each slice edge."""
    s = min(20, H - 4, W - 4)
    return [
        [(1, 1, 5, 7)],                                               # column residue 1
        [(0, 0, 4, 4), (H - 6, W - 5, 6, 5), (2, 2, 9, 9)],           # flush top-left, flush bottom-right, overlapping the first
        [(3, 2, s, s)],                                               # residue 2, the trainers' square where it fits
        [(0, W - 9, 3, 9), (H - 3, 0, 3, 6)],                         # residue 3 (W % 4 == 0) or 1, flush right / top; flush left / bottom
        [(5, 4, 3, 8)],                                               # residue 0
        [(H // 2, 3, 1, W - 3)],                                      # one row up to the row end: the vector straddling the row end is split
        [(4, 7, 6, 2), (4, 9, 6, 2), (9, 7, 3, 4)],                   # residue 3; abutting and overlapping
    ]


def rects_case(kind, n, shape, seed=0):
    """int32 [n,3,4] of (row, col, height, width), height 0 = unused.  'none': no window anywhere (the named no-window case); 'mixed': the
    fixed lists in turn, then random windows, with one sample in four of a batch of 8 or more left without a window."""
    H, W = shape[0], shape[1]
    r = np.zeros((n, 3, 4), np.int32)
    if kind == 'none':
        return r
    fixed = _fixed_windows(H, W)
    rng = np.random.default_rng(seed + 4)
    for b in range(n):
        if b < len(fixed):
            wins = fixed[(b + 1) % len(fixed)] if n <= 3 else fixed[b]      # n = 1 takes the three-window list
        elif n >= 8 and b % 4 == 3:
            wins = []
        else:
            wins = []
            for _ in range(int(rng.integers(1, 4))):
                h, w = int(rng.integers(1, H // 2)), int(rng.integers(1, W // 2))
                wins.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
        for k, win in enumerate(wins):
            r[b, k] = win
    return r


def rect_masks(rects, shape):
    """fp32 [n,H,W,C]: 0 inside any window of the sample (all channels), 1 elsewhere."""
    m = np.ones((len(rects),) + tuple(shape), np.float32)
    for b, wins in enumerate(np.asarray(rects).tolist()):
        for r, c, h, w in wins:
            if h:
                m[b, r:r + h, c:c + w] = 0
    return m


def noise_reference(n, shape, noise):
    sigma, seed, step, sample0, stream = noise
    return orng.normal(n, int(np.prod(shape)), seed, step, sample0, stream).reshape((n,) + tuple(shape))


def assemble_reference(src, idx, rects, noise=None):
    """The statement: x = src[idx] (+ sigma * normal, fp32 multiply then fp32 add), x_ce = x * mask.  -> (x, x_ce or None, mask or None)."""
    x = src if idx is None else src[np.asarray(idx)]
    if noise is not None and noise[0] != 0:
        with np.errstate(invalid='ignore', over='ignore'):
            x = x + np.float32(noise[0]) * noise_reference(len(x), src.shape[1:], noise)
    if rects is None:
        return x.astype(np.float32), None, None
    mask = rect_masks(rects, src.shape[1:])
    with np.errstate(invalid='ignore'):
        return x.astype(np.float32), (x * mask).astype(np.float32), mask


def masks_something(rects, shape):
    """The condition on a masking case: at least one pixel zeroed and at least one left untouched."""
    m = rect_masks(rects, shape)
    return bool((m == 0).any() and (m == 1).any())


def noise_bound(x, ref, sigma):
    """|out - (x + sigma * ref)| <= sigma * 4e-6 * max(1, max|ref|) + ulp(x): the generator's tolerance scaled by sigma, plus one ulp of |x| for
    the rounding of the sum (elementwise)."""
    return np.float64(sigma) * NOISE_TOL * max(1.0, float(np.abs(ref).max())) + np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
