"""Shared by tests/test_crops_host.py (CPU, the host statement utils/crops.py), tests/test_crops_kernels_host.py (CPU, the kernel source
compiled for the host) and tests/test_gpu_crops.py (the device): the volumes, batches and windows the component measurements and the crop
gather are held on, the label model of uad_cc_label (that of tests/test_gpu_lesionwise.py::expected_labels), literal restatements of the
reference lines (dataloaders/MSLUB.py:200-222, BRAINWEB.py:166-173) and the phantom of the ingestion tests.  Computed once per case and cached;
callers must not write into what they get.

PROPS_SHAPES straddle the 32 x 8 x 4 labelling tile of csrc/uad_cc.hip and the 1024-voxel tile of csrc/uad_crops.hip: 35 voxels; 256 (one wave
row of a tile, a quarter of it); 297; 9805 (ten tiles, the last partial); 65536 (64 full tiles); 10080."""
import functools

import numpy as np
import scipy.ndimage

from unsupervised_anomaly_detection_brain_mri_amd.utils import crops

FULL = np.ones((3, 3, 3), bool)
PROPS_SHAPES = [(1, 7, 5), (1, 8, 32), (1, 9, 33), (5, 37, 53), (4, 128, 128), (9, 16, 70)]
FILLS = (0.02, 0.30)
SLABS = (0, 1, 2)
KINDS = ('fill2', 'fill30', 'chain')
SPAN_SHAPE = (5, 37, 53)


def shape_id(s):
    return '%dx%dx%d' % tuple(s)


def blobs(rng, shape, fill):
    """Smooth random blobs at about `fill` foreground (tests/test_gpu_lesionwise.py)."""
    f = scipy.ndimage.uniform_filter(rng.random(shape).astype(np.float32), 3, mode='constant')
    return f > np.quantile(f, 1.0 - fill)


def diagonal_chain(shape):
    """One voxel per step along the long diagonal, every coordinate moving by at most 1: 8- / 26-connected, never 4- / 6-connected throughout."""
    v = np.zeros(shape, bool)
    T = max(shape)
    t = np.arange(T)
    z, y, x = (np.round(t * (s - 1) / max(T - 1, 1)).astype(int) for s in shape)
    v[z, y, x] = True
    return v


@functools.lru_cache(maxsize=None)
def mask(shape, kind):
    """bool [D,H,W].  fill2 / fill30: random blobs; chain: the diagonal chain; span: one component that visits every 32 x 8 x 4 labelling
    tile and every 1024-voxel tile (every fourth row, joined at alternating ends: a serpentine through each slice, the same in every slice);
    corner: two squares that touch at one corner (one 8-connected component), a diagonal pair and a pixel two rows off; full: one full slice between empty ones; empty."""
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2] + len(kind))
    if kind in ('fill2', 'fill30'):
        m = blobs(rng, shape, 0.02 if kind == 'fill2' else 0.30)
    elif kind == 'chain':
        m = diagonal_chain(shape)
    elif kind == 'span':
        m = np.zeros(shape, bool)
        m[:, ::4, :] = True
        for i, y in enumerate(range(0, shape[1] - 4, 4)):
            m[:, y:y + 5, -1 if i % 2 == 0 else 0] = True
    elif kind == 'corner':
        m = np.zeros(shape, bool)
        m[0, :3, :3] = True
        m[0, 3:5, 3:5] = True                                   # (2,2) and (3,3) touch at a corner: joined
        m[-1, 0, 0] = True
        m[-1, 1, 1] = True
        m[-1, 3, 0] = True                                      # two rows down: its own component
    elif kind == 'full':
        m = np.zeros(shape, bool)
        m[shape[0] // 2] = True
    elif kind == 'empty':
        m = np.zeros(shape, bool)
    else:
        raise KeyError(kind)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def labels_model(shape, kind, slab=0):
    """What uad_cc_label returns for mask(shape, kind): 1 + the smallest linear index of the voxel's scipy component, slab by slab (int32)."""
    m = mask(shape, kind)
    D = m.shape[0]
    step = D if slab <= 0 or slab >= D else slab
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    out = np.zeros(m.shape, np.int32)
    for s0 in range(0, D, step):
        lab, n = scipy.ndimage.label(m[s0:s0 + step], structure=FULL)
        if n:
            mins = np.asarray(scipy.ndimage.minimum(idx[s0:s0 + step], lab, index=np.arange(1, n + 1))).astype(np.int64)
            out[s0:s0 + step] = np.where(lab > 0, mins[np.maximum(lab, 1) - 1] + 1, 0)
    out.setflags(write=False)
    return out


def props_loop(m, slab=0):
    """The literal form of component_props: np.argwhere per scipy label, one Python row per component, sorted by the first index."""
    m = np.asarray(m) != 0
    D, H, W = m.shape
    step = D if slab <= 0 or slab >= D else slab
    rows = []
    for s0 in range(0, D, step):
        lab, n = scipy.ndimage.label(m[s0:s0 + step], structure=FULL)
        for i in range(1, n + 1):
            c = np.argwhere(lab == i)
            c[:, 0] += s0
            lin = (c[:, 0] * H + c[:, 1]) * W + c[:, 2]
            rows.append([int(lin.min()), len(c), int(c[:, 0].sum()), int(c[:, 1].sum()), int(c[:, 2].sum())])
    rows.sort()
    return np.array(rows, np.int64).reshape(-1, 5)


@functools.lru_cache(maxsize=None)
def props_reference(shape, kind, slab=0):
    """The host statement on mask(shape, kind), once (tests/test_crops_host.py pins it against props_loop)."""
    p = crops.component_props(mask(shape, kind), slab)
    p.setflags(write=False)
    return p


# ---------------------------------------------------------------------------------------------------------------- the window gather
CROP_BATCH = (7, 66, 72)             # n, H, W: the full-slice window has a width that is a multiple of four
CROP_SIZES = [(1, 1), (3, 5), (64, 64), (66, 72)]      # (crop_h, crop_w): single words, a quad and a tail, 16-byte stores, the whole slice
CROP_SLICES = [3, 0, 6, 3, 5, 1, 3]  # non-monotone, one slice three times


@functools.lru_cache(maxsize=None)
def crop_batch():
    """[7,66,72] float32 of ordinary values with +-0, denormals, +-1e30, inf and NaNs with payloads (quiet and signalling) spread through it."""
    rng = np.random.default_rng(66)
    a = rng.standard_normal(CROP_BATCH).astype(np.float32)
    pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x000b8ad6, 0x7149f2ca, 0xf149f2ca, 0x7f800000, 0x7fc00000, 0x7fc12345, 0xffc00001,
                     0x7f812345], np.uint32)
    u = a.view(np.uint32).copy()
    hit = rng.random(CROP_BATCH) < 0.3
    u[hit] = pool[rng.integers(0, pool.size, int(hit.sum()))]
    out = u.view(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def crop_origins(size):
    """int32 [7,3] for a (crop_h, crop_w) window in CROP_BATCH: the slices of CROP_SLICES, `left` at every residue mod 4 (0, 1, 2, 3, then the
    largest origin, then 5 and 6) where the width leaves room, `top` from 0 to the largest."""
    ch, cw = size
    n, H, W = CROP_BATCH
    tops = [0, 1, H - ch, 2, 0, H - ch, 1]
    lefts = [0, 1, 2, 3, W - cw, 5, 6]
    o = np.array([[s, min(t, H - ch), min(l, W - cw)] for s, t, l in zip(CROP_SLICES, tops, lefts)], np.int32)
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def crop_reference(size):
    r = crops.crop_windows(crop_batch(), crop_origins(size), size[0], size[1])
    r.setflags(write=False)
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- the reference lines
def reference_lesion_crops(slice_data, slice_seg, crop_w, crop_h):
    """dataloaders/MSLUB.py:200-222 on one slice, in the reference's own floats: label (8-connectivity), regionprops in label order (raster
    order of the first pixel), prop['centroid'] = the mean of the pixel coordinates, the four float clamps, int(), crop(), the shape check.
    -> [(image_crop, seg_crop)]."""
    lab, n = scipy.ndimage.label(np.asarray(slice_seg) != 0, structure=np.ones((3, 3), bool))
    comps = sorted((np.argwhere(lab == i) for i in range(1, n + 1)), key=lambda c: (c[0][0], c[0][1]))      # argwhere is raster-ordered: c[0] is the first pixel
    out = []
    for c in comps:
        centroid = c.mean(axis=0)
        cx = centroid[1]
        cy = centroid[0]
        if cy < crop_h // 2:
            cy = crop_h // 2
        if cy > (slice_data.shape[0] - (crop_h // 2)):
            cy = (slice_data.shape[0] - (crop_h // 2))
        if cx < crop_w // 2:
            cx = crop_w // 2
        if cx > (slice_data.shape[1] - (crop_w // 2)):
            cx = (slice_data.shape[1] - (crop_w // 2))
        y, x = int(cy) - (crop_h // 2), int(cx) - (crop_w // 2)
        image_crop = slice_data[y:y + crop_h, x:x + crop_w]
        seg_crop = slice_seg[y:y + crop_h, x:x + crop_w]
        if image_crop.shape[0] != crop_h or image_crop.shape[1] != crop_w:
            continue
        out.append((image_crop, seg_crop, (y, x)))
    return out


def crops_loop(images, labels, kept, spec, rng=None):
    """The crop step of the reference's slice loop, slice by slice, on the UNCROPPED output (images, labels, kept) of volume_to_slices (which
    the existing tests pin): spec = ('center', w, h) | ('lesions', w, h) | ('random', w, h, per_slice).  'random' crops the label map at the
    image's origins (the package's stated deviation from BRAINWEB.py:173).  -> (images, labels, kept)."""
    from unsupervised_anomaly_detection_brain_mri_amd.utils.nifti import crop_center
    mode, w, h = spec[:3]
    oi, ol, ok = [], [], []
    for sd, ss, s in zip(images, labels, kept):
        if mode == 'center':
            oi.append(crop_center(sd, w, h)); ol.append(crop_center(ss, w, h)); ok.append(s)
        elif mode == 'lesions':
            for ic, sc, _ in reference_lesion_crops(sd, ss, w, h):
                oi.append(ic); ol.append(sc); ok.append(s)
        else:
            rx = rng.randint(0, high=(sd.shape[1] - w), size=spec[3])
            ry = rng.randint(0, high=(sd.shape[0] - h), size=spec[3])
            for r in range(spec[3]):
                oi.append(sd[ry[r]:ry[r] + h, rx[r]:rx[r] + w]); ol.append(ss[ry[r]:ry[r] + h, rx[r]:rx[r] + w]); ok.append(s)
    if not oi:
        return np.zeros((0, h, w), np.float32), np.zeros((0, h, w), np.float32), []
    return np.stack(oi).astype(np.float32), np.stack(ol).astype(np.float32), ok


# ---------------------------------------------------------------------------------------------------------------- the ingestion phantom
PHANTOM_SHAPE = (12, 40, 44)


@functools.lru_cache(maxsize=None)
def phantom(seed=0):
    """(vol float64, seg {0,1}, brainmask {0,1}, tissue uint8) of shape 12 x 40 x 44 for both loaders.  Lesions sit in the interior, on each
    of the four borders and in a corner, several per slice, one spanning slices; slices 0 and 1 have none; slice 11 is empty (dropped by both
    loaders' slice filters).  tissue: the BrainWeb classes with 10 where seg is set, 2 (GM) elsewhere: nothing is masked away, so the lesion
    map of loader='brainweb' is seg."""
    rng = np.random.default_rng(seed)
    D, H, W = PHANTOM_SHAPE
    vol = 100.0 + 50.0 * rng.random(PHANTOM_SHAPE)
    seg = np.zeros(PHANTOM_SHAPE, np.float64)
    seg[2:5, 0:3, 10:14] = 1                                     # top border
    seg[2:4, 37:40, 20:23] = 1                                   # bottom border
    seg[3:6, 15:19, 0:2] = 1                                     # left border
    seg[3:6, 20:22, 41:44] = 1                                   # right border
    seg[5:8, 38:40, 42:44] = 1                                   # bottom-right corner
    seg[6:9, 18:23, 18:24] = 1                                   # interior
    seg[6, 19, 30] = seg[6, 20, 31] = seg[6, 21, 30] = 1         # a diagonal chain: one 8-connected component
    seg[9, 5, 5] = 1                                             # one pixel
    seg[10, 10:13, 10:12] = seg[10, 30:32, 30:35] = 1
    vol += 80.0 * seg
    vol[11] = 0.0
    brainmask = np.ones(PHANTOM_SHAPE, np.float64)
    tissue = np.where(seg > 0, 10, 2).astype(np.uint8)
    for a in (vol, seg, brainmask, tissue):
        a.setflags(write=False)
    return vol, seg, brainmask, tissue


def loader_inputs(loader, seed=0):
    """-> (positional arguments of volume_to_slices, keywords) for the phantom."""
    vol, seg, brainmask, tissue = phantom(seed)
    if loader == 'brainweb':
        return (vol, tissue), dict(loader='brainweb', slice_start=0, slice_end=155)
    return (vol, seg, brainmask), dict(slice_start=0, slice_end=155)
