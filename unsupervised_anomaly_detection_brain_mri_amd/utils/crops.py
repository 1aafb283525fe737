"""The crop modes of the reference's dataset classes (`useCrops`) beyond cropType 'center': per-component measurements of a label volume, the
lesion-centred crop windows built on them and the random crop windows, as the host statement the device ops (csrc/uad_crops.hip:
uad_cc_props, uad_crop2d) are held to.

cropType 'lesions' (dataloaders/MSLUB.py:200-222, the same lines in MSISBI2015.py / MSSEG2008.py): `skimage.measure.label` of the label slice
(8-connectivity on a 2-D array), `regionprops`, and one crop per component centred on its centroid, the centre clamped so that the window
starts inside the slice; a window that still leaves the slice is dropped by the shape check (:219-220).
cropType 'random' (dataloaders/BRAINWEB.py:166-173): `numRandomCropsPerSlice` windows per slice whose corners come from two
`numpy.random.randint` calls.

Plain numpy and scipy.  skimage is not installed here: the labelling is scipy.ndimage.label with the full 3x3x3 structure (inside one slice
that is 8-connectivity) and the measurements are written down from what `regionprops` documents -- label order = raster order of a
component's first pixel, centroid = the mean of its pixel coordinates.  This statement has NOT been compared with skimage's own output.

Everything is integer arithmetic: a component is (first, area, sum_z, sum_y, sum_x), and the crop origin is formed from the FLOORED centroid
sum // area.  The reference clamps the float centroid and then takes int(); for integer bounds and non-negative coordinates the two agree
(tests/test_crops_host.py holds that against a literal float restatement of the reference lines)."""
import numpy as np

PROPS_COLUMNS = ('first', 'area', 'sum_z', 'sum_y', 'sum_x')
_FULL = np.ones((3, 3, 3), bool)


def component_props(labels_or_mask, slab=0):
    """[D,H,W] volume (non-zero = foreground: a binary mask, or a label volume of the same `slab`) -> int64 [K,5], one row per 26-connected
    component: first (its smallest linear index (z*H + y)*W + x), area, sum_z, sum_y, sum_x (sums of its voxel coordinates).
    slab: groups of `slab` consecutive slices are labelled independently (<= 0 or >= D: the whole volume), the model of
    tests/test_gpu_lesionwise.py::expected_labels; slab = 1 labels every slice on its own, which is skimage.measure.label of a 2-D slice.
    Rows are ordered by `first`, ascending: slice-major for slab = 1, and inside a slice regionprops' order."""
    from scipy.ndimage import label
    mask = np.asarray(labels_or_mask) != 0
    if mask.ndim != 3:
        raise ValueError(f'component_props expects a [D,H,W] volume, got {mask.shape}')
    D, H, W = mask.shape
    slab = D if slab <= 0 or slab >= D else int(slab)
    rows = []
    for s0 in range(0, D, slab):
        lab, n = label(mask[s0:s0 + slab], structure=_FULL)
        if n == 0:
            continue
        idx = np.flatnonzero(lab).astype(np.int64)                  # ascending linear index inside the group
        comp = lab.ravel()[idx].astype(np.int64) - 1
        lin = idx + s0 * H * W
        z, rem = np.divmod(lin, H * W)
        y, x = np.divmod(rem, W)
        p = np.zeros((n, 5), np.int64)
        p[:, 0] = np.iinfo(np.int64).max
        np.minimum.at(p[:, 0], comp, lin)
        np.add.at(p[:, 1], comp, 1)
        np.add.at(p[:, 2], comp, z)
        np.add.at(p[:, 3], comp, y)
        np.add.at(p[:, 4], comp, x)
        rows.append(p[np.argsort(p[:, 0], kind='stable')])
    return np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)


def _check_window(H, W, crop_w, crop_h):
    H, W, crop_w, crop_h = int(H), int(W), int(crop_w), int(crop_h)
    if crop_w < 1 or crop_h < 1:
        raise ValueError(f'crop size must be positive, got {crop_w} x {crop_h} (width x height)')
    return H, W, crop_w, crop_h


def lesion_crop_origins(props, H, W, crop_w, crop_h):
    """MSLUB.py:203-220 in integers.  props: component_props(label_batch, slab=1) of an [n,H,W] batch -> int32 [k,3] of (slice, top, left),
    one row per component whose window lies inside the slice, in the order of `props`.
    cy = sum_y // area, cx = sum_x // area; cy is clamped to [crop_h//2, H - crop_h//2], cx to [crop_w//2, W - crop_w//2]; top = cy - crop_h//2,
    left = cx - crop_w//2.  A window that leaves the slice is dropped (the reference's shape check): with an odd size that is the case
    exactly when the centre sits on the upper bound (top + crop_h = H + 1); with an even size never.  crop_w > W or crop_h > H raises
    ValueError (the reference yields no crop there)."""
    H, W, crop_w, crop_h = _check_window(H, W, crop_w, crop_h)
    if crop_w > W or crop_h > H:
        raise ValueError(f'crop {crop_h} x {crop_w} (height x width) is larger than the slice {H} x {W}')
    p = np.asarray(props, np.int64).reshape(-1, 5)
    if p.shape[0] == 0:
        return np.zeros((0, 3), np.int32)
    s = p[:, 0] // (H * W)
    cy = np.clip(p[:, 3] // p[:, 1], crop_h // 2, H - crop_h // 2)
    cx = np.clip(p[:, 4] // p[:, 1], crop_w // 2, W - crop_w // 2)
    top, left = cy - crop_h // 2, cx - crop_w // 2
    inside = (top + crop_h <= H) & (left + crop_w <= W)
    return np.stack([s, top, left], axis=1)[inside].astype(np.int32)


def random_crop_origins(n_slices, H, W, crop_w, crop_h, per_slice, rng=None):
    """BRAINWEB.py:167-171: per slice rx = rng.randint(0, high=W - crop_w, size=per_slice), then ry = rng.randint(0, high=H - crop_h,
    size=per_slice) -> int32 [n_slices * per_slice, 3] of (slice, ry[r], rx[r]).  rng: a numpy.random.RandomState, or the numpy.random module
    (the default, as the reference), so that a seeded legacy stream gives the reference's draws.  `high` is exclusive: the last row and
    column of origins are never drawn, as in the reference.  W - crop_w <= 0 or H - crop_h <= 0 raises ValueError."""
    H, W, crop_w, crop_h = _check_window(H, W, crop_w, crop_h)
    if W - crop_w <= 0 or H - crop_h <= 0:
        raise ValueError(f'random crops of {crop_h} x {crop_w} (height x width) need a larger slice than {H} x {W}: randint(0, high <= 0)')
    if per_slice < 0 or n_slices < 0:
        raise ValueError('n_slices and per_slice must not be negative')
    rng = np.random if rng is None else rng
    out = np.zeros((int(n_slices) * int(per_slice), 3), np.int32)
    for s in range(int(n_slices)):
        rx = rng.randint(0, high=W - crop_w, size=per_slice)
        ry = rng.randint(0, high=H - crop_h, size=per_slice)
        rows = out[s * per_slice:(s + 1) * per_slice]
        rows[:, 0], rows[:, 1], rows[:, 2] = s, ry, rx
    return out


def check_origins(origins, n, H, W, crop_h, crop_w):
    """-> int32 [k,3]; ValueError unless every (slice, top, left) names a slice of the batch and a window inside it."""
    o = np.asarray(origins)
    if o.size == 0:
        return np.zeros((0, 3), np.int32)
    if o.ndim != 2 or o.shape[1] != 3 or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f'origins must be an integer [k,3] array of (slice, top, left), got shape {o.shape} dtype {o.dtype}')
    o = o.astype(np.int64)
    if crop_h < 1 or crop_w < 1 or crop_h > H or crop_w > W:
        raise ValueError(f'crop {crop_h} x {crop_w} does not fit a {H} x {W} slice')
    if o[:, 0].min() < 0 or o[:, 0].max() >= n:
        raise ValueError(f'origin slices must lie in [0, {n})')
    if o[:, 1].min() < 0 or (o[:, 1] + crop_h).max() > H or o[:, 2].min() < 0 or (o[:, 2] + crop_w).max() > W:
        raise ValueError(f'a {crop_h} x {crop_w} window leaves the {H} x {W} slice')
    return o.astype(np.int32)


def crop_windows(batch, origins, crop_h, crop_w):
    """image_utils.crop (img[y:y + height, x:x + width]) of slice origins[j][0] of an [n,H,W] batch at (top, left) = origins[j][1:] ->
    [k,crop_h,crop_w] of the batch's dtype; the values are copied."""
    b = np.asarray(batch)
    if b.ndim != 3:
        raise ValueError(f'batch must be [n,H,W], got {b.shape}')
    o = check_origins(origins, b.shape[0], b.shape[1], b.shape[2], int(crop_h), int(crop_w))
    out = np.empty((o.shape[0], int(crop_h), int(crop_w)), b.dtype)
    for j, (s, t, l) in enumerate(o):
        out[j] = b[s, t:t + crop_h, l:l + crop_w]
    return out
