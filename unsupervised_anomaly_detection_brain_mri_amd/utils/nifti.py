"""NIfTI-1 volumes without SimpleITK / nibabel, and the volume -> slice-cache pipeline of the reference's dataset classes.

`read_nifti` parses the 348-byte NIfTI-1 header (`.nii`, `.nii.gz`; single-file, little- or big-endian) and returns the voxel array in the
index order the reference sees: utils/NII.py reads with SimpleITK and takes `sitk.GetArrayFromImage`, i.e. [z, y, x] (the file's x runs
fastest), with `scl_slope * v + scl_inter` applied when the header asks for it and NaNs set to 0 (NII.py:12-16).

`volume_to_slices` restates what dataloaders/MSLUB.py:146-196,247-275 (and its siblings MSISBI2015 / MSSEG2008 / BRAINWEB) do to one volume:
binarise the brain mask at 0.1 and multiply (skull stripping, NII.py:75-81), clamp to the [0, 99.8] percentiles and scale by the maximum
(`normalize('scaling', 0, 99.8)`, NII.py:50-70), walk the slices `sliceStart .. sliceEnd` of the chosen view, drop the "empty" ones
(90th percentile < 0.2, MSLUB.py:161), zero-pad to and `scipy.ndimage.zoom` onto `sliceResolution`, binarise the label slice at 0.9.
`nii.denoise()` (SimpleITK's CurvatureFlow, three iterations of time step 0.125; NII.py:85-87, called before skull stripping by MSLUB.py:242,
MSISBI2015.py:231, MSSEG2008.py:241,246) is the keyword `curvature_flow` of `volume_to_slices`: utils/curvature_flow.py states ITK's update
from its source, and csrc/uad_flow.hip runs the same arithmetic on the device with the same bits.  That statement has not been compared with
SimpleITK's own output yet, which is why `denoise=True` still raises and the filter has a keyword of its own.

`volume_to_slices(loader='brainweb')` restates the training set's preparation instead (dataloaders/BRAINWEB.py:125-185, 266-292): one
tissue-class map for the skull map and the lesion map, the constant-slice filter, `cv2.resize` (utils/resize.py; csrc/uad_resize.hip on the
device) for slices larger than `sliceResolution` and zero padding otherwise.

`volume_to_slices(crops=...)` adds the reference's crop modes (`useCrops`: cropType 'center' | 'lesions' | 'random'; MSLUB.py:186-222,
BRAINWEB.py:165-180): utils/crops.py states the component measurements and the window arithmetic, csrc/uad_crops.hip runs them on the device.

`volume_to_slices(normalization='standardization')` takes NII.normalize's other method (NII.py:53-75; the default the reference's loaders
declare, while its configurations use 'scaling') in the place of the scaling: utils/standardize.py states it -- three fp64 sums in a defined
order, each scalar rounded to float32 once --, csrc/uad_moments.hip runs it on the device with the same bits.

`build_cache` turns a list of patients into the slice cache of utils/slice_cache.py with the reference's patient-level TRAIN / VAL / TEST
partition (a permutation of the patients cut at floor(fraction * n), MSLUB.py:71-90)."""
import gzip
import math
import struct

import numpy as np

_DTYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4', 1024: 'i8', 1280: 'u8'}
VIEW_MAPPING = {'saggital': 2, 'coronal': 1, 'axial': 0}          # dataset Options.viewMapping (MSLUB.py:53) on the [z, y, x] array


def read_nifti(path):
    """-> (data [z,y,x] float64, header dict with dim, pixdim, datatype, vox_offset, scl_slope, scl_inter)."""
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(path, 'rb') as f:
        raw = f.read()
    if len(raw) < 352:
        raise ValueError(f'{path}: too short for a NIfTI-1 file')
    end = '<'
    if struct.unpack('<i', raw[:4])[0] != 348:
        end = '>'
        if struct.unpack('>i', raw[:4])[0] != 348:
            raise ValueError(f'{path}: sizeof_hdr is not 348 (not NIfTI-1)')
    magic = raw[344:348]
    if magic not in (b'n+1\x00', b'ni1\x00'):
        raise ValueError(f'{path}: bad NIfTI magic {magic!r}')
    if magic == b'ni1\x00':
        raise ValueError(f'{path}: two-file NIfTI (.hdr / .img) is not supported')
    dim = struct.unpack(end + '8h', raw[40:56])
    datatype, bitpix = struct.unpack(end + '2h', raw[70:74])
    pixdim = struct.unpack(end + '8f', raw[76:108])
    vox_offset, slope, inter = struct.unpack(end + '3f', raw[108:120])
    if datatype not in _DTYPES:
        raise ValueError(f'{path}: unsupported NIfTI datatype {datatype}')
    nd = dim[0]
    if nd < 3 or nd > 4 or (nd == 4 and dim[4] != 1):
        raise ValueError(f'{path}: expected a 3-D volume, header dim = {dim}')
    nx, ny, nz = dim[1:4]
    dt = np.dtype(end + _DTYPES[datatype])
    off = int(vox_offset) if vox_offset >= 352 else 352
    cnt = nx * ny * nz
    if len(raw) < off + cnt * dt.itemsize:
        raise ValueError(f'{path}: voxel data is truncated')
    data = np.frombuffer(raw, dt, cnt, off).reshape(nz, ny, nx).astype(np.float64)      # x fastest in the file = the [z,y,x] C array
    if slope != 0.0 and not (slope == 1.0 and inter == 0.0):
        data = data * slope + inter
    data[np.isnan(data)] = 0
    return data, dict(dim=dim, pixdim=pixdim, datatype=datatype, bitpix=bitpix, vox_offset=off, scl_slope=slope, scl_inter=inter, endian=end)


def write_nifti(path, data_zyx, dtype='f4', pixdim=(1.0, 1.0, 1.0)):
    """Minimal single-file NIfTI-1 writer (tests, exporting results)."""
    a = np.asarray(data_zyx)
    nz, ny, nx = a.shape
    code = {v: k for k, v in _DTYPES.items()}[np.dtype(dtype).str[1:]]
    hdr = bytearray(348)
    struct.pack_into('<i', hdr, 0, 348)
    struct.pack_into('<8h', hdr, 40, 3, nx, ny, nz, 1, 1, 1, 1)
    struct.pack_into('<2h', hdr, 70, code, np.dtype(dtype).itemsize * 8)
    struct.pack_into('<8f', hdr, 76, 1.0, pixdim[0], pixdim[1], pixdim[2], 0, 0, 0, 0)
    struct.pack_into('<3f', hdr, 108, 352.0, 1.0, 0.0)
    hdr[344:348] = b'n+1\x00'
    payload = bytes(hdr) + b'\x00' * 4 + np.ascontiguousarray(a, '<' + np.dtype(dtype).str[1:]).tobytes()
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(path, 'wb') as f:
        f.write(payload)


_NRRD_TYPES = {'signed char': 'i1', 'int8': 'i1', 'int8_t': 'i1', 'uchar': 'u1', 'unsigned char': 'u1', 'uint8': 'u1', 'uint8_t': 'u1',
               'short': 'i2', 'short int': 'i2', 'signed short': 'i2', 'int16': 'i2', 'int16_t': 'i2', 'ushort': 'u2', 'unsigned short': 'u2',
               'uint16': 'u2', 'uint16_t': 'u2', 'int': 'i4', 'signed int': 'i4', 'int32': 'i4', 'int32_t': 'i4', 'uint': 'u4', 'unsigned int': 'u4',
               'uint32': 'u4', 'uint32_t': 'u4', 'longlong': 'i8', 'long long': 'i8', 'int64': 'i8', 'int64_t': 'i8', 'ulonglong': 'u8',
               'unsigned long long': 'u8', 'uint64': 'u8', 'uint64_t': 'u8', 'float': 'f4', 'double': 'f8'}


def read_nrrd(path):
    """NRRD (attached header; encodings raw / gzip) -> (data, header dict) in the index order of `nrrd.read` that dataloaders/NRRD.py:11 relies
    on: shape = the header's `sizes` (first axis fastest, i.e. Fortran order)."""
    raw = open(path, 'rb').read()
    if not raw.startswith(b'NRRD'):
        raise ValueError(f'{path}: not an NRRD file')
    end = raw.find(b'\n\n')
    crlf = raw.find(b'\r\n\r\n')
    if crlf != -1 and (end == -1 or crlf < end):
        head, body = raw[:crlf], raw[crlf + 4:]
    elif end != -1:
        head, body = raw[:end], raw[end + 2:]
    else:
        raise ValueError(f'{path}: no header terminator')
    hdr = {}
    for line in head.decode('ascii', 'replace').splitlines()[1:]:
        if line.startswith('#') or ':' not in line:
            continue
        k, v = line.split(':', 1)
        hdr[k.strip().lower()] = v.lstrip('=').strip()
    if 'data file' in hdr or 'datafile' in hdr:
        raise ValueError(f'{path}: detached NRRD data files are not supported')
    t = hdr.get('type', '').lower()
    if t not in _NRRD_TYPES:
        raise ValueError(f'{path}: unsupported NRRD type {t!r}')
    sizes = [int(v) for v in hdr['sizes'].split()]
    enc = hdr.get('encoding', 'raw').lower()
    if enc in ('gzip', 'gz'):
        body = gzip.decompress(body)
    elif enc != 'raw':
        raise ValueError(f'{path}: unsupported NRRD encoding {enc!r}')
    dt = np.dtype(('>' if hdr.get('endian', 'little').lower() == 'big' else '<') + _NRRD_TYPES[t])
    cnt = int(np.prod(sizes))
    if len(body) < cnt * dt.itemsize:
        raise ValueError(f'{path}: NRRD data is truncated')
    return np.frombuffer(body, dt, cnt).reshape(sizes, order='F'), hdr


def _has_order_stats(engine):
    return engine is not None and all(hasattr(engine, op) for op in ('select_quantiles', 'clamp_scale', 'percentile'))


def _has_standardize(engine):
    return _has_order_stats(engine) and all(hasattr(engine, op) for op in ('shifted_sums', 'standardize'))


def _clamp_bounds_on(engine, v, lower, upper):
    """The percentile clamp of NII.normalize on an fp32 array resident with `engine`, without a sort: ONE select call brackets the lower
    percentile, the upper percentile and the maximum (q = {lower, upper, 1}).  Clamping is monotone, so the order statistics of the
    lower-clamped array are the clamped order statistics: the upper percentile is interpolated from the clamped brackets, exactly what
    np.percentile returns after `v[v < q] = q`.  -> (clamp_lo, clamp_hi, top): float32 bounds (None = no clamp) and the clamped maximum."""
    from .order_stats import finish_linear, percentile_fractions
    f32 = np.dtype(np.float32)
    ql = percentile_fractions(0 if lower is None else lower, f32)
    qu = percentile_fractions(100 if upper is None else upper, f32)
    m, lo, hi = engine.select_quantiles(v, [float(ql), float(qu), 1.0], [ql.dtype == np.float32, qu.dtype == np.float32, False])
    clamp_lo = clamp_hi = None
    top = np.float32(hi[0, 2])                                              # v.max()
    if lower is not None:
        clamp_lo = finish_linear(m, lo[:, 0], hi[:, 0], ql, f32)[0]
        lo, hi = np.where(lo < clamp_lo, clamp_lo, lo), np.where(hi < clamp_lo, clamp_lo, hi)
        top = clamp_lo if top < clamp_lo else top
    if upper is not None:
        clamp_hi = finish_linear(m, lo[:, 1], hi[:, 1], qu, f32)[0]
        top = clamp_hi if top > clamp_hi else top
    return clamp_lo, clamp_hi, top


def _normalize_scaling_on(engine, v, lower, upper):
    """normalize_scaling of an fp32 array resident with `engine` (engine._dev), without leaving the engine: the one select call of
    _clamp_bounds_on, then one clamp-and-scale pass.  NaN-free input."""
    clamp_lo, clamp_hi, top = _clamp_bounds_on(engine, v, lower, upper)
    scale = np.float32(1.0 / top) if top > 0.0 else np.float32(1.0)
    return engine.clamp_scale(v, clamp_lo, clamp_hi, scale)


def _normalize_standardization_on(engine, v, lower, upper):
    """normalize_standardization of an fp32 array resident with `engine`: the one select call of _clamp_bounds_on, then engine.standardize --
    three ordered-sum launches with a 16-byte download each and one clamp-and-standardize pass.  NaN-free input."""
    clamp_lo, clamp_hi, _ = _clamp_bounds_on(engine, v, lower, upper)
    return engine.standardize(v, clamp_lo, clamp_hi)


NORMALIZATIONS = ('scaling', 'standardization')         # NII.normalize's methods (NII.py:53-75)


def _normalization_setting(normalization):
    if normalization not in NORMALIZATIONS:
        raise ValueError(f"normalization must be 'scaling' or 'standardization', got {normalization!r}")
    return normalization


def normalize_scaling(vol, lower=0, upper=99.8, engine=None):
    """NII.normalize(method='scaling', lowerpercentile, upperpercentile) (NII.py:50-66).
    engine: an engine with the device order statistics (device_ops.DeviceOps.select_quantiles / clamp_scale): both percentiles and the maximum
    come from one device select call and the clamp-and-scale is one device pass; the same float32 array comes back.  The device path takes
    Python-scalar percentiles and NaN-free input (volume_to_slices zeroes NaNs first); an engine without the ops gets the host statement.
    Bit-equal to the host statement except for the SIGN of a zero that a zero-valued lower percentile clamps negative values to: numpy's
    comes out of its partition order, the op knows one zero (+0).  With lower = 0, the pipeline's setting, nothing is clamped from below."""
    if _has_order_stats(engine) and all(p is None or isinstance(p, (int, float)) for p in (lower, upper)):
        out = _normalize_scaling_on(engine, engine._dev(np.ascontiguousarray(vol, np.float32)), lower, upper)
        return out.cpu().numpy().reshape(np.shape(vol))
    v = vol.astype(np.float32)
    if lower is not None:
        q = np.percentile(v, lower); v[v < q] = q
    if upper is not None:
        q = np.percentile(v, upper); v[v > q] = q
    if v.max() > 0.0:
        v = v * np.float32(1.0 / v.max())
    return v


def normalize_standardization(vol, lower=0, upper=99.8, engine=None):
    """NII.normalize(method='standardization', lowerpercentile, upperpercentile) (NII.py:53-75): the percentile clamp of normalize_scaling, then
    c = v - mean(v) and c / std(c) in float32.  utils/standardize.py states it; its three sums are fp64 sums in a defined order, each scalar
    rounded to float32 once -- not numpy's float32 sums in numpy's own order (a stated deviation; DESIGN).  A constant volume gives NaN.
    engine: an engine with the order statistics and the ordered sums (device_ops.DeviceOps.select_quantiles / shifted_sums / standardize): one
    select call gives the clamp bounds, three sum launches and one map pass follow; the same float32 array comes back, bit for bit (but
    for the sign of a zero-valued lower clamp, as in normalize_scaling, which shows only where the mean is zero too).  Python-scalar
    percentiles and NaN-free input; an engine without the ops gets the host statement."""
    if _has_standardize(engine) and all(p is None or isinstance(p, (int, float)) for p in (lower, upper)):
        out = _normalize_standardization_on(engine, engine._dev(np.ascontiguousarray(vol, np.float32)), lower, upper)
        return out.cpu().numpy().reshape(np.shape(vol))
    from .standardize import standardize
    return standardize(vol, lower, upper)


def crop_center(img, cropx, cropy):
    """utils/image_utils.py:4-12."""
    y, x = img.shape[:2]
    sx, sy = x // 2 - cropx // 2, y // 2 - cropy // 2
    return img[sy:sy + cropy, sx:sx + cropx]


def volume_to_slices(vol, seg=None, brainmask=None, axis='axial', slice_start=0, slice_end=155, slice_resolution=None, skull_stripping=True,
                     view_mapping=None, empty_percentile=90, empty_thresh=0.2, denoise=False, rotations=(0,), center_crop=None, engine=None,
                     device_stats=None, device_rotate=None, curvature_flow=None, spacing=(1, 1, 1), loader='mslub', skull_removal=True,
                     background_removal=True, crops=None, rng=None, normalization='scaling'):
    """-> (images [k,H,W] float32 in [0,1], labels [k,H,W] float32 in {0,1}, slice indices kept).
    rotations: angles in degrees, one output per angle and slice (dataloaders/BRAINWEB.py:156-162: scipy.ndimage.rotate, reshape False, the label
    map with mode 'nearest'); center_crop (width, height): the `useCrops` / cropType 'center' option (MSLUB.py:206-210).
    engine: an engine with the device `zoom` op (device_ops.DeviceOps.zoom): the kept, padded slices are resampled in one batched device call each
    for the image ('constant') and the label map ('nearest', fp32, then >= 0.9) instead of two scipy calls per slice.
    device_stats (default: on when `engine` has the order-statistic ops, device_ops.DeviceOps.select_quantiles): the masked volume is moved to
    slice-major order and uploaded ONCE as fp32, normalised there (_normalize_scaling_on), the empty-slice filter is one segmented select with
    one segment per slice, and the kept slices are padded and resampled from the device-resident volume -- no second upload of the image.
    The label path is unchanged.  Same kept slices and the same bits as device_stats=False.
    device_rotate (default: on when `engine` has the `rotate` op, device_ops.DeviceOps.rotate): the rotations run on the device -- the resampled
    batch stays there after engine.zoom, one rotate call for the images ('constant') and one for the label maps ('nearest', fp32; they are not
    thresholded again, as on the host) cover all non-zero angles, angle 0 passes through, center_crop is a slice of the result and both maps come
    back in ONE download -- instead of two scipy.ndimage.rotate calls per slice and angle.  Same order (slice-major, angle-minor); values
    within the fp32 rounding of the host loop's.  Without a non-zero angle, with engine=None or a stand-in without the op: the host loop.
    curvature_flow: None (off) | True = (3, 0.125) | (iterations, time_step): the reference's nii.denoise() (NII.py:85-87), applied to the
    NaN-zeroed fp64 volume BEFORE skull stripping, which is where MSLUB.py:242 calls it; spacing = (sx, sy, sz), the voxel size the filter
    scales its differences by (build_cache takes it from the NIfTI header).  The arithmetic is utils/curvature_flow.py's -- ITK's update written
    down from its source, not yet compared with SimpleITK's own output.  With an engine that has the `curvature_flow` op
    (device_ops.DeviceOps.curvature_flow) it runs there, same bits; with device_stats on, the skull-strip multiply and the move to slice-major order
    happen on the device too, so the volume is uploaded once and not downloaded in between.  Without such an engine: the host statement.
    loader: 'mslub' (default) is everything above, the MS datasets' preparation.  'brainweb' is the training set's
    (dataloaders/BRAINWEB.py:125-185, 266-292; see _brainweb_to_slices): `seg` is the TISSUE-CLASS volume (values 0 .. 10) that supplies both
    the skull map -- skull_removal drops FAT, MUSCLE, SKIN, SKULL, CONNECTIVE (4, 5, 6, 7, 9), background_removal drops BACKGROUND (0) -- and
    the lesion map (== 10); constant slices are dropped; a slice larger than slice_resolution on either axis is resized with utils/resize.py
    (cv2.resize: bilinear image, nearest label), otherwise zero-padded; no spline, no re-threshold.  brainmask must be None and
    curvature_flow off (the reference does not denoise BrainWeb); skull_stripping, empty_percentile, empty_thresh and device_stats do not
    apply.
    crops: None | ('center', w, h) | ('lesions', w, h) | ('random', w, h, per_slice): the reference's `useCrops` with its cropType, cropWidth,
    cropHeight and numRandomCropsPerSlice (MSLUB.py:186-222, BRAINWEB.py:165-180), applied to every prepared (and rotated) slice; utils/crops.py
    states the arithmetic.  ('center', w, h) IS center_crop=(w, h); giving both raises ValueError.  'lesions': one crop per 8-connected
    component of the label slice, centred on its centroid, the centre clamped into the slice, a window that still leaves the slice dropped
    (MSLUB.py:200-222); a non-zero rotation raises ValueError -- the MS loaders have no rotations and a spline-rotated label map is not
    binary; loader='brainweb' is allowed (its lesion map is binary).  'random': per slice and angle per_slice windows whose corners are
    drawn from `rng` -- a numpy.random.RandomState, default the numpy.random module as in the reference -- by randint(0, W - w) and
    randint(0, H - h) (BRAINWEB.py:167-170).  The image crop and the label crop share their origins; the reference appends the IMAGE crop
    as the label (BRAINWEB.py:173), here the label map is cropped: a stated deviation.
    Output order: slice-major, angle-minor, then the crops of that slice and angle in origin order (components in raster order of their first
    pixel; random crops in draw order); `kept` carries the slice index of every crop.
    With an engine that has `region_props` and `crop` (device_ops.DeviceOps) the prepared image batch and label batch stay on the device, the
    labels go through region_props(slab=1), the origins are formed on the host from the small table, one crop call serves the images and
    one the labels, and one download follows.  Without such an engine: the host statement.  The same crops bit for bit.
    normalization: 'scaling' (default; what the reference's configurations use) | 'standardization' (the default its loaders declare,
    MSLUB.py:49, BRAINWEB.py:55): NII.normalize's method (NII.py:53-75), with the same [0, 99.8] percentile clamp, for both loaders --
    normalize_standardization in the place of normalize_scaling; the values are then no longer in [0, 1].  Everything behind it is applied
    unchanged, as the reference applies it whatever the method: the empty-slice filter's `percentile < 0.2`, BrainWeb's constant-slice filter,
    zoom / resize, rotations, crops.  With device_stats (or loader='brainweb' on an engine with `resize`) and an engine that has the ordered
    sums (device_ops.DeviceOps.shifted_sums / standardize) the volume stays resident: no extra upload or download, the same kept slices
    and the same bits as the host route; an engine without them takes the host statement for the normalisation (both loaders; only an
    explicit device_stats=True with such an engine raises).  Any other value raises ValueError."""
    _normalization_setting(normalization)
    spec = _crop_setting(crops, center_crop, rotations)
    if spec is not None and spec[0] == 'center':
        center_crop, spec = (spec[1], spec[2]), None
    on_device = spec is not None and hasattr(engine, 'region_props') and hasattr(engine, 'crop')
    out = _prepared_slices(vol, seg, brainmask, axis, slice_start, slice_end, slice_resolution, skull_stripping, view_mapping, empty_percentile, empty_thresh,
                           denoise, rotations, center_crop, engine, device_stats, device_rotate, curvature_flow, spacing, loader, skull_removal, background_removal,
                           resident=on_device, normalization=normalization)
    if spec is None:
        return out
    return _crop_slices(out[0], out[1], out[2], spec, rng, engine if on_device else None)


def _is_tensor(a):
    return hasattr(a, 'data_ptr')


def _crop_setting(crops, center_crop, rotations):
    """volume_to_slices' `crops` keyword -> None | (mode, w, h[, per_slice]), validated."""
    if crops is None:
        return None
    try:
        mode, w, h = crops[0], int(crops[1]), int(crops[2])
        per = int(crops[3]) if mode == 'random' else None
        if len(crops) != (4 if mode == 'random' else 3):
            raise IndexError
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"crops must be ('center', w, h), ('lesions', w, h) or ('random', w, h, per_slice), got {crops!r}") from None
    if mode not in ('center', 'lesions', 'random'):
        raise ValueError(f"crops: the mode must be 'center', 'lesions' or 'random', got {mode!r}")
    if w < 1 or h < 1 or (per is not None and per < 1):
        raise ValueError(f'crops: sizes and the number of crops per slice must be positive, got {crops!r}')
    if center_crop is not None:
        raise ValueError("give either center_crop or crops, not both (crops=('center', w, h) is center_crop=(w, h))")
    if mode == 'lesions' and any(a != 0 for a in rotations):
        raise ValueError("crops 'lesions' does not go with rotations: the MS loaders have none, and a spline-rotated label map is not binary")
    return (mode, w, h) if per is None else (mode, w, h, per)


def _crop_slices(images, labels, kept, spec, rng, engine):
    """The crop step of volume_to_slices for 'lesions' / 'random' on the prepared batches (host arrays, or device tensors with `engine`)."""
    from .crops import component_props, crop_windows, lesion_crop_origins, random_crop_origins
    cw, ch = spec[1], spec[2]
    if not len(kept):
        return np.zeros((0, ch, cw), np.float32), np.zeros((0, ch, cw), np.float32), []
    H, W = (int(v) for v in images.shape[-2:])
    if spec[0] == 'lesions':
        props = engine.region_props(labels, slab=1) if engine is not None else component_props(labels, slab=1)
        origins = lesion_crop_origins(props, H, W, cw, ch)
    else:
        origins = random_crop_origins(len(kept), H, W, cw, ch, spec[3], rng)
    if engine is not None:
        import torch
        both = torch.stack([engine.crop(images, origins, (ch, cw)), engine.crop(labels, origins, (ch, cw))]).cpu().numpy()      # the one download
        im, lb = both[0], both[1]
    else:
        im, lb = crop_windows(np.asarray(images, np.float32), origins, ch, cw), crop_windows(np.asarray(labels, np.float32), origins, ch, cw)
    return im, lb, [kept[int(i)] for i in origins[:, 0]]


def _resident_result(sds, sss, kept_s, rotations):
    """The prepared batches as they are (device tensors stay on the device), one entry per slice and angle: only reached without a non-zero
    angle, so an angle's entry is the slice itself."""
    R = len(rotations)
    out = []
    for b in (sds, sss):
        if _is_tensor(b):
            out.append(b.repeat_interleave(R, dim=0) if R != 1 else b)
        else:
            b = np.asarray(np.stack(b), np.float32)
            out.append(np.repeat(b, R, axis=0) if R != 1 else b)
    return out[0], out[1], [s for s in kept_s for _ in rotations]


def _prepared_slices(vol, seg, brainmask, axis, slice_start, slice_end, slice_resolution, skull_stripping, view_mapping, empty_percentile, empty_thresh, denoise,
                     rotations, center_crop, engine, device_stats, device_rotate, curvature_flow, spacing, loader, skull_removal, background_removal, resident=False, normalization='scaling'):
    """volume_to_slices up to and including rotations and center_crop.  resident: leave batches that are on the device there (device tensors
    [k,H,W] come back in the place of host arrays) when no host step is left to do, i.e. unless a non-zero angle has to be rotated on the host."""
    from scipy.ndimage import rotate, zoom
    if loader == 'brainweb':
        if brainmask is not None:
            raise ValueError("loader='brainweb' takes no brainmask: the skull map comes from the tissue classes in `seg`")
        if _flow_setting(curvature_flow) is not None or denoise:
            raise ValueError("loader='brainweb' does not denoise: the reference calls nii.denoise() for the MS datasets only")
        return _brainweb_to_slices(vol, seg, axis, slice_start, slice_end, slice_resolution, view_mapping, rotations, center_crop, engine, device_rotate,
                                   skull_removal, background_removal, resident, normalization)
    if loader != 'mslub':
        raise ValueError(f"loader must be 'mslub' or 'brainweb', got {loader!r}")
    if denoise:
        raise NotImplementedError("nii.denoise() is SimpleITK's CurvatureFlow filter (MSLUB.py:257); it is not restated here")
    vm = view_mapping or VIEW_MAPPING
    ax = vm[axis]
    flow = _flow_setting(curvature_flow)
    vol = np.array(vol, np.float64)
    vol[np.isnan(vol)] = 0.0
    if seg is None:
        seg = np.zeros_like(vol)
    seg = (np.asarray(seg) >= 0.9).astype(np.float64)                       # MSLUB.py:264-265
    standardization = _normalization_setting(normalization) == 'standardization'
    if device_stats is None:
        device_stats = _has_standardize(engine) if standardization else _has_order_stats(engine)
    elif device_stats and not _has_order_stats(engine):
        raise ValueError('device_stats needs an engine with the order-statistic ops (select_quantiles, clamp_scale)')
    elif device_stats and standardization and not _has_standardize(engine):
        raise ValueError("device_stats with normalization='standardization' needs an engine with the ordered sums (shifted_sums, standardize)")
    flow_dev = None
    if flow is not None:                                                    # nii.denoise(), before the skull map (MSLUB.py:242,257)
        if hasattr(engine, 'curvature_flow'):
            flow_dev = engine.curvature_flow(vol, spacing, time_step=flow[1], iterations=flow[0])
            if not device_stats:
                vol, flow_dev = flow_dev.cpu().numpy(), None
        else:
            from .curvature_flow import curvature_flow as flow_host
            vol = flow_host(vol, spacing, time_step=flow[1], iterations=flow[0])
    if skull_stripping and brainmask is not None:
        if flow_dev is not None:                                            # (the host `vol` only lends its shape from here on)
            import torch
            flow_dev = flow_dev * torch.from_numpy(np.asarray(brainmask) >= 0.1).to(flow_dev.device, flow_dev.dtype)
        else:
            vol = vol * (np.asarray(brainmask) >= 0.1)                      # NII.apply_skullmap
    if device_rotate is None:
        device_rotate = hasattr(engine, 'rotate')
    elif device_rotate and not hasattr(engine, 'rotate'):
        raise ValueError('device_rotate needs an engine with the rotate op')
    device_rotate = bool(device_rotate) and any(a != 0 for a in rotations)
    resident = resident and (device_rotate or not any(a != 0 for a in rotations))
    vol_dev = keep_dev = None
    if device_stats:
        if flow_dev is not None:                                            # the host lines below, on the resident filtered volume
            import torch
            moved = flow_dev.movedim(ax, 0).to(torch.float32).contiguous()
        else:
            moved = engine._dev(np.ascontiguousarray(np.moveaxis(vol, ax, 0), np.float32))
        vol_dev = _normalize_standardization_on(engine, moved, 0, 99.8) if standardization else _normalize_scaling_on(engine, moved, 0, 99.8)
        s_end = min(slice_end, vol.shape[ax])
        if s_end > slice_start:
            stat = engine.percentile(vol_dev[slice_start:s_end], empty_percentile, segments=s_end - slice_start)
            keep_dev = [slice_start + int(i) for i in np.flatnonzero(~(stat < empty_thresh))]      # MSLUB.py:161, one segment per slice
        else:
            keep_dev = []
    else:
        vol = normalize_standardization(vol) if standardization else normalize_scaling(vol)
    sds, sss, kept_s = [], [], []
    for s in (keep_dev if device_stats else range(slice_start, min(slice_end, vol.shape[ax]))):
        idx = [slice(None)] * 3
        idx[ax] = s
        sd, ss = vol[tuple(idx)], seg[tuple(idx)]               # (device_stats: sd only lends its shape; the image stays on the device)
        if not device_stats and np.percentile(sd, empty_percentile) < empty_thresh:              # MSLUB.py:161: skip "empty" slices
            continue
        if slice_resolution is not None:
            H, W = slice_resolution
            py = (math.floor((H - sd.shape[0]) / 2.0), math.ceil((H - sd.shape[0]) / 2.0)) if sd.shape[0] < H else (0, 0)
            px = (math.floor((W - sd.shape[1]) / 2.0), math.ceil((W - sd.shape[1]) / 2.0)) if sd.shape[1] < W else (0, 0)
            if py != (0, 0) or px != (0, 0):
                sd = np.pad(sd, (py, px), 'constant'); ss = np.pad(ss, (py, px), 'constant')
            f = float(H) / float(sd.shape[0])                               # one factor for both axes, as the reference (:179-180)
            if engine is None:
                sd = zoom(sd, f)
                ss = zoom(ss, f, mode='nearest')
                ss = (ss >= 0.9).astype(np.float64)
        sds.append(sd); sss.append(ss); kept_s.append(s)
    if device_stats and sds:
        # the kept slices, gathered and zero-padded where they are: rows of the slice-major device volume into the padded batch
        kept_dev = vol_dev[keep_dev]
        hp, wp = sds[0].shape
        h, w = kept_dev.shape[1:]
        if (hp, wp) != (h, w):
            y0, x0 = math.floor((hp - h) / 2.0) if h < hp else 0, math.floor((wp - w) / 2.0) if w < wp else 0
            padded = kept_dev.new_zeros((kept_dev.shape[0], hp, wp))
            padded[:, y0:y0 + h, x0:x0 + w] = kept_dev
            kept_dev = padded
        sds = kept_dev
    if engine is not None and slice_resolution is not None and len(sds):
        f = float(slice_resolution[0]) / float(sds[0].shape[0])
        hw = tuple(int(round(i * f)) for i in sds[0].shape)                 # scipy.ndimage.zoom's output shape
        sds = engine.zoom(sds if device_stats else np.stack(sds), hw, mode='constant')
        sss = engine.zoom(np.stack(sss), hw, mode='nearest')
        if device_rotate or resident:
            import torch
            sss = (sss.to(torch.float64) >= 0.9).to(torch.float32)          # the host line below, on the resident batch
        else:
            sds = list(sds.cpu().numpy())
            sss = list((sss.cpu().numpy().astype(np.float64) >= 0.9).astype(np.float64))
    elif device_stats and len(sds) and not device_rotate and not resident:
        sds = list(sds.cpu().numpy())
    if device_rotate and len(sds):
        return _rotate_on(engine, sds, sss, kept_s, rotations, center_crop, resident)
    if resident and len(sds) and center_crop is None:
        return _resident_result(sds, sss, kept_s, rotations)
    imgs, labs, kept = [], [], []
    for sd, ss, s in zip(sds, sss, kept_s):
        for angle in rotations:
            sdr, ssr = (sd, ss) if angle == 0 else (rotate(sd, angle, reshape=False), rotate(ss, angle, reshape=False, mode='nearest'))
            if center_crop is not None:
                sdr, ssr = crop_center(sdr, center_crop[0], center_crop[1]), crop_center(ssr, center_crop[0], center_crop[1])
            imgs.append(np.asarray(sdr, np.float32)); labs.append(np.asarray(ssr, np.float32)); kept.append(s)
    if not imgs:
        return np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0), np.float32), []
    return np.stack(imgs), np.stack(labs), kept


BRAINWEB_SKULL_CLASSES = (4, 5, 6, 7, 9)      # BRAINWEB.LABELS FAT, MUSCLE, SKIN, SKULL, CONNECTIVE (BRAINWEB.py:273-277)
BRAINWEB_BACKGROUND, BRAINWEB_LESION = 0, 10


def _brainweb_to_slices(vol, tissue, axis, slice_start, slice_end, slice_resolution, view_mapping, rotations, center_crop, engine, device_rotate,
                        skull_removal, background_removal, resident=False, normalization='scaling'):
    """volume_to_slices(loader='brainweb'): dataloaders/BRAINWEB.py:125-185 with load_volume_and_groundtruth (:266-292) on the repo's arrays.
    NaN -> 0; the skull map is 1 except at the dropped tissue classes and multiplies the volume when either flag is set; the lesion map is
    tissue == 10; normalize_scaling(0, 99.8) -- or, with normalization='standardization', normalize_standardization(0, 99.8) --; then per slice of [slice_start, min(slice_end, n)): a CONSTANT slice (numpy.unique(...).size == 1,
    :133) is skipped; a slice larger than slice_resolution on either axis is resized -- utils/resize.py's resize_linear for the image,
    resize_nearest for the label -- and every other slice is zero-padded, centred with `//` starts (:144-154).
    The output-shape quirk: the reference hands tuple(sliceResolution) to cv2.resize, which reads it as (width, height), so a RESIZED slice
    has shape (slice_resolution[1], slice_resolution[0]) while a PADDED one has shape slice_resolution.  Restated as it is; only a
    non-square resolution shows it.
    A masked voxel is +0 here whatever its sign was (the reference's multiply leaves -0 for a negative one; the two compare equal).
    With an engine that has the `resize` op the whole path runs on the device: one upload of the slice-major volume (fp32) and of the tissue
    classes (uint8), engine.mask_by_label, _normalize_scaling_on, the constant-slice filter as ONE select_quantiles call with q = [0, 1] and
    one segment per slice (constant <=> minimum == maximum: the input is NaN-free and +-0 compare equal there as in numpy.unique),
    engine.resize(index=kept) or a padded copy for both maps, then _rotate_on or one download.  Same kept slices and the same bits as
    engine=None; rotated outputs within the fp32 rounding documented for engine.rotate."""
    from scipy.ndimage import rotate
    from .resize import resize_linear, resize_nearest
    ax = (view_mapping or VIEW_MAPPING)[axis]
    vol = np.array(vol, np.float64)
    vol[np.isnan(vol)] = 0.0
    if tissue is None:
        raise ValueError("loader='brainweb' needs the tissue-class volume as `seg`")
    tissue_in = np.asarray(tissue)
    if tissue_in.shape != vol.shape:
        raise ValueError(f'tissue-class volume {tissue_in.shape} and volume {vol.shape} differ in shape')
    tissue = tissue_in.astype(np.uint8)
    if not np.array_equal(tissue, tissue_in):
        raise ValueError('the tissue-class volume must hold integer class values 0 .. 255')
    dropped = (BRAINWEB_SKULL_CLASSES if skull_removal else ()) + ((BRAINWEB_BACKGROUND,) if background_removal else ())
    keep = [c for c in range(256) if c not in dropped]
    standardization = _normalization_setting(normalization) == 'standardization'
    # an engine with `resize` but without the ordered sums: the host route below, as the MS loaders' path does without device_stats
    on_device = engine is not None and hasattr(engine, 'resize') and (not standardization or _has_standardize(engine))
    if device_rotate is None:
        device_rotate = hasattr(engine, 'rotate')
    elif device_rotate and not hasattr(engine, 'rotate'):
        raise ValueError('device_rotate needs an engine with the rotate op')
    device_rotate = bool(device_rotate) and any(a != 0 for a in rotations)
    resident = resident and (device_rotate or not any(a != 0 for a in rotations))
    n = vol.shape[ax]
    s_end = min(slice_end, n)
    h, w = np.moveaxis(vol, ax, 0).shape[1:]
    resized = slice_resolution is not None and (h > slice_resolution[0] or w > slice_resolution[1])      # :140
    if on_device:
        import torch
        moved = engine._dev(np.ascontiguousarray(np.moveaxis(vol, ax, 0), np.float32))
        masked, lesion = engine.mask_by_label(moved, np.ascontiguousarray(np.moveaxis(tissue, ax, 0)), keep, BRAINWEB_LESION, out=moved)
        vol_dev = _normalize_standardization_on(engine, masked, 0, 99.8) if standardization else _normalize_scaling_on(engine, masked, 0, 99.8)
        kept_s = []
        if s_end > slice_start:
            _, lo, hi = engine.select_quantiles(vol_dev[slice_start:s_end], [0.0, 1.0], [False, False], segments=s_end - slice_start)
            kept_s = [slice_start + int(i) for i in np.flatnonzero(~(lo[:, 0] == hi[:, 1]))]           # :133, one segment per slice
        if not kept_s:
            return np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0), np.float32), []
        if resized:
            out_hw = (slice_resolution[1], slice_resolution[0])             # cv2's dsize is (width, height)
            sds = engine.resize(vol_dev, out_hw, mode='linear', index=kept_s)
            sss = engine.resize(lesion, out_hw, mode='nearest', index=kept_s)
        else:
            sds, sss = vol_dev[kept_s], lesion[kept_s]
            if slice_resolution is not None:
                H, W = slice_resolution
                y0, x0 = (H - h) // 2, (W - w) // 2
                both = sds.new_zeros((2, len(kept_s), H, W))
                both[0, :, y0:y0 + h, x0:x0 + w] = sds
                both[1, :, y0:y0 + h, x0:x0 + w] = sss
                sds, sss = both[0], both[1]
        if device_rotate:
            return _rotate_on(engine, sds, sss, kept_s, rotations, center_crop, resident)
        if resident and center_crop is None:
            return _resident_result(sds, sss, kept_s, rotations)
        both = torch.stack([sds, sss]).cpu().numpy()                        # the one download
        sds, sss = list(both[0]), list(both[1])
    else:
        if dropped:
            vol = np.where(np.isin(tissue, dropped), 0.0, vol)              # :272-289
        lesion = (tissue == BRAINWEB_LESION).astype(np.float32)             # :283-286
        vol = normalize_standardization(vol) if standardization else normalize_scaling(vol)      # :292
        sds, sss, kept_s = [], [], []
        for s in range(slice_start, s_end):
            idx = [slice(None)] * 3
            idx[ax] = s
            sd, ss = vol[tuple(idx)], lesion[tuple(idx)]
            if np.unique(sd).size == 1:                                     # :133
                continue
            if resized:
                sd = resize_linear(sd, (slice_resolution[1], slice_resolution[0]))
                ss = resize_nearest(ss, (slice_resolution[1], slice_resolution[0]))
            elif slice_resolution is not None:
                H, W = slice_resolution
                y0, x0 = (H - h) // 2, (W - w) // 2
                pd, ps = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
                pd[y0:y0 + h, x0:x0 + w] = sd
                ps[y0:y0 + h, x0:x0 + w] = ss
                sd, ss = pd, ps
            sds.append(sd); sss.append(ss); kept_s.append(s)
        if device_rotate and len(sds):
            return _rotate_on(engine, sds, sss, kept_s, rotations, center_crop, resident)
    imgs, labs, kept = [], [], []
    for sd, ss, s in zip(sds, sss, kept_s):
        for angle in rotations:
            sdr, ssr = (sd, ss) if angle == 0 else (rotate(sd, angle, reshape=False), rotate(ss, angle, reshape=False, mode='nearest'))
            if center_crop is not None:
                sdr, ssr = crop_center(sdr, center_crop[0], center_crop[1]), crop_center(ssr, center_crop[0], center_crop[1])
            imgs.append(np.asarray(sdr, np.float32)); labs.append(np.asarray(ssr, np.float32)); kept.append(s)
    if not imgs:
        return np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0), np.float32), []
    return np.stack(imgs), np.stack(labs), kept


def _flow_setting(curvature_flow):
    """volume_to_slices' `curvature_flow` keyword -> None | (iterations, time_step)."""
    if curvature_flow is None or curvature_flow is False:
        return None
    if curvature_flow is True:
        return 3, 0.125                                                     # NII.py:86
    try:
        iterations, time_step = curvature_flow
    except (TypeError, ValueError):
        raise ValueError(f'curvature_flow must be None, True or (iterations, time_step), got {curvature_flow!r}') from None
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f'curvature_flow: iterations must be a non-negative integer, got {iterations!r}')
    return int(iterations), float(time_step)


def _rotate_on(engine, images, labels, kept_s, rotations, center_crop, resident=False):
    """volume_to_slices' rotation step on the device: images / labels [k,H,W] (device tensors, or host arrays where no device step came before)
    -> the (images, labels, kept) volume_to_slices returns.  engine.rotate takes up to 16 angles a call.  resident: no download, the two
    [k * angles, H, W] batches come back as device tensors (for the crop step)."""
    import torch
    angles = [a for a in rotations if a != 0]
    out = []
    for batch, mode in ((images, 'constant'), (labels, 'nearest')):
        rot = torch.cat([engine.rotate(batch, angles[i:i + 16], mode=mode) for i in range(0, len(angles), 16)], dim=1)
        plain = torch.as_tensor(np.stack(batch) if isinstance(batch, list) else batch, dtype=torch.float32, device=rot.device)
        full = rot.new_empty((rot.shape[0], len(rotations)) + tuple(rot.shape[2:]))
        k = 0
        for j, a in enumerate(rotations):
            if a == 0:
                full[:, j] = plain
            else:
                full[:, j] = rot[:, k]
                k += 1
        out.append(full)
    both = torch.stack(out)                                                 # [2, k, R, H, W]
    if center_crop is not None:                                             # crop_center, as a slice of the batch
        y, x = both.shape[-2:]
        sx, sy = x // 2 - center_crop[0] // 2, y // 2 - center_crop[1] // 2
        both = both[..., sy:sy + center_crop[1], sx:sx + center_crop[0]]
    if resident:
        both = both.contiguous().reshape(2, -1, both.shape[-2], both.shape[-1])
        return both[0], both[1], [s for s in kept_s for _ in rotations]
    both = both.contiguous().cpu().numpy()                                            # the one download
    both = both.reshape(2, -1, both.shape[-2], both.shape[-1])              # slice-major, angle-minor
    return both[0], both[1], [s for s in kept_s for _ in rotations]


def partition_patients(n_patients, partition=None, rng=None):
    """Patient-level split of MSLUB.py:71-90: a permutation cut at floor(fraction * n) (fractions <= 1) or at absolute counts."""
    partition = partition or {'TRAIN': 0.7, 'VAL': 0.2, 'TEST': 0.1}
    rng = rng or np.random.default_rng(0)
    ridx = rng.permutation(n_patients)
    out, taken = {}, 0
    for split in partition:
        k = math.floor(partition[split] * n_patients) if partition[split] <= 1.0 else int(partition[split])
        k = min(k, n_patients - taken)
        out[split] = ridx[taken:taken + k]
        taken += k
    return out


def build_cache(directory, patients, partition=None, seed=0, engine=None, **slice_options):
    """patients: [{'name', 'volume': path, 'groundtruth': path or None, 'skullmap': path or None}] -> slice cache in `directory`.
    slice_options: volume_to_slices keywords (device_stats, curvature_flow, normalization, loader / skull_removal / background_removal, crops / rng among them: one
    `rng` serves all patients in order, and it is not recorded in the cache's options; with
    loader='brainweb' 'groundtruth' names the tissue-class volume and 'skullmap' is ignored); engine: volume_to_slices' device resampler / order
    statistics / curvature flow.  Unless slice_options names a `spacing`, each volume gets its own from its header: abs(pixdim[1:4]), a zero
    replaced by 1.0.
    The label map's "brain" class is `image > 0`, which is the skull-stripped brain only with normalization='scaling': a standardized
    background is negative and zero is the volume's mean, so with 'standardization' that class marks the pixels above the mean (and the
    lesion class stays exact).  Whatever reads the cache's brain mask (next_batch(return_brainmask=True), the context-encoder boxes, the
    evaluation's mask) needs a 'scaling' cache; a standardized cache serves training on the images.
    Returns the index dict that was written."""
    from .slice_cache import SET_TYPES, write_cache
    split = partition_patients(len(patients), partition, np.random.default_rng(seed))
    set_of = {}
    for name, ids in split.items():
        for i in ids:
            set_of[int(i)] = SET_TYPES.index(name)
    images, labels, sets, owner = [], [], [], []
    for i, p in enumerate(patients):
        if i not in set_of:
            continue
        vol, hdr = read_nifti(p['volume'])
        seg = read_nifti(p['groundtruth'])[0] if p.get('groundtruth') else None
        msk = read_nifti(p['skullmap'])[0] if p.get('skullmap') and slice_options.get('loader', 'mslub') != 'brainweb' else None
        spacing = tuple(abs(float(d)) or 1.0 for d in hdr['pixdim'][1:4])
        im, lb, kept = volume_to_slices(vol, seg, msk, engine=engine, **{'spacing': spacing, **slice_options})
        if len(kept):
            images.append(im); labels.append(lb); sets += [set_of[i]] * len(kept); owner += [p.get('name', str(i))] * len(kept)
    if not images:
        raise ValueError('no slice survived the filters')
    images = np.concatenate(images)[..., None]
    labels = np.concatenate(labels)
    # label map in BRAINWEB.LABELS values so that the cache's brain-mask LUT works: 10 = LESION, 2 = GM for every other in-brain pixel
    # (non-zero after skull stripping), 0 = BACKGROUND
    lab_u8 = np.where(labels > 0, 10, np.where(images[..., 0] > 0, 2, 0)).astype(np.uint8)
    write_cache(directory, images, sets, lab_u8, patients=owner,
                options={k: (list(v) if isinstance(v, tuple) else v) for k, v in slice_options.items() if k != 'rng'})
    return {'slices': int(images.shape[0]), 'shape': list(images.shape), 'split': {k: [int(i) for i in v] for k, v in split.items()}}
