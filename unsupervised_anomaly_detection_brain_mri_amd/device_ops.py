"""The model-independent device ops of the evaluation and ingestion paths (erosion, 3-D median, splines, curvature flow, resize, component
labelling, crops, 8-bit rendering, order statistics, histograms, confusion counts, residual maps, sort-based metrics) as a class that stands alone: the C
entry points take no model handle, so neither does DeviceOps.  The AE-family Engine and the f-AnoGAN GanEngine inherit it."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .utils.order_stats import OrderStatOps, as_float32_exact


class _DevArray:
    """__cuda_array_interface__ shim: lets torch alias a raw device pointer without copying."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {'shape': (int(count),), 'typestr': '<f4', 'data': (int(ptr), False),
                                         'version': 2, 'strides': None}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def zoom_output_hw(in_hw, factors):
    """The output shape scipy.ndimage.zoom gives a [h,w] slice: round(h * zoom) per axis (one factor serves both axes)."""
    f = (factors, factors) if np.isscalar(factors) else tuple(factors)
    return tuple(int(round(i * z)) for i, z in zip(in_hw, f))


def rotation_transform(angle, in_hw):
    """(matrix [2,2], offset [2]) that scipy.ndimage.rotate(a, angle, reshape=False) hands to affine_transform for a [h,w] slice, formed with
    scipy's own numpy expressions (cosdg / sindg, the M @ v product) so that the doubles are the same bit for bit."""
    from scipy.special import cosdg, sindg
    c, s = cosdg(angle), sindg(angle)
    m = np.array([[c, s], [-s, c]])
    in_center = (np.asarray(in_hw) - 1) / 2
    return m, in_center - m @ in_center


def check_rects(rects, n, h, w):
    """The window table of assemble_batch / context_mask, validated on the host: integers [n,3,4] of (row, col, height, width), a window with
    height 0 unused, every used one non-empty and inside the h x w slice -> contiguous int32 [n,3,4]; ValueError otherwise."""
    r = np.asarray(rects)
    if r.shape != (n, 3, 4) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f'rects must be integers of shape [{n},3,4], got {r.dtype} {r.shape}')
    r = r.astype(np.int64)
    used = r[..., 2] != 0
    bad = used & ((r[..., 0] < 0) | (r[..., 1] < 0) | (r[..., 2] < 0) | (r[..., 3] <= 0) | (r[..., 0] + r[..., 2] > h) | (r[..., 1] + r[..., 3] > w))
    if bad.any():
        b, k = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f'window {k} of sample {b} {tuple(int(v) for v in r[b, k])} leaves the {h} x {w} slice')
    return np.ascontiguousarray(r, np.int32)


class DeviceOps(OrderStatOps):
    """The device ops on one GPU; no model handle (close() is a no-op so that callers can treat it like an engine).
    quantile / percentile / histogram come from utils.order_stats.OrderStatOps over the raw ops select_quantiles / histogram_edges below."""

    def __init__(self, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError('uad_hip needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback')
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        torch.cuda.set_device(self.device)

    def close(self):
        pass

    def _dev(self, a, shape=None):
        """-> contiguous fp32 device tensor of an array / tensor (None stays None), of `shape` when one is given."""
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f'expected shape {tuple(shape)}, got {tuple(t.shape)}')
        return t

    def _f32(self, a, what, ndim, nonempty=False):
        """_dev(a) of rank `ndim` (and, with nonempty, of at least one element); `what` words the ValueError."""
        t = self._dev(a)
        if t.dim() != ndim or (nonempty and t.numel() == 0):
            raise ValueError(f'{what}, got {tuple(t.shape)}')
        return t

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---------------------------------------------------------------- scoring
    def erode_cross(self, masks, iterations=12):
        """Brain-mask erosion on device (utils/Evaluation.py:84-89): masks [n,H,W] (any dtype, nonzero = set) -> fp32 0/1 tensor."""
        mk = self._f32(masks, 'masks must be [n,H,W]', 3)
        out = torch.empty_like(mk)
        _lib.check(self.lib.uad_erode_cross(_ptr(mk), mk.shape[0], mk.shape[1], mk.shape[2], int(iterations), _ptr(out),
                                            self._stream()))
        return out

    def median3d(self, volume, ksize=5):
        """5x5x5 median filter of a [D,H,W] volume, scipy 'reflect' boundary (utils/Evaluation.py:108-110)."""
        v = self._f32(volume, 'volume must be [D,H,W]', 3)
        out = torch.empty_like(v)
        _lib.check(self.lib.uad_median3d(_ptr(v), v.shape[0], v.shape[1], v.shape[2], int(ksize), _ptr(out), self._stream()))
        return out

    def zoom(self, slices, out_hw, mode='constant', integer=False):
        """scipy.ndimage.zoom(s, (H/h, W/w), order=3, mode=mode) of every slice of a [n,h,w] array / tensor on the device (uad_zoom_spline3;
        utils/Evaluation.py:223-232, 323-334).  out_hw = (H, W): the caller computes the shape as scipy does (zoom_output_hw).  mode 'constant'
        (cval 0) | 'nearest'.  integer=False -> fp32 tensor [n,H,W]; integer=True -> int32, the spline value rounded half away from zero,
        which is what scipy returns for an integer-typed label / skull map."""
        if mode not in ('constant', 'nearest'):
            raise ValueError(f"zoom mode must be 'constant' or 'nearest', got {mode!r}")
        s = self._f32(slices, 'slices must be [n,h,w]', 3)
        n, h, w = s.shape
        H, W = (int(v) for v in out_hw)
        out = torch.empty((n, H, W), device=self.device, dtype=torch.int32 if integer else torch.float32)
        if n == 0:
            return out
        boundary = _lib.ZOOM_NEAREST if mode == 'nearest' else _lib.ZOOM_CONSTANT
        nbytes = int(self.lib.uad_zoom_spline3_workspace(n, h, w, boundary))
        ws = torch.empty(max(nbytes // 8, 1), device=self.device, dtype=torch.float64)       # stream-ordered caching allocator: safe to drop after the launch
        _lib.check(self.lib.uad_zoom_spline3(_ptr(s), n, h, w, H, W, boundary, _lib.ZOOM_I32 if integer else _lib.ZOOM_F32, _ptr(out), _ptr(ws),
                                             nbytes, self._stream()))
        return out

    def affine(self, slices, matrices, offsets, out_hw=None, mode='constant', integer=False):
        """scipy.ndimage.affine_transform(s, M, offset, output_shape=out_hw, order=3, mode=mode) of every slice of a [n,h,w] array / tensor
        under each of K <= 16 transforms on the device (uad_affine_spline3; one spline prefilter serves all K) -> [n,K,H,W].  matrices [K,2,2]
        (or one [2,2]), offsets [K,2] (or one [2]): output pixel (Y,X) reads input coordinate M @ (Y,X) + offset.  out_hw None = (h,w).
        mode 'constant' (cval 0) | 'nearest'; integer as in zoom (int32, the spline rounded half away from zero)."""
        if mode not in ('constant', 'nearest'):
            raise ValueError(f"affine mode must be 'constant' or 'nearest', got {mode!r}")
        s = self._f32(slices, 'slices must be [n,h,w]', 3)
        m = np.asarray(matrices, np.float64)
        o = np.asarray(offsets, np.float64)
        if m.ndim == 2:
            m, o = m[None], o[None]
        if m.ndim != 3 or m.shape[1:] != (2, 2) or o.shape != (m.shape[0], 2):
            raise ValueError(f'matrices must be [K,2,2] with offsets [K,2], got {m.shape} / {o.shape}')
        K = m.shape[0]
        if not 1 <= K <= _lib.AFFINE_MAX_K:
            raise ValueError(f'1 .. {_lib.AFFINE_MAX_K} transforms a call, got {K}')
        n, h, w = s.shape
        H, W = (h, w) if out_hw is None else (int(v) for v in out_hw)
        out = torch.empty((n, K, H, W), device=self.device, dtype=torch.int32 if integer else torch.float32)
        xf = np.ascontiguousarray(np.concatenate([m.reshape(K, 4), o], axis=1))          # m00 m01 m10 m11 off0 off1
        boundary = _lib.ZOOM_NEAREST if mode == 'nearest' else _lib.ZOOM_CONSTANT
        if n == 0:
            return out
        nbytes = int(self.lib.uad_affine_spline3_workspace(n, h, w, boundary))
        ws = torch.empty(max(nbytes // 8, 1), device=self.device, dtype=torch.float64)       # stream-ordered caching allocator: safe to drop after the launch
        _lib.check(self.lib.uad_affine_spline3(_ptr(s), n, h, w, H, W, xf.ctypes.data_as(C.POINTER(C.c_double)), K, boundary,
                                               _lib.ZOOM_I32 if integer else _lib.ZOOM_F32, _ptr(out), _ptr(ws), nbytes, self._stream()))
        return out

    def rotate(self, slices, angles, mode='constant', integer=False):
        """scipy.ndimage.rotate(s, angle, reshape=False, order=3, mode=mode) of every slice of a [n,h,w] array / tensor for each of up to 16
        angles [degrees] -> [n,K,h,w] (dataloaders/BRAINWEB.py:156-162: the `rotations` augmentation, 'nearest' for the label map).  Matrix and
        offset are formed with scipy's own expressions, so the six doubles are scipy's bit for bit (90 and 180 degrees give exact 0 / +-1).
        Angles that are multiples of 360 are not special-cased: the caller skips them."""
        s = slices if isinstance(slices, torch.Tensor) else np.asarray(slices)
        if s.ndim != 3:
            raise ValueError(f'slices must be [n,h,w], got {tuple(s.shape)}')
        ms, offs = zip(*(rotation_transform(a, s.shape[1:]) for a in np.atleast_1d(np.asarray(angles, np.float64)))) if np.size(angles) else ((), ())
        return self.affine(s, np.array(ms).reshape(-1, 2, 2), np.array(offs).reshape(-1, 2), None, mode=mode, integer=integer)

    def curvature_flow(self, vol, spacing=(1, 1, 1), time_step=0.125, iterations=3):
        """nii.denoise() (utils/NII.py:85-87: sitk.CurvatureFlow(timeStep=0.125, numberOfIterations=3)) of one [z,y,x] volume on the device
        (uad_curvature_flow): the arithmetic of utils/curvature_flow.py -- ITK's update written down from its source, not yet compared with
        SimpleITK's own output -- and its bits.  vol: host array or device tensor; float32 is uploaded as it is and widened exactly on the
        device, everything else goes through float64.  spacing = (sx, sy, sz).  -> float64 device tensor [z,y,x]; the input is not modified."""
        v = vol
        if not isinstance(v, torch.Tensor):
            a = np.asarray(v)
            v = torch.from_numpy(np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64))
        v = v.to(self.device, torch.float32 if v.dtype == torch.float32 else torch.float64).contiguous()
        if v.dim() != 3 or v.numel() == 0:
            raise ValueError(f'vol must be a non-empty [z,y,x] volume, got {tuple(v.shape)}')
        if int(iterations) != iterations:
            raise ValueError(f'iterations must be an integer, got {iterations!r}')
        if len(spacing) != 3:
            raise ValueError(f'spacing must be (sx, sy, sz), got {spacing!r}')
        sp = (C.c_double * 3)(*(float(s) for s in spacing))
        nz, ny, nx = v.shape
        out = torch.empty((nz, ny, nx), device=self.device, dtype=torch.float64)
        ws = None
        if iterations >= 2:                                      # stream-ordered caching allocator: safe to drop after the launches
            ws = torch.empty(int(self.lib.uad_curvature_flow_workspace(nz, ny, nx)) // 8, device=self.device, dtype=torch.float64)
        _lib.check(self.lib.uad_curvature_flow(_ptr(v), int(v.dtype == torch.float32), nz, ny, nx, sp, float(time_step), int(iterations), _ptr(out), _ptr(ws),
                                               self._stream()))
        return out

    def resize(self, slices, out_hw, mode='linear', index=None):
        """cv2.resize(s, (W, H)) of slices of a [n_in,h,w] array / tensor on the device (uad_resize2d; dataloaders/BRAINWEB.py:140-142):
        mode 'linear' = the default INTER_LINEAR (the image), 'nearest' = INTER_NEAREST (the label map), the arithmetic of utils/resize.py --
        OpenCV 4.2's resize.cpp written down, not compared with OpenCV's own output -- and its bits.  out_hw = (H, W).  index: None = every
        slice in order, otherwise the input slice of each output slice (any order, repeats allowed; validated here, on the host), so that the
        kept slices of a resident slice-major volume are resized where they lie.  -> fp32 device tensor [n,H,W]."""
        if mode not in ('linear', 'nearest'):
            raise ValueError(f"resize mode must be 'linear' or 'nearest', got {mode!r}")
        s = self._f32(slices, 'slices must be a non-empty [n,h,w]', 3, nonempty=True)
        n_in, h, w = s.shape
        H, W = (int(v) for v in out_hw)
        if H < 1 or W < 1:
            raise ValueError(f'out_hw must be positive, got {(H, W)}')
        idx, n = None, n_in
        if index is not None:
            host = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index)
            if host.size == 0:
                host = host.astype(np.int64)
            if host.ndim != 1 or not np.issubdtype(host.dtype, np.integer):
                raise ValueError(f'index must be a 1-D integer list, got shape {host.shape} dtype {host.dtype}')
            if host.size and (host.min() < 0 or host.max() >= n_in):
                raise ValueError(f'index entries must lie in [0, {n_in}), got {int(host.min())} .. {int(host.max())}')
            n = int(host.size)
            idx = torch.from_numpy(np.ascontiguousarray(host, np.int32)).to(self.device)
        out = torch.empty((n, H, W), device=self.device, dtype=torch.float32)
        if n == 0:
            return out
        _lib.check(self.lib.uad_resize2d(_ptr(s), n_in, h, w, _ptr(idx), n, H, W, _lib.RESIZE_NEAREST if mode == 'nearest' else _lib.RESIZE_LINEAR,
                                         _ptr(out), self._stream()))
        return out

    def mask_by_label(self, vol, labels, keep, lesion_label=None, out=None):
        """The skull-map multiply and the lesion binarisation of BRAINWEB.load_volume_and_groundtruth (dataloaders/BRAINWEB.py:266-289) in one
        device pass (uad_mask_by_label): vol (fp32, any shape) where the uint8 tissue class `labels` is one of `keep`, +0 elsewhere.
        -> the masked fp32 device tensor, or with lesion_label (masked, lesion) where lesion = 1.0 at labels == lesion_label, else 0.0.
        out: None = a new tensor; `vol` itself (a device tensor) masks in place."""
        v = self._dev(vol)
        lb = labels if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if lb.dtype not in (torch.uint8, np.uint8):
            raise TypeError(f'labels must be uint8, got {lb.dtype}')
        if not isinstance(lb, torch.Tensor):
            lb = torch.from_numpy(np.ascontiguousarray(lb))
        lb = lb.to(self.device).contiguous()
        if lb.shape != v.shape or v.numel() == 0:
            raise ValueError(f'vol {tuple(v.shape)} and labels {tuple(lb.shape)} must be non-empty and of one shape')
        lut = np.zeros(256, np.uint8)
        keep = [int(k) for k in keep]
        if any(k < 0 or k > 255 for k in keep) or (lesion_label is not None and not 0 <= int(lesion_label) <= 255):
            raise ValueError('label values are bytes: 0 .. 255')
        lut[keep] = 1
        lut_d = torch.from_numpy(lut).to(self.device)
        if out is None:
            out = torch.empty_like(v)
        elif not (isinstance(out, torch.Tensor) and out.is_contiguous() and out.dtype == torch.float32 and out.shape == v.shape and out.device == v.device):
            raise ValueError('out must be a contiguous fp32 device tensor of vol\'s shape')
        lesion = torch.empty_like(v) if lesion_label is not None else None
        _lib.check(self.lib.uad_mask_by_label(_ptr(v), _ptr(lb), v.numel(), _ptr(lut_d), _ptr(out), _ptr(lesion),
                                              -1 if lesion_label is None else int(lesion_label), self._stream()))
        return out if lesion_label is None else (out, lesion)

    def mc_stats(self, recs, mask=None):
        """Monte-Carlo dropout statistics (utils/Evaluation.py:238-266): recs [K, ...] device / host array of K reconstructions, mask
        broadcastable to one sample.  Returns (mean, epistemic variance) of the masked reconstructions as device tensors."""
        r = self._dev(recs)
        K, total = r.shape[0], r[0].numel()
        m = None
        if mask is not None:
            m = self._dev(mask).expand(r.shape[1:]).contiguous()
        mean, var = torch.empty_like(r[0]), torch.empty_like(r[0])
        _lib.check(self.lib.uad_mc_stats(_ptr(r), _ptr(m), K, total, _ptr(mean), _ptr(var), self._stream()))
        return mean, var

    def cc_filter(self, volume, max_voxels=7):
        """filter_3d_connected_components (utils/Evaluation.py:113-127) of a [D,H,W] volume (bool / float, non-zero = foreground):
        components of at most `max_voxels` voxels are zeroed.  Returns a float device tensor."""
        v = self._f32(volume, 'cc_filter expects a [D,H,W] volume', 3)
        out = torch.empty_like(v)
        _lib.check(self.lib.uad_cc_filter(_ptr(v), v.shape[0], v.shape[1], v.shape[2], int(max_voxels), _ptr(out), self._stream()))
        return out

    def cc_label(self, volume, slab=0):
        """26-connected component labelling of a [D,H,W] volume (bool / float, non-zero = foreground) -> int32 device tensor: 0 = background,
        otherwise 1 + the smallest linear index of the voxel's component.  slab > 0: groups of `slab` slices are labelled independently
        (the reference's chunks of 20, utils/Evaluation.py:141)."""
        v = self._f32(volume, 'cc_label expects a [D,H,W] volume', 3)
        out = torch.empty(v.shape, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.uad_cc_label(_ptr(v), v.shape[0], v.shape[1], v.shape[2], int(slab), _ptr(out), None, self._stream()))
        return out

    def detection_rate(self, pred, gt, slab=20, min_voxels=8):
        """compute_detection_rate (utils/Evaluation.py:130-172) on the device: lesion-wise (TPs, FPs, FNs) of a predicted against a
        ground-truth [D,H,W] volume, counted on 26-connected components in chunks of `slab` slices.  Python ints."""
        p = self._f32(pred, 'detection_rate expects a [D,H,W] volume', 3)
        g = self._f32(gt, 'detection_rate expects a [D,H,W] volume', 3)
        if p.shape != g.shape:
            raise ValueError(f'prediction {tuple(p.shape)} and ground truth {tuple(g.shape)} differ in shape')
        counts = torch.empty(3, device=self.device, dtype=torch.int64)
        _lib.check(self.lib.uad_detection_rate(_ptr(p), _ptr(g), p.shape[0], p.shape[1], p.shape[2], int(slab), int(min_voxels), _ptr(counts),
                                               self._stream()))
        tps, fps, fns = (int(c) for c in counts.cpu().tolist())
        return tps, fps, fns

    def _label_bytes(self, gt, n):
        """-> contiguous uint8 device tensor [n], non-zero = lesion: uint8 data as it is (a resident tensor is not copied, a host array goes up
        once); a numpy array or a tensor of any other integer / bool dtype is made uint8 (`!= 0`) where it lives and uploaded once."""
        if isinstance(gt, torch.Tensor):
            if gt.dtype.is_floating_point or gt.dtype.is_complex:
                raise ValueError(f'labels must be of an integer or bool dtype, got {gt.dtype}')
            t = gt.reshape(-1)
            if t.dtype != torch.uint8:
                t = (t != 0).to(torch.uint8)
            t = t.to(self.device).contiguous()
        else:
            a = np.asarray(gt)
            if not (np.issubdtype(a.dtype, np.integer) or a.dtype == bool):
                raise ValueError(f'labels must be of an integer or bool dtype, got {a.dtype}')
            a = a.reshape(-1)
            t = torch.from_numpy(np.ascontiguousarray(a if a.dtype == np.uint8 else (a != 0).view(np.uint8))).to(self.device)
        if t.numel() != n:
            raise ValueError(f'{t.numel()} labels for {n} values')
        return t

    def confusion_counts(self, pred, gt, lengths, thr=0.0):
        """utils.confusion.confusion_counts on the device (uad_confusion_by_segment): {TP, FP, FN, TN} of `pred > thr` against `gt != 0` for each
        of the contiguous segments of `lengths` voxels (the patients of a stacked volume) -> numpy int64 [P, 4].  pred: a device fp32 tensor of
        any shape, or an array that is uploaded; gt: see _label_bytes; lengths: non-negative integers that add up to the number of voxels
        (ValueError otherwise); thr is taken as float32.  Three launches (zero, count, TN), of which the count reads 5 B per voxel, one download of 32 B per segment."""
        from .utils.confusion import segment_offsets
        t = self._dev(pred).reshape(-1)
        n = t.numel()
        lab = self._label_bytes(gt, n)
        offsets = segment_offsets(lengths, n)
        n_seg = offsets.size - 1
        if n_seg > 65535:
            raise ValueError(f'at most 65535 segments a call, got {n_seg}')
        if n_seg == 0:
            return np.zeros((0, 4), np.int64)
        off = torch.from_numpy(offsets).to(self.device)
        counts = torch.empty((n_seg, 4), device=self.device, dtype=torch.int64)
        _lib.check(self.lib.uad_confusion_by_segment(_ptr(t), float(thr), _ptr(lab), n, _ptr(off), n_seg, int(np.diff(offsets).max()), _ptr(counts),
                                                     self._stream()))
        return counts.cpu().numpy()

    def region_props(self, volume_or_labels, slab=0):
        """skimage's label + regionprops as dataloaders/MSLUB.py:201-206 use them, on the device (uad_cc_label + uad_cc_props; the statement is
        utils/crops.py's component_props -- skimage is not a dependency and has not been compared with): a [D,H,W] volume -> host int64 array
        [K,5], one row per 26-connected component: first (smallest linear index), area, sum_z, sum_y, sum_x, ordered by `first`.
        An int32 array / tensor is taken as a LABEL volume (the output of cc_label; `slab` is then the labelling's and is not used here);
        anything else is a mask (non-zero = foreground) and is labelled first in groups of `slab` slices (1: every slice on its own, the
        8-connectivity of a 2-D slice).  The count comes from the labelling (one small synchronising download), after which the table is
        allocated exactly; for a label volume a table of 4096 rows is tried first."""
        v = volume_or_labels
        is_labels = (v.dtype == torch.int32) if isinstance(v, torch.Tensor) else (np.asarray(v).dtype == np.int32)
        count = None
        if is_labels:
            lab = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(self.device).contiguous()
            if lab.dim() != 3:
                raise ValueError('region_props expects a [D,H,W] volume')
        else:
            m = self._f32(v, 'region_props expects a [D,H,W] volume', 3)
            if m.numel() == 0:
                raise ValueError('region_props expects a non-empty volume')
            lab = torch.empty(m.shape, device=self.device, dtype=torch.int32)
            cnt = torch.empty(1, device=self.device, dtype=torch.int32)
            _lib.check(self.lib.uad_cc_label(_ptr(m), m.shape[0], m.shape[1], m.shape[2], int(slab), _ptr(lab), _ptr(cnt), self._stream()))
            count = int(cnt.item())
            if count == 0:
                return np.zeros((0, 5), np.int64)
        D, H, W = lab.shape
        nbytes = int(self.lib.uad_cc_props_workspace(D, H, W))
        if nbytes == 0:
            raise ValueError(f'region_props: a volume of {D} x {H} x {W} is empty or has 2^31 voxels or more')
        ws = torch.empty((nbytes + 7) // 8, device=self.device, dtype=torch.int64)          # stream-ordered caching allocator: safe to drop after the launches
        n_dev = torch.empty(1, device=self.device, dtype=torch.int32)
        cap = count if count is not None else 4096
        while True:
            props = torch.empty((cap, 5), device=self.device, dtype=torch.int64)
            _lib.check(self.lib.uad_cc_props(_ptr(lab), D, H, W, _ptr(props), cap, _ptr(n_dev), _ptr(ws), self._stream()))
            n = int(n_dev.item())
            if n <= cap:
                return props[:n].cpu().numpy()
            cap = n

    def crop(self, slices, origins, crop_hw):
        """image_utils.crop (img[y:y + height, x:x + width]; dataloaders/MSLUB.py:215-218, BRAINWEB.py:172-173) for k windows of a [n,h,w]
        array / tensor in one device pass (uad_crop2d).  origins: HOST integer array [k,3] of (slice, top, left), any order, repeats allowed,
        validated here: the slice in range and the window inside it.  crop_hw = (height, width).  -> fp32 device tensor [k,height,width];
        the words are copied (+-0, denormals and NaN payloads survive).  k = 0 gives an empty tensor without a launch."""
        from .utils.crops import check_origins
        s = self._f32(slices, 'slices must be a non-empty [n,h,w]', 3, nonempty=True)
        n_in, h, w = s.shape
        ch, cw = (int(v) for v in crop_hw)
        if ch < 1 or cw < 1 or ch > h or cw > w:
            raise ValueError(f'crop_hw {(ch, cw)} must be positive and fit the {h} x {w} slice')
        host = np.asarray(origins.cpu() if isinstance(origins, torch.Tensor) else origins)
        o = check_origins(host, n_in, h, w, ch, cw)
        k = int(o.shape[0])
        out = torch.empty((k, ch, cw), device=self.device, dtype=torch.float32)
        if k == 0:
            return out
        od = torch.from_numpy(np.ascontiguousarray(o)).to(self.device)
        for j0 in range(0, k, 65535):                                       # one grid holds 65535 windows
            kk = min(65535, k - j0)
            _lib.check(self.lib.uad_crop2d(_ptr(s), n_in, h, w, _ptr(od[j0:j0 + kk]), kk, ch, cw, _ptr(out[j0:j0 + kk]), self._stream()))
        return out

    # ---------------------------------------------------------------- context masking and instance noise of a batch (csrc/uad_batch.hip)
    def brain_boxes(self, masks_or_labels, lut=None):
        """The bounding box of the non-zero pixels of every slice (trainers/CE.py:124-126: np.argwhere of the brain mask) on the device
        (uad_brain_boxes / uad_brain_boxes_f32) -> int32 device tensor [n,4] of (row_min, row_max, col_min, col_max), both ends inclusive,
        (-1,-1,-1,-1) for a slice without a non-zero pixel.  A uint8 array / tensor [n,h,w] is a label store, read through `lut` ([256] uint8,
        None = the label value); anything else is an fp32 mask [n,h,w] (a trailing channel axis of 1 is dropped), non-zero = set."""
        a = masks_or_labels
        if (a.dtype == torch.uint8) if isinstance(a, torch.Tensor) else (np.asarray(a).dtype == np.uint8):
            lab = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(self.device).contiguous()
            if lab.dim() != 3 or lab.numel() == 0:
                raise ValueError(f'labels must be a non-empty [n,h,w], got {tuple(lab.shape)}')
            lut_d = None
            if lut is not None:
                lut_d = lut if isinstance(lut, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lut))
                if lut_d.dtype != torch.uint8 or tuple(lut_d.shape) != (256,):
                    raise ValueError(f'lut must be [256] uint8, got {tuple(lut_d.shape)} {lut_d.dtype}')
                lut_d = lut_d.to(self.device).contiguous()
            out = torch.empty((lab.shape[0], 4), device=self.device, dtype=torch.int32)
            _lib.check(self.lib.uad_brain_boxes(_ptr(lab), lab.shape[0], lab.shape[1], lab.shape[2], _ptr(lut_d), _ptr(out), self._stream()))
            return out
        if lut is not None:
            raise ValueError('lut goes with a uint8 label store')
        m = self._f32_batch(a, 'masks')
        if m.shape[0] == 0:
            raise ValueError('masks must be a non-empty [n,h,w]')
        out = torch.empty((m.shape[0], 4), device=self.device, dtype=torch.int32)
        _lib.check(self.lib.uad_brain_boxes_f32(_ptr(m), m.shape[0], m.shape[1], m.shape[2], _ptr(out), self._stream()))
        return out

    def assemble_batch(self, src, index=None, rects=None, noise=None, want_x=True):
        """The batch and its context-masked companion in one device pass (uad_assemble_batch): x[b] = src[index[b]] (index None: src[b]) plus
        sigma * N(0,1) with noise = (sigma, seed, step, sample0, stream) -- the numbers engine.rng_fill gives job `stream` of a call with the
        same (seed, step, sample0); the reference's Options.addInstanceNoise, dataloaders/BRAINWEB.py:459 -- and x_ce[b] = x[b] * m_b with m_b
        zero inside sample b's windows (trainers/CE.py:128-139).  src: fp32 [N,h,w,c] array / tensor; index: integer list, a HOST one is
        validated, a device int32 tensor is taken as it is (DeviceDataset's own); rects: [n,3,4] integers (row, col, height, width), height 0 =
        unused -- a host table is validated here (shape, every used window inside the slice), a device int32 tensor only for its shape.
        -> (x, x_ce) device tensors [n,h,w,c]; x is None with want_x=False, x_ce is None without rects."""
        s = self._f32(src, 'src must be a non-empty [N,h,w,c]', 4, nonempty=True)
        N, h, w, c = s.shape
        if (h * w * c) % 4:
            raise ValueError(f'h * w * c must be a multiple of 4, got {h} x {w} x {c}')
        idx, n = None, N
        if index is not None:
            if isinstance(index, torch.Tensor) and index.is_cuda:
                if index.dtype != torch.int32 or index.dim() != 1:
                    raise ValueError('a device index must be a 1-D int32 tensor')
                idx = index.contiguous()
            else:
                host = np.asarray(index.numpy() if isinstance(index, torch.Tensor) else index)
                if host.ndim != 1 or host.size == 0 or not np.issubdtype(host.dtype, np.integer):
                    raise ValueError(f'index must be a non-empty 1-D integer list, got shape {host.shape} dtype {host.dtype}')
                if host.min() < 0 or host.max() >= N:
                    raise ValueError(f'index entries must lie in [0, {N}), got {int(host.min())} .. {int(host.max())}')
                idx = torch.from_numpy(np.ascontiguousarray(host, np.int32)).to(self.device)
            n = int(idx.numel())
            if n == 0:
                raise ValueError('index must not be empty')
        rd = None
        if rects is not None:
            if isinstance(rects, torch.Tensor) and rects.is_cuda:
                if rects.dtype != torch.int32 or tuple(rects.shape) != (n, 3, 4):
                    raise ValueError(f'rects must be int32 [{n},3,4], got {rects.dtype} {tuple(rects.shape)}')
                rd = rects.contiguous()
            else:
                rd = torch.from_numpy(check_rects(rects.numpy() if isinstance(rects, torch.Tensor) else rects, n, h, w)).to(self.device)
        elif not want_x:
            raise ValueError('nothing asked for: want_x=False without rects')
        sigma, seed, step, sample0, stream = (0.0, 0, 0, 0, 0) if noise is None else noise
        if not (0.0 <= float(sigma) < math.inf):
            raise ValueError(f'sigma must be finite and >= 0, got {sigma!r}')
        if int(sample0) < 0 or int(step) < 0:
            raise ValueError('step and sample0 must be >= 0')
        x = torch.empty((n, h, w, c), device=self.device, dtype=torch.float32) if want_x else None
        x_ce = torch.empty((n, h, w, c), device=self.device, dtype=torch.float32) if rd is not None else None
        for j0 in range(0, n, 65535):                                       # one grid holds 65535 samples
            k = min(65535, n - j0)
            part = lambda t: None if t is None else _ptr(t[j0:j0 + k])
            _lib.check(self.lib.uad_assemble_batch(_ptr(s) if idx is not None else _ptr(s[j0:j0 + k]), part(idx), k, h, w, c, part(rd), float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step),
                                                   int(sample0) + j0, int(stream), part(x), part(x_ce), self._stream()))
        return x, x_ce

    def context_mask(self, batch, rects):
        """batch * mask of trainers/CE.py:139 for a device batch [n,h,w,c] and its windows [n,3,4] -> the masked device tensor."""
        return self.assemble_batch(batch, rects=rects, want_x=False)[1]

    # ---------------------------------------------------------------- 8-bit rendering of the sample images (csrc/uad_render.hip)
    def _f32_batch(self, a, what, shape=None):
        """-> contiguous fp32 device tensor [n,h,w] of an array / tensor (a trailing channel axis of 1 is dropped)."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
        t = t.to(self.device, torch.float32)
        if t.dim() == 4 and t.shape[3] == 1:
            t = t[..., 0]
        if t.dim() != 3 or t.shape[1] < 1 or t.shape[2] < 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
            raise ValueError(f'{what} must be [n,h,w] with h, w >= 1' + (f' of shape {tuple(shape)}' if shape is not None else '') + f', got {tuple(t.shape)}')
        return t.contiguous()

    def render_gray(self, x):
        """normalize_and_squeeze (utils/Evaluation.py:368: cv2.normalize(x, None, 0, 255, NORM_MINMAX), astype('uint8')) of every slice of a
        [n,h,w] array / tensor on the device (uad_render_minmax_u8) -> uint8 device tensor [n,h,w] with the bytes of utils/render.py's
        minmax_u8 -- OpenCV's documented arithmetic written down, not compared with OpenCV's own output.  Integer label maps are cast to
        fp32 (label_u8)."""
        t = self._f32_batch(x, 'x')
        out = torch.empty(tuple(t.shape), device=self.device, dtype=torch.uint8)
        _lib.check(self.lib.uad_render_minmax_u8(_ptr(t), t.shape[0], t.shape[1] * t.shape[2], _ptr(out), self._stream()))
        return out

    def render_heatmap(self, d, lut=None):
        """The squashed heat map with its colour bar (utils/Evaluation.py:319-321) of every slice of a [n,h,w] residual array / tensor on the
        device (uad_render_heatmap) -> uint8 device tensor [n,h,w,4], the bytes of utils/render.py's heatmap_rgba up to the last place of
        exp().  lut: a [256,4] uint8 colour table (array or tensor); None = the package's jet table."""
        from .utils import render
        t = self._f32_batch(d, 'd')
        if lut is None:
            if getattr(self, '_jet_lut', None) is None:
                self._jet_lut = torch.from_numpy(render.jet_u8().copy()).to(self.device)
            lut_d = self._jet_lut
        else:
            lut_d = lut if isinstance(lut, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lut))
            if lut_d.dtype != torch.uint8 or tuple(lut_d.shape) != (256, 4):
                raise ValueError(f'lut must be [256,4] uint8, got {tuple(lut_d.shape)} {lut_d.dtype}')
            lut_d = lut_d.to(self.device).contiguous()
        out = torch.empty(tuple(t.shape) + (4,), device=self.device, dtype=torch.uint8)
        _lib.check(self.lib.uad_render_heatmap(_ptr(t), t.shape[0], t.shape[1], t.shape[2], _ptr(lut_d), _ptr(out), self._stream()))
        return out

    def render_overlay(self, x, pred, gt):
        """image_utils.augment_prediction_and_groundtruth_to_image (utils/Evaluation.py:501-507) for a [n,h,w] batch on the device
        (uad_render_overlay): x the image, pred the thresholded prediction (non-zero = set), gt the label map (non-zero = set) -> uint8 device
        tensor [n,h,w,3] with the bytes of utils/render.py's overlay_rgb (not the reference's all-black cv2.normalize call: a stated
        deviation)."""
        t = self._f32_batch(x, 'x')
        p = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(pred) != 0, np.float32))
        p = self._f32_batch(p, 'pred', t.shape)
        g = gt if isinstance(gt, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(gt) != 0, np.uint8))
        g = (g.to(self.device) != 0).to(torch.uint8)
        if g.dim() == 4 and g.shape[3] == 1:
            g = g[..., 0]
        if tuple(g.shape) != tuple(t.shape):
            raise ValueError(f'gt must have the shape of x {tuple(t.shape)}, got {tuple(g.shape)}')
        g = g.contiguous()
        out = torch.empty(tuple(t.shape) + (3,), device=self.device, dtype=torch.uint8)
        _lib.check(self.lib.uad_render_overlay(_ptr(t), _ptr(p), _ptr(g), t.shape[0], t.shape[1] * t.shape[2], _ptr(out), self._stream()))
        return out

    # ---------------------------------------------------------------- order statistics (csrc/uad_select.hip)
    def _f32_exact(self, values):
        """-> contiguous fp32 device tensor of a float32 / float64 array or tensor; ValueError when a float64 value is not a float32 number."""
        if isinstance(values, torch.Tensor):
            if values.dtype == torch.float64:
                f = values.to(torch.float32)
                if not bool((f.to(torch.float64) == values).all()):
                    raise ValueError('float64 values that float32 cannot represent: the device order statistics would not equal numpy')
                values = f
            elif values.dtype != torch.float32:
                raise TypeError(f'order statistics take float32 or float64 values, got {values.dtype}')
            return values.to(self.device).contiguous()
        return torch.from_numpy(np.ascontiguousarray(as_float32_exact(values))).to(self.device)

    def select_workspace(self, segments=1):
        """A workspace tensor for select_quantiles calls of up to `segments` segments (any contents; the call initialises it)."""
        nbytes = int(self.lib.uad_select_workspace(int(segments)))
        return torch.empty(max(nbytes // 8, 1), device=self.device, dtype=torch.int64)

    def select_quantiles(self, values, fractions, f32_index, segments=None, nonneg_only=False, workspace=None):
        """uad_select_quantiles: per segment (row of values.reshape(segments, -1); None = the whole array) the count m of values that pass
        the filter and, for each fraction q, the order statistics x_(floor v), x_(min(floor v + 1, m - 1)) around v = (m - 1) * q, formed in
        float32 where f32_index[j] (numpy's index type for a float32 fraction) and in float64 otherwise.
        -> (m [n_seg] int64, lo [n_seg,k] float32, hi [n_seg,k] float32) on the host; NaN brackets where m == 0.  NaN-free input."""
        t = self._f32_exact(values)
        n_seg = 1 if segments is None else int(segments)
        k = len(fractions)
        if n_seg < 1 or t.numel() == 0 or t.numel() % n_seg:
            raise ValueError(f'{t.numel()} values do not split into {n_seg} non-empty segments')
        if not 1 <= k <= _lib.SELECT_MAX_Q or len(f32_index) != k:
            raise ValueError(f'1 .. {_lib.SELECT_MAX_Q} fractions with one index type each, got {k} / {len(f32_index)}')
        ws = workspace if workspace is not None else self.select_workspace(n_seg)
        m = torch.empty(n_seg, device=self.device, dtype=torch.int64)
        br = torch.empty((n_seg, 2 * k), device=self.device, dtype=torch.float32)
        q = (C.c_double * k)(*[float(v) for v in fractions])
        mask = sum(1 << j for j, f in enumerate(f32_index) if f)
        _lib.check(self.lib.uad_select_quantiles(_ptr(t), n_seg, t.numel() // n_seg, q, k, mask, _lib.SELECT_NONNEG if nonneg_only else _lib.SELECT_ALL,
                                                 _ptr(m), _ptr(br), _ptr(ws), ws.numel() * ws.element_size(), self._stream()))
        br = br.cpu().numpy()
        return m.cpu().numpy(), br[:, 0::2], br[:, 1::2]

    def histogram_edges(self, values, edges32):
        """uad_histogram_edges: counts [bins] (numpy int64) of edges32[i] <= v < edges32[i + 1], last bin closed, outside values dropped."""
        t = self._f32_exact(values)
        e = torch.from_numpy(np.ascontiguousarray(edges32, np.float32)).to(self.device)
        counts = torch.empty(e.numel() - 1, device=self.device, dtype=torch.int64)
        _lib.check(self.lib.uad_histogram_edges(_ptr(t), t.numel(), _ptr(e), e.numel() - 1, _ptr(counts), self._stream()))
        return counts.cpu().numpy()

    def clamp_scale(self, values, lo=None, hi=None, scale=1.0, out=None):
        """uad_clamp_scale: (v < lo ? lo : v > hi ? hi : v) * scale elementwise in fp32 -> device tensor of values' shape (out may be values)."""
        t = self._dev(values)
        out = torch.empty_like(t) if out is None else out
        _lib.check(self.lib.uad_clamp_scale(_ptr(t), t.numel(), -math.inf if lo is None else float(lo), math.inf if hi is None else float(hi),
                                            float(scale), _ptr(out), self._stream()))
        return out

    # ---------------------------------------------------------------- ordered sums and standardization (csrc/uad_moments.hip)
    def shifted_sums_workspace(self, n):
        """A workspace tensor for shifted_sums / standardize calls over up to n values (any contents)."""
        nbytes = int(self.lib.uad_shifted_sums_workspace(int(n)))
        return torch.empty(max(nbytes // 8, 2), device=self.device, dtype=torch.float64)

    def shifted_sums(self, values, clamp_lo=None, clamp_hi=None, shift=0.0, centre=0.0, workspace=None):
        """uad_shifted_sums: for u = f32(f32(clamp(v) - shift) - centre) -> (sum u, sum f32(u * u)) as Python floats: fp64 sums in the defined
        order of include/uad_hip.h, bit-equal to utils.standardize.shifted_sums.  One pass, one 16-byte synchronising download."""
        t = self._dev(values).reshape(-1)
        ws = workspace if workspace is not None else self.shifted_sums_workspace(t.numel())
        if not isinstance(ws, torch.Tensor) or ws.device != t.device or not ws.is_contiguous():
            raise ValueError(f'workspace must be a contiguous tensor on {t.device} (shifted_sums_workspace gives one)')
        sums = torch.empty(2, device=self.device, dtype=torch.float64)
        _lib.check(self.lib.uad_shifted_sums(_ptr(t), t.numel(), -math.inf if clamp_lo is None else float(clamp_lo),
                                             math.inf if clamp_hi is None else float(clamp_hi), float(shift), float(centre), _ptr(sums), _ptr(ws),
                                             ws.numel() * ws.element_size(), self._stream()))
        s = sums.cpu().numpy()
        return float(s[0]), float(s[1])

    last_moments = None                # (mean32, std32) of the latest standardize call on this object; None before the first

    def standardize(self, values, clamp_lo=None, clamp_hi=None, out=None, return_moments=False):
        """NII.normalize('standardization') of utils/NII.py:53-75 behind given clamp bounds (None = no bound), on the device: three shifted_sums
        launches -- sum v, sum c, sum e^2, each read back and rounded to float32 once (utils.standardize.moments_from) -- and one
        uad_clamp_standardize pass, out = (clamp(v) - mean32) / std32 -> fp32 device tensor of values' shape.  out: None, or a contiguous fp32
        tensor on this device with values' number of elements (it may be `values` itself); anything else raises ValueError.
        return_moments: -> (out, (mean32, std32)), the way to get the scalars of THIS call; they also stay in self.last_moments, which the
        next call on this object overwrites, whatever stream or caller it comes from.  Bit-equal to utils.standardize.standardize_clamped."""
        from .utils.standardize import moments_from
        t = self._dev(values)
        if out is None:
            out = torch.empty_like(t)
        elif (not isinstance(out, torch.Tensor) or out.device != t.device or out.dtype != torch.float32 or not out.is_contiguous()
              or out.numel() != t.numel()):
            raise ValueError(f'out must be a contiguous float32 tensor of {t.numel()} elements on {t.device}, got '
                             f'{(out.dtype, tuple(out.shape), str(out.device), out.is_contiguous()) if isinstance(out, torch.Tensor) else type(out).__name__}')
        ws = self.shifted_sums_workspace(t.numel())
        mean32, std32 = moments_from(lambda shift, centre: self.shifted_sums(t, clamp_lo, clamp_hi, shift, centre, workspace=ws), t.numel())
        self.last_moments = (mean32, std32)
        _lib.check(self.lib.uad_clamp_standardize(_ptr(t), t.numel(), -math.inf if clamp_lo is None else float(clamp_lo),
                                                  math.inf if clamp_hi is None else float(clamp_hi), float(mean32), float(std32), _ptr(out), self._stream()))
        return (out, (mean32, std32)) if return_moments else out

    # ---------------------------------------------------------------- per-class histograms (csrc/uad_select.hip, csrc/uad_hist.hip)
    def _class_ids(self, ids, n):
        """-> contiguous uint8 device tensor [n] of class ids (a numpy array or a tensor of any integer type)."""
        t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ids))
        t = t.reshape(-1).to(self.device).to(torch.uint8).contiguous()
        if t.numel() != n:
            raise ValueError(f'{t.numel()} class ids for {n} values')
        return t

    def select_quantiles_masked(self, values, ids, class_id, lo32, hi32, fractions, f32_index, workspace=None):
        """uad_select_quantiles_masked: select_quantiles of the values v with ids == class_id and lo32 <= v <= hi32 (float32 bounds).
        -> (m int, lo [k] float32, hi [k] float32) on the host; NaN brackets when m == 0."""
        t = self._f32_exact(values).reshape(-1)
        lab = self._class_ids(ids, t.numel())
        k = len(fractions)
        if t.numel() == 0:
            raise ValueError('no values to select from')
        if not 1 <= k <= _lib.SELECT_MAX_Q or len(f32_index) != k:
            raise ValueError(f'1 .. {_lib.SELECT_MAX_Q} fractions with one index type each, got {k} / {len(f32_index)}')
        ws = workspace if workspace is not None else self.select_workspace(1)
        m = torch.empty(1, device=self.device, dtype=torch.int64)
        br = torch.empty(2 * k, device=self.device, dtype=torch.float32)
        q = (C.c_double * k)(*[float(v) for v in fractions])
        mask = sum(1 << j for j, f in enumerate(f32_index) if f)
        _lib.check(self.lib.uad_select_quantiles_masked(_ptr(t), _ptr(lab), t.numel(), int(class_id), float(lo32), float(hi32), q, k, mask, _ptr(m), _ptr(br),
                                                        _ptr(ws), ws.numel() * ws.element_size(), self._stream()))
        br = br.cpu().numpy()
        return int(m.cpu().numpy()[0]), br[0::2], br[1::2]

    def histogram_workspace(self, n):
        """A workspace tensor for histogram_by_class calls over up to n values (any contents)."""
        nbytes = int(self.lib.uad_histogram_by_class_workspace(int(n)))
        return torch.empty(max(nbytes // 8, 2), device=self.device, dtype=torch.int64)

    def histogram_by_class(self, values, ids, n_classes, edges32=None, centre=None, moments=True, workspace=None):
        """uad_histogram_by_class, nothing downloaded: (counts int64 [n_classes, bins] or None without edges32, class_count int64 [n_classes],
        sums float64 [n_classes]) as DEVICE tensors (the last two None with moments=False).  sums = sum of v per class, or with centre (float64
        [n_classes], device tensor or array) the sum of (v - centre[c])^2, over all values of the class.  A table of more than
        HISTOGRAM_MAX_BINS bins is counted in chunks of that many, one launch each: a chunk that is not the last gets its last edge lowered by
        one float32 ulp, which closes it exactly where the next one opens."""
        t = self._f32_exact(values).reshape(-1)
        n, k = t.numel(), int(n_classes)
        lab = self._class_ids(ids, n)
        bins = 0 if edges32 is None else len(edges32) - 1
        if bins == 0 and not moments:
            raise ValueError('neither a histogram nor moments asked for')
        cen = None
        if centre is not None:
            cen = (centre if isinstance(centre, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centre, np.float64))).to(self.device, torch.float64).contiguous()
            if cen.numel() != k:
                raise ValueError(f'{cen.numel()} centres for {k} classes')
        cnt = torch.empty(k, device=self.device, dtype=torch.int64) if moments else None
        sums = torch.empty(k, device=self.device, dtype=torch.float64) if moments else None
        ws = None
        if moments:
            ws = workspace if workspace is not None else self.histogram_workspace(n)
        ws_bytes = 0 if ws is None else ws.numel() * ws.element_size()
        if bins == 0:
            _lib.check(self.lib.uad_histogram_by_class(_ptr(t), _ptr(lab), n, k, None, 0, _ptr(cen), None, _ptr(cnt), _ptr(sums), _ptr(ws), ws_bytes, self._stream()))
            return None, cnt, sums
        e = np.ascontiguousarray(edges32, np.float32)
        counts = torch.empty((k, bins), device=self.device, dtype=torch.int64)
        step = _lib.HISTOGRAM_MAX_BINS
        for c0 in range(0, bins, step):
            nb = min(step, bins - c0)
            sub = e[c0:c0 + nb + 1].copy()
            if c0 + nb < bins:
                sub[-1] = np.nextafter(sub[-1], np.float32(-np.inf))
            ed = torch.from_numpy(sub).to(self.device)
            part = counts if nb == bins else torch.empty((k, nb), device=self.device, dtype=torch.int64)
            first = c0 == 0 and moments
            _lib.check(self.lib.uad_histogram_by_class(_ptr(t), _ptr(lab), n, k, _ptr(ed), nb, _ptr(cen), _ptr(part), _ptr(cnt) if first else None,
                                                       _ptr(sums) if first else None, _ptr(ws) if first else None, ws_bytes if first else 0, self._stream()))
            if part is not counts:
                counts[:, c0:c0 + nb] = part
        return counts, cnt, sums

    def labelled_histogram(self, values, labels, bins, range, as_dtype=None):
        """utils.histograms.labelled_histograms(values, labels, bins, range) -- the reference's plot_histogram_with_labels (utils/utils.py:44-71)
        -- on the device: [{'class', 'n', 'bins', 'mean', 'var'}] per class of np.unique(labels).  values: a device fp32 tensor, or a float32 /
        float64 array whose values are float32 numbers (ValueError otherwise); labels: a numpy array or a tensor of values' shape (the unique
        classes and the uint8 class ids are formed on the host and uploaded once).  bins: 'auto', an integer or an edge array.  as_dtype: the
        numpy dtype the statement would see (default: that of `values`) -- it decides the type of the edges and of the range test, exactly
        as in numpy; float64 for fp32 residuals whose host copy is float64.  'auto' takes one masked select (class 0 inside the range) and
        the host half utils.histograms.auto_bin_count; then two histogram launches (sums, then counts and centred squares) and ONE download.
        Counts and edges are numpy's exactly; mean and var are two-pass fp64 sums in a fixed order (utils.histograms.TooManyBins above
        MAX_DEVICE_BINS bins: the caller takes the host statement)."""
        import operator
        from .utils import histograms as H
        from .utils.order_stats import edges_to_float32, value_dtype
        dtype = np.dtype(as_dtype) if as_dtype is not None else value_dtype(values)
        if dtype not in (np.float32, np.float64):
            raise TypeError(f'histograms take float32 or float64 values, got {dtype}')
        t = self._f32_exact(values).reshape(-1)
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if lab.size != t.numel():
            raise ValueError(f'{lab.size} labels for {t.numel()} values')
        classes, ids = H.class_ids(lab)
        k = classes.size
        if k == 0:
            return []
        ids = self._class_ids(ids, t.numel())
        if isinstance(bins, str):
            if bins != 'auto':
                raise ValueError(f"bins: 'auto', an integer or an edge array, got {bins!r}")
            first, last = H.outer_edges(range)
            lo32, hi32 = H.range_to_float32(first, last, dtype)
            m, lo, hi = self.select_quantiles_masked(t, ids, 0, lo32, hi32, H.AUTO_Q, [False] * len(H.AUTO_Q))
            n_bins = H.auto_bin_count(m, lo[0], hi[3], (lo[1], hi[1]), (lo[2], hi[2]), range, dtype)
            if n_bins > H.MAX_DEVICE_BINS:
                raise H.TooManyBins(n_bins)
            edges = H.equal_bin_edges(n_bins, range, dtype)
        elif np.ndim(bins) == 0:
            if operator.index(bins) > H.MAX_DEVICE_BINS:
                raise H.TooManyBins(operator.index(bins))
            edges = H.equal_bin_edges(operator.index(bins), range, dtype)
        else:
            edges = np.asarray(bins)
            if edges.ndim != 1 or edges.size < 2 or np.any(edges[:-1] > edges[1:]):
                raise ValueError('`bins` must be 1d and increase monotonically, when an array')
            if edges.size - 1 > H.MAX_DEVICE_BINS:
                raise H.TooManyBins(edges.size - 1)
        ws = self.histogram_workspace(t.numel())
        _, cnt, sums = self.histogram_by_class(t, ids, k, workspace=ws)
        mean = sums / cnt.to(torch.float64)                           # k fp64 divisions, on the device: no download between the launches
        counts, _, sq = self.histogram_by_class(t, ids, k, edges32=edges_to_float32(edges), centre=mean, workspace=ws)
        var = sq / cnt.to(torch.float64)
        flat = torch.cat([counts.reshape(-1), mean.view(torch.int64), var.view(torch.int64)]).cpu().numpy()
        nb = edges.size - 1
        n = flat[:k * nb].reshape(k, nb).astype(np.float64)
        mean, var = flat[k * nb:k * nb + k].view(np.float64), flat[k * nb + k:].view(np.float64)
        return [{'class': c, 'n': n[i], 'bins': edges, 'mean': mean[i], 'var': var[i]} for i, c in enumerate(classes)]

    def scores(self, predictions, labels):
        """One descending device sort of all voxel scores -> Scores object (AUROC, AUPRC, dice at thresholds)."""
        return Scores(self, predictions, labels)

    def residual(self, x, x_rec, mask=None, pos_only=True, prior_thresh=None):
        """Residual anomaly map on device (utils/Evaluation.py:282-289).  Returns (map, l1err_per_sample)."""
        x = self._dev(x)
        xr = self._dev(x_rec, x.shape)
        mk = self._dev(mask, x.shape) if mask is not None else None
        n = x.shape[0]
        hw = int(np.prod(x.shape[1:]))
        out = torch.empty_like(x)
        l1 = torch.empty(n, device=self.device)
        thr = -math.inf if prior_thresh is None else float(prior_thresh)
        _lib.check(self.lib.uad_residual(_ptr(x), _ptr(xr), _ptr(mk), n, hw, 1 if pos_only else 0, thr, _ptr(out),
                                         _ptr(l1), self._stream()))
        return out, l1


class Scores:
    """trainers/Metrics.py's threshold metrics from ONE device sort (uad_scores_*): auroc (sklearn roc_curve + auc),
    auprc (sklearn average_precision_score), dice(pred > t, label) for arbitrary thresholds."""

    def __init__(self, engine, predictions, labels):
        self.lib = engine.lib
        self._stream = engine._stream
        p = engine._dev(predictions).reshape(-1)
        if isinstance(labels, torch.Tensor):
            y = labels.to(device=engine.device, dtype=torch.float32).reshape(-1)
        else:
            y = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1) != 0, np.float32)).to(engine.device)
        if p.numel() != y.numel():
            raise ValueError(f'predictions ({p.numel()}) and labels ({y.numel()}) differ in size')
        h = C.c_void_p()
        _lib.check(self.lib.uad_scores_create(_ptr(p), _ptr(y), p.numel(), C.byref(h), self._stream()))
        self.handle = h
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self.lib.uad_scores_auc(h, C.byref(a), C.byref(b), C.byref(c)))
        self.auroc, self.auprc, self.positives = a.value, b.value, c.value

    def dice_at(self, thresholds):
        t = np.ascontiguousarray(np.atleast_1d(thresholds), np.float64)
        out = np.empty_like(t)
        _lib.check(self.lib.uad_scores_dice(self.handle, t.ctypes.data_as(C.POINTER(C.c_double)), t.size,
                                            out.ctypes.data_as(C.POINTER(C.c_double)), self._stream()))
        return out

    def threshold_at_precision(self, precision):
        """The threshold of the first point of Metrics.compute_prc's curve (increasing threshold) whose precision is <= `precision`:
        thr[np.argmax(prec <= precision)] (utils/Evaluation.py:439)."""
        t = C.c_double()
        _lib.check(self.lib.uad_scores_threshold_at_precision(self.handle, float(precision), C.byref(t)))
        return t.value

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.uad_scores_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
