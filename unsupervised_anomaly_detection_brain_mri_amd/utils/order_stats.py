"""Host half of the device order statistics (include/uad_hip.h: uad_select_quantiles, uad_histogram_edges): what numpy does around the
sort, restated so that `engine.quantile` / `percentile` / `histogram` return what np.quantile / np.percentile / np.histogram of the
installed numpy return, value and dtype.

The select op hands back, per segment, m (the values that pass the filter) and for every fraction q the two order statistics that
bracket numpy's 'linear' virtual index (m - 1) * q.  Everything else is numpy's own arithmetic, kept in numpy's own types:
  * the fraction: np.percentile divides q by `a.dtype.type(100)`, np.quantile casts a Python scalar q to a.dtype -- so a float32 array with
    a Python-scalar q gets a FLOAT32 fraction, and `(n - 1) * q` (a Python int times a float32) is a float32 index; an array-valued or
    np.float64 q gives a float64 index and, through gamma, a float64 result even for float32 data;
  * the interpolation: numpy.lib._function_base_impl._lerp -- a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5 -- in the
    result type of (data, gamma).  `lo + (hi - lo) * g` alone is NOT what numpy returns.
`OrderStatOps` is the mixin that turns an object with the three raw ops (select_quantiles, histogram_edges, clamp_scale: device_ops.DeviceOps on
the device, a numpy model in the CPU tests) into one with quantile / percentile / histogram."""
import numpy as np

MAX_Q = 4          # include/uad_hip.h: UAD_SELECT_MAX_Q


def value_dtype(values):
    """numpy dtype of a numpy array or a torch tensor (float32 / float64 only)."""
    dt = np.dtype(str(values.dtype).replace('torch.', '')) if not isinstance(values, np.ndarray) else values.dtype
    if dt not in (np.float32, np.float64):
        raise TypeError(f'order statistics take float32 or float64 values, got {dt}')
    return dt


def as_float32_exact(a):
    """float32 copy of a float32 / float64 numpy array; ValueError when a float64 value is not a float32 number (the device op
    selects among float32 keys, so such an array cannot be held to numpy exactly).  NaN-free input is the op's precondition."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a
    if a.dtype != np.float64:
        raise TypeError(f'order statistics take float32 or float64 values, got {a.dtype}')
    f = a.astype(np.float32)
    if not np.array_equal(f.astype(np.float64), a):
        raise ValueError('float64 values that float32 cannot represent: the device order statistics would not equal numpy')
    return f


def percentile_fractions(q, dtype):
    """np.percentile's own first step (numpy/lib/_function_base_impl.py: percentile)."""
    return np.asanyarray(np.true_divide(q, dtype.type(100) if dtype.kind == 'f' else 100))


def quantile_fractions(q, dtype):
    """np.quantile's own first step."""
    if isinstance(q, (int, float)) and dtype.kind == 'f':
        return np.asanyarray(q, dtype=dtype)
    return np.asanyarray(q)


def _checked_fractions(q):
    if q.ndim > 1:
        raise ValueError('q must be a scalar or 1d')
    if q.dtype not in (np.float32, np.float64):
        raise TypeError(f'q resolves to {q.dtype}: only float32 / float64 fractions are restated here')
    if not (np.all(q >= 0) and np.all(q <= 1)):
        raise ValueError('Quantiles must be in the range [0, 1]')
    if q.size < 1 or q.size > MAX_Q:
        raise ValueError(f'1 .. {MAX_Q} quantiles per call, got {q.size}')
    return q


def lerp(a, b, t):
    """numpy.lib._function_base_impl._lerp."""
    diff_b_a = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff_b_a * t))
    np.subtract(b, diff_b_a * (1 - t), out=out, where=t >= 0.5, casting='unsafe', dtype=type(out.dtype))
    return out


def linear_gamma(m, q):
    """gamma of numpy's method 'linear' for a slice of m values and the fraction q (a 0-d array or numpy scalar of numpy's own type):
    _quantile's virtual index (n - 1) * q, _get_indexes' floor (-1 when the index is at or above the last) and _get_gamma."""
    vi = np.asanyarray((int(m) - 1) * q)
    prev = np.asanyarray(np.floor(vi))
    if vi >= int(m) - 1:
        prev = np.asanyarray(-1, dtype=vi.dtype)
    return np.asanyarray(vi - prev, dtype=vi.dtype)


def finish_linear(m, lo, hi, q, dtype):
    """np.quantile(..., method='linear') from the select op's contract.  m: [n_seg] counts; lo, hi: [n_seg] float32 brackets; q: one
    fraction in numpy's type; dtype: the data's.  -> [n_seg] array in numpy's result type; nan where m == 0."""
    m = np.asarray(m).reshape(-1)
    with np.errstate(invalid='ignore'):
        a, b = np.asarray(lo).astype(dtype).reshape(-1), np.asarray(hi).astype(dtype).reshape(-1)
    out = None
    for mv in np.unique(m):
        sel = m == mv
        r = lerp(a[sel], b[sel], linear_gamma(mv, q)) if mv > 0 else np.full(int(sel.sum()), np.nan, np.result_type(dtype, q.dtype))
        if out is None:
            out = np.empty(m.shape, r.dtype)
        out[sel] = r
    return out


class OrderStatOps:
    """quantile / percentile / histogram over the raw ops of `self`:
      select_quantiles(values, fractions, f32_index, segments=None, nonneg_only=False) -> (m [n_seg] int64, lo [n_seg,k], hi [n_seg,k] float32)
      histogram_edges(values, edges32) -> [bins] int64
    values: a numpy array or torch tensor, float32 or float64 with float32-representable values (ValueError otherwise), NaN-free."""

    def _order_stat(self, values, q, segments, nonneg_only):
        dtype = value_dtype(values)
        scalar = q.ndim == 0
        qs = _checked_fractions(q).reshape(-1)
        m, lo, hi = self.select_quantiles(values, [float(v) for v in qs], [q.dtype == np.float32] * qs.size, segments=segments, nonneg_only=nonneg_only)
        res = np.stack([finish_linear(m, lo[:, j], hi[:, j], qs[j], dtype) for j in range(qs.size)])      # [k, n_seg], as numpy orders it
        if segments is None:
            res = res[:, 0]
        return res[0][()] if scalar else res

    def quantile(self, values, q, segments=None, nonneg_only=False):
        """np.quantile(values, q) (method 'linear') of the whole array, or with segments = n of every row of values.reshape(n, -1);
        nonneg_only: of values[values >= 0] (per row).  q: as numpy takes it, at most 4 entries.  Value AND dtype are numpy's."""
        return self._order_stat(values, quantile_fractions(q, value_dtype(values)), segments, nonneg_only)

    def percentile(self, values, q, segments=None, nonneg_only=False):
        """np.percentile(values, q): see quantile."""
        return self._order_stat(values, percentile_fractions(q, value_dtype(values)), segments, nonneg_only)

    def histogram(self, values, bins, range=None):
        """np.histogram(values, bins=bins, range=range) with an integer `bins` -> (counts int64, edges).  The edges ARE numpy's
        (np.histogram_bin_edges), so its edge rounding is inherited; range=None takes the extremes from one select call."""
        dtype = value_dtype(values)
        if range is None:
            _, lo, hi = self.select_quantiles(values, [0.0, 1.0], [False, False])
            range = (dtype.type(lo[0, 0]), dtype.type(hi[0, 1]))
        edges = np.histogram_bin_edges(np.empty(0, dtype), int(bins), range)
        return self.histogram_edges(values, edges_to_float32(edges)), edges


def edges_to_float32(edges):
    """float32 edge table that bins float32-representable values exactly as the given (float32 or float64) edges do: an inner edge e is
    replaced by the smallest float32 >= e (e <= v  <=>  ceil32(e) <= v for a float32 v), the closed last edge by the largest float32 <= e."""
    e = np.asarray(edges)
    f = e.astype(np.float32)
    if e.dtype == np.float32:
        return f
    e = e.astype(np.float64)
    up = np.where(f.astype(np.float64) < e, np.nextafter(f, np.float32(np.inf)), f)
    last = f[-1] if np.float64(f[-1]) <= e[-1] else np.nextafter(f[-1], np.float32(-np.inf))
    up[-1] = last
    return up.astype(np.float32)
