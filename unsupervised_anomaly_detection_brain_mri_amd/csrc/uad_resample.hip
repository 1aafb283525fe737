// Cubic-spline slice resampling on the device: scipy.ndimage.zoom(order=3, prefilter=True, grid_mode=False) per [h,w] slice of a batch
// (reference utils/Evaluation.py:223-232 -- three zoom calls per slice on the host -- and :323-334, the exportVolumes de-zoom), and
// scipy.ndimage.affine_transform(order=3) -- the rotation augmentation of the dataset classes (dataloaders/BRAINWEB.py:156-162) -- on the
// same prefilter: affine_interp_kernel below gathers the 4 x 4 taps at coordinates that are affine in the output pixel.
//   1. zoom_cols_kernel   fp32 -> fp64, edge-replicated padding ('nearest': 12 samples a side), gain 6 and the causal / anticausal
//                         recursion (pole sqrt(3) - 2) along y: one thread per (slice, padded x), coalesced across x.
//   2. zoom_rows_kernel   the same recursion along x: one wave owns 64 rows and walks them in 64-column tiles staged through LDS, so
//                         that global accesses stay row-contiguous; each lane carries its row's recursion state from tile to tile.
//   3. zoom_interp_kernel one thread per output pixel: 4 x 4 taps of the fp64 coefficient plane (L2-resident), fp32 or rounded int32 out.
//   4. affine_interp_kernel  (uad_affine_spline3) the same taps at affine coordinates, K transforms on one prefilter; 16 x 16 output tiles.
// All arithmetic is fp64 and written in scipy's order of operations (ni_splines.c, ni_interpolation.c: NI_ZoomShift) without fused
// multiply-adds, because the integer maps must round as scipy rounds them.  Latency- and bandwidth-shaped work: no matrix cores, no
// atomics (a slice's bits do not depend on the batch around it), vector stores only.
// tests/native/resample_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co.,
// the launch layer at the end of the file is left out), so that their arithmetic is checked against scipy without a GPU.
#include <cmath>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

#define fail uad_fail

namespace {

constexpr int ZOOM_PAD = 12;       // scipy.ndimage._interpolation._prepad_for_spline_filter: npad of mode 'nearest'
constexpr int ZOOM_HORIZON = 48;   // |z|^48 = 3.5e-28: on longer lines the mirrored sum of the causal initial value stops here
constexpr int ZOOM_TILE = 64;
static_assert(ZOOM_HORIZON <= ZOOM_TILE, "the row pass takes its initial value from the first tile");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ni_interpolation.c: the mirror extension of a tap index (NI_ZoomShift's edge offsets), len >= 2
__device__ __forceinline__ int mirror_index(int idx, int len) {
    const int s2 = 2 * len - 2;
    if (idx < 0) {
        idx = s2 * (-idx / s2) + idx;
        idx = idx <= 1 - len ? idx + s2 : -idx;
    } else if (idx >= len) {
        idx -= s2 * (idx / s2);
        if (idx >= len) idx = s2 - idx;
    }
    return idx;
}

// The initial values of the prefilter recursion (ni_splines.c).  PREFILTER_MIRROR: _init_causal_mirror / _init_anticausal_mirror, what
// spline_filter uses for modes 'mirror' and 'constant' and what the zoom op uses on its padded 'nearest' planes too (its coordinates never
// reach the outer padding).  PREFILTER_REFLECT: _init_causal_reflect / _init_anticausal_reflect, what spline_filter(mode='nearest') really
// does to the padded line -- the affine op needs it, because rotated corners do read the outer padding.
enum { PREFILTER_MIRROR = 0, PREFILTER_REFLECT = 1 };

// The causal initial value of a line given by an accessor (already multiplied by the gain); zn = z^(len-1) (mirror) or z^len (reflect).
// len > ZOOM_HORIZON: the terms past the horizon (and every zn term) are below fp64 round-off and are left out.
template <int INIT, class F>
__device__ __forceinline__ double causal_init(F at, int len, double z, double zn) {
    double zi = z;
    if (INIT == PREFILTER_REFLECT) {
        const double c0 = at(0);
        double s;
        if (len > ZOOM_HORIZON) {
            s = c0;
            for (int i = 1; i < ZOOM_HORIZON; ++i) { s += zi * at(i); zi *= z; }
            s *= z;
        } else {
            s = c0 + zn * at(len - 1);
            for (int i = 1; i < len; ++i) { s += zi * (at(i) + zn * at(len - 1 - i)); zi *= z; }
            s *= z / (1 - zn * zn);
        }
        return s + c0;
    }
    if (len > ZOOM_HORIZON) {
        double s = at(0);
        for (int i = 1; i < ZOOM_HORIZON; ++i) { s += zi * at(i); zi *= z; }
        return s;
    }
    double s = at(0) + zn * at(len - 1);
    for (int i = 1; i < len - 1; ++i) { s += zi * (at(i) + zn * at(len - 1 - i)); zi *= z; }
    return s / (1 - zn * zn);
}

// the last sample of the anticausal sweep from the last two of the causal one
template <int INIT>
__device__ __forceinline__ double anticausal_init(double prev2, double prev, double z) {
    return INIT == PREFILTER_REFLECT ? prev * (z / (z - 1)) : (z * prev2 + prev) * z / (z * z - 1);
}

template <int INIT = PREFILTER_MIRROR>
__global__ void __launch_bounds__(256) zoom_cols_kernel(const float* __restrict__ in, int n, int h, int w, int pad, int hp, int wp, double z,
                                                        double zn, double* __restrict__ coef) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)n * wp) return;
    const int slice = (int)(gid / wp), xq = (int)(gid % wp);
    const float* src = in + (size_t)slice * h * w + clampi(xq - pad, 0, w - 1);
    double* dst = coef + (size_t)slice * hp * wp + xq;
    auto at = [&](int yq) { return (double)src[(size_t)clampi(yq - pad, 0, h - 1) * w] * 6.0; };
    double prev = causal_init<INIT>(at, hp, z, zn), prev2 = prev;
    dst[0] = prev;
    for (int y = 1; y < hp; ++y) {
        prev2 = prev;
        prev = at(y) + z * prev;
        dst[(size_t)y * wp] = prev;
    }
    double nxt = anticausal_init<INIT>(prev2, prev, z);
    dst[(size_t)(hp - 1) * wp] = nxt;
    for (int y = hp - 2; y >= 0; --y) {
        nxt = z * (nxt - dst[(size_t)y * wp]);
        dst[(size_t)y * wp] = nxt;
    }
}

// rows: the [n * hp] lines of length wp of the coefficient planes, contiguous.  One wave per 64 rows; tile[r][c] with a leading dimension
// of 65 doubles keeps both the row-wise staging (lane = column) and the recursion (lane = row) free of LDS bank conflicts.
template <int INIT = PREFILTER_MIRROR>
__global__ void __launch_bounds__(ZOOM_TILE) zoom_rows_kernel(double* __restrict__ coef, int rows, int wp, double z, double zn) {
    __shared__ double tile[ZOOM_TILE][ZOOM_TILE + 1];
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * ZOOM_TILE;
    const int nr = rows - r0 < ZOOM_TILE ? rows - r0 : ZOOM_TILE;
    const int ntiles = (wp + ZOOM_TILE - 1) / ZOOM_TILE;
    double* base = coef + (size_t)r0 * wp;
    double prev = 0.0, prev2 = 0.0, nxt = 0.0;
    for (int pass = 0; pass < 2; ++pass) {                       // 0: causal, tiles left to right; 1: anticausal, right to left
        for (int jj = 0; jj < ntiles; ++jj) {
            const int j = pass == 0 ? jj : ntiles - 1 - jj;
            const int c0 = j * ZOOM_TILE;
            const int nc = wp - c0 < ZOOM_TILE ? wp - c0 : ZOOM_TILE;
            const double gain = pass == 0 ? 6.0 : 1.0;           // scipy scales the line by the filter gain before the causal sweep
            if (lane < nc)
                for (int r = 0; r < nr; ++r) tile[r][lane] = base[(size_t)r * wp + c0 + lane] * gain;
            __syncthreads();
            if (lane < nr) {
                double* row = tile[lane];
                if (pass == 0) {
                    int k = 0;
                    if (j == 0) {
                        prev = causal_init<INIT>([&](int i) { return row[i]; }, wp, z, zn);
                        prev2 = prev;
                        row[0] = prev;
                        k = 1;
                    }
                    for (; k < nc; ++k) {
                        prev2 = prev;
                        prev = row[k] + z * prev;
                        row[k] = prev;
                    }
                } else {
                    int k = nc - 1;
                    if (j == ntiles - 1) {
                        nxt = anticausal_init<INIT>(prev2, prev, z);
                        row[k] = nxt;
                        --k;
                    }
                    for (; k >= 0; --k) {
                        nxt = z * (nxt - row[k]);
                        row[k] = nxt;
                    }
                }
            }
            __syncthreads();
            if (lane < nc)
                for (int r = 0; r < nr; ++r) base[(size_t)r * wp + c0 + lane] = tile[r][lane];
            __syncthreads();
        }
    }
}

// NI_ZoomShift for one axis: output sample o -> first tap, the four (mirror-folded) tap indices and the cubic B-spline weights
// (ni_splines.c get_spline_interpolation_weights, order 3)
// Returns false where scipy writes cval: the product o * zoom of the LAST sample can round to just above len - 1 (128 -> 181: 180 * (127 / 180) =
// 127.00000000000001), which mode 'constant' treats as outside the line -- that output column / row is 0 in scipy, and here.  ('nearest' reads
// the padded plane, where the coordinate is inside.)
__device__ __forceinline__ bool zoom_taps(int o, double zoom, int pad, int len, int idx[4], double wt[4]) {
    double cc = (double)o * zoom;
    cc += (double)pad;
    const bool inside = cc <= (double)(len - 1);
    const double fl = floor(cc);
    const int start = (int)fl - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = mirror_index(start + k, len);
    const double y = cc - fl, zc = 1.0 - y;
    wt[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    wt[2] = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0;
    wt[0] = zc * zc * zc / 6.0;
    wt[3] = 1.0 - wt[0] - wt[1] - wt[2];
    return inside;
}

__global__ void __launch_bounds__(256) zoom_interp_kernel(const double* __restrict__ coef, int n, int pad, int hp, int wp, int H, int W, double zy,
                                                          double zx, int out_kind, void* __restrict__ out) {
    const int X = blockIdx.x * 64 + threadIdx.x;
    const int Y = blockIdx.y * 4 + threadIdx.y;
    if (X >= W || Y >= H) return;
    int iy[4], ix[4];
    double wy[4], wx[4];
    const bool inside_y = zoom_taps(Y, zy, pad, hp, iy, wy);
    const bool inside = zoom_taps(X, zx, pad, wp, ix, wx) && inside_y;
    for (int s = blockIdx.z; s < n; s += gridDim.z) {
        const double* c = coef + (size_t)s * hp * wp;
        double t = 0.0;
        if (inside) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double* row = c + (size_t)iy[i] * wp;
#pragma unroll
                for (int j = 0; j < 4; ++j) t += row[ix[j]] * wy[i] * wx[j];
            }
        }
        const size_t o = ((size_t)s * H + Y) * W + X;
        if (out_kind == UAD_ZOOM_I32) ((int*)out)[o] = t > 0 ? (int)(t + 0.5) : (int)(t - 0.5);
        else ((float*)out)[o] = (float)t;
    }
}

inline int zoom_pad(int boundary) { return boundary == UAD_ZOOM_NEAREST ? ZOOM_PAD : 0; }

// ---- affine transforms (NI_GeometricTransform with a matrix and an offset) ----------------------------------------------------------
struct AffineTable { double v[UAD_AFFINE_MAX_K][6]; };      // m00 m01 m10 m11 off0 off1 per transform; a kernel argument (768 bytes)

// One axis of one output pixel: input coordinate c (unpadded) -> whether scipy computes the pixel at all, the four tap indices and the cubic
// weights.  'constant' (pad 0): outside [0, raw - 1] scipy writes cval; inside, taps that step over the edge are mirror-folded.  'nearest':
// the coordinate moves by the padding and is NOT clamped; the tap INDICES are clamped to the padded line (rotated corners do step beyond it).
// The index arithmetic is done on a clamped copy of floor(c) so that no coordinate, however far out (or NaN), overflows the int conversion;
// within 8 samples of the line the copy is floor(c) itself, beyond that all four taps clamp to the same end either way.
__device__ __forceinline__ bool affine_taps(double c, int pad, int raw, int len, int idx[4], double wt[4]) {
    const bool inside = pad != 0 || !(c < 0.0 || c > (double)(raw - 1));
    const double cc = c + (double)pad;
    const double fl = floor(cc);
    const int start = (int)fmin(fmax(fl, -8.0), (double)(len + 8)) - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = pad != 0 ? clampi(start + k, 0, len - 1) : mirror_index(start + k, len);
    const double y = cc - fl, zc = 1.0 - y;
    wt[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    wt[2] = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0;
    wt[0] = zc * zc * zc / 6.0;
    wt[3] = 1.0 - wt[0] - wt[1] - wt[2];
    return inside;
}

// One thread per output pixel of a 16 x 16 tile; a wave is a 16 x 4 block of it, so that its 16 x 64 taps stay within a few rows and columns
// of the (L2-resident) coefficient plane at any angle -- a 64-pixel output row would read along a tilted line 64 samples long.  Coordinates,
// inside test, tap indices and weights are formed once per (pixel, transform) and reused over the slices of the grid-z stride.  The sum is
// scipy's: t += coef * wy * wx, rows outer.  out: [n, K, H, W].
__global__ void __launch_bounds__(256) affine_interp_kernel(const double* __restrict__ coef, int n, int K, int pad, int h, int w, int H, int W,
                                                            AffineTable tab, int out_kind, void* __restrict__ out) {
    const int X = blockIdx.x * 16 + threadIdx.x;
    const int Y = blockIdx.y * 16 + threadIdx.y;
    if (X >= W || Y >= H) return;
    const int hp = h + 2 * pad, wp = w + 2 * pad;
    for (int k = 0; k < K; ++k) {
        const double* m = tab.v[k];
        const double cy = ((double)Y * m[0] + (double)X * m[1]) + m[4];      // the matrix sum first, then the offset: scipy's order
        const double cx = ((double)Y * m[2] + (double)X * m[3]) + m[5];
        int iy[4], ix[4];
        double wy[4], wx[4];
        const bool inside_y = affine_taps(cy, pad, h, hp, iy, wy);
        const bool inside = affine_taps(cx, pad, w, wp, ix, wx) && inside_y;
        for (int s = blockIdx.z; s < n; s += gridDim.z) {
            const double* c = coef + (size_t)s * hp * wp;
            double t = 0.0;
            if (inside) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double* row = c + (size_t)iy[i] * wp;
#pragma unroll
                    for (int j = 0; j < 4; ++j) t += row[ix[j]] * wy[i] * wx[j];
                }
            }
            const size_t o = (((size_t)s * K + k) * H + Y) * W + X;
            if (out_kind == UAD_ZOOM_I32) ((int*)out)[o] = t > 0 ? (int)(t + 0.5) : (int)(t - 0.5);
            else ((float*)out)[o] = (float)t;
        }
    }
}

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
extern "C" {

size_t uad_zoom_spline3_workspace(int n, int h, int w, int boundary) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const int pad = zoom_pad(boundary);
    return (size_t)n * (size_t)(h + 2 * pad) * (size_t)(w + 2 * pad) * sizeof(double);
}

int uad_zoom_spline3(const float* in, int n, int h, int w, int H, int W, int boundary, int out_kind, void* out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!in || !out || !workspace || n <= 0 || H <= 0 || W <= 0) return fail(UAD_ERR_INVALID, "zoom_spline3: bad arguments");
    if (h < 2 || w < 2) return fail(UAD_ERR_INVALID, "zoom_spline3: a line needs at least 2 samples, got %dx%d", h, w);
    if (boundary != UAD_ZOOM_CONSTANT && boundary != UAD_ZOOM_NEAREST) return fail(UAD_ERR_INVALID, "zoom_spline3: unknown boundary %d", boundary);
    if (out_kind != UAD_ZOOM_F32 && out_kind != UAD_ZOOM_I32) return fail(UAD_ERR_INVALID, "zoom_spline3: unknown out_kind %d", out_kind);
    const int pad = zoom_pad(boundary), hp = h + 2 * pad, wp = w + 2 * pad;
    if ((size_t)n * hp > 0x7fffffffULL || (size_t)n * wp > 0x7fffffffULL || (size_t)H * W > 0x7fffffffULL)
        return fail(UAD_ERR_UNSUPPORTED, "zoom_spline3: batch too large");
    if ((H + 3) / 4 > 65535) return fail(UAD_ERR_UNSUPPORTED, "zoom_spline3: output too tall");
    const size_t need = uad_zoom_spline3_workspace(n, h, w, boundary);
    if (workspace_bytes < need) return fail(UAD_ERR_INVALID, "zoom_spline3: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (((size_t)workspace & 15) != 0) return fail(UAD_ERR_INVALID, "zoom_spline3: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* coef = (double*)workspace;
    const double z = std::sqrt(3.0) - 2.0;                      // ni_splines.c get_filter_poles, order 3
    const double zy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 1.0, zx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 1.0;
    const size_t cols = (size_t)n * wp;
    hipLaunchKernelGGL(zoom_cols_kernel<PREFILTER_MIRROR>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, in, n, h, w, pad, hp, wp, z, std::pow(z, hp - 1), coef);
    HIP_TRY(hipGetLastError());
    const int rows = n * hp;
    hipLaunchKernelGGL(zoom_rows_kernel<PREFILTER_MIRROR>, dim3((unsigned)((rows + ZOOM_TILE - 1) / ZOOM_TILE)), dim3(ZOOM_TILE), 0, st, coef, rows, wp, z, std::pow(z, wp - 1));
    HIP_TRY(hipGetLastError());
    const dim3 grid((W + 63) / 64, (H + 3) / 4, n < 65535 ? n : 65535);
    hipLaunchKernelGGL(zoom_interp_kernel, grid, dim3(64, 4), 0, st, (const double*)coef, n, pad, hp, wp, H, W, zy, zx, out_kind, out);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

size_t uad_affine_spline3_workspace(int n, int h, int w, int boundary) { return uad_zoom_spline3_workspace(n, h, w, boundary); }

}  // extern "C"

namespace {
template <int INIT>
int affine_prefilter(const float* in, int n, int h, int w, int pad, double* coef, hipStream_t st) {
    const int hp = h + 2 * pad, wp = w + 2 * pad;
    const double z = std::sqrt(3.0) - 2.0;
    const int e = INIT == PREFILTER_REFLECT ? 0 : 1;           // zn = z^len (reflect) or z^(len-1) (mirror)
    const size_t cols = (size_t)n * wp;
    hipLaunchKernelGGL(zoom_cols_kernel<INIT>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, in, n, h, w, pad, hp, wp, z, std::pow(z, hp - e), coef);
    HIP_TRY(hipGetLastError());
    const int rows = n * hp;
    hipLaunchKernelGGL(zoom_rows_kernel<INIT>, dim3((unsigned)((rows + ZOOM_TILE - 1) / ZOOM_TILE)), dim3(ZOOM_TILE), 0, st, coef, rows, wp, z, std::pow(z, wp - e));
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
}  // namespace

extern "C" {

int uad_affine_spline3(const float* in, int n, int h, int w, int H, int W, const double* xf, int K, int boundary, int out_kind, void* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!in || !out || !workspace || !xf || n <= 0 || H <= 0 || W <= 0) return fail(UAD_ERR_INVALID, "affine_spline3: bad arguments");
    if (h < 2 || w < 2) return fail(UAD_ERR_INVALID, "affine_spline3: a line needs at least 2 samples, got %dx%d", h, w);
    if (K < 1 || K > UAD_AFFINE_MAX_K) return fail(UAD_ERR_INVALID, "affine_spline3: 1 .. %d transforms a call, got %d", UAD_AFFINE_MAX_K, K);
    if (boundary != UAD_ZOOM_CONSTANT && boundary != UAD_ZOOM_NEAREST) return fail(UAD_ERR_INVALID, "affine_spline3: unknown boundary %d", boundary);
    if (out_kind != UAD_ZOOM_F32 && out_kind != UAD_ZOOM_I32) return fail(UAD_ERR_INVALID, "affine_spline3: unknown out_kind %d", out_kind);
    const int pad = zoom_pad(boundary), hp = h + 2 * pad, wp = w + 2 * pad;
    if ((size_t)n * hp > 0x7fffffffULL || (size_t)n * wp > 0x7fffffffULL || (size_t)H * W > 0x7fffffffULL)
        return fail(UAD_ERR_UNSUPPORTED, "affine_spline3: batch too large");
    if ((H + 15) / 16 > 65535) return fail(UAD_ERR_UNSUPPORTED, "affine_spline3: output too tall");
    const size_t need = uad_affine_spline3_workspace(n, h, w, boundary);
    if (workspace_bytes < need) return fail(UAD_ERR_INVALID, "affine_spline3: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (((size_t)workspace & 15) != 0) return fail(UAD_ERR_INVALID, "affine_spline3: workspace must be 16-byte aligned");
    AffineTable tab = {};
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < 6; ++j) {
            if (!std::isfinite(xf[k * 6 + j])) return fail(UAD_ERR_INVALID, "affine_spline3: transform %d has a non-finite entry", k);
            tab.v[k][j] = xf[k * 6 + j];
        }
    hipStream_t st = (hipStream_t)stream;
    double* coef = (double*)workspace;
    const int rc = pad ? affine_prefilter<PREFILTER_REFLECT>(in, n, h, w, pad, coef, st) : affine_prefilter<PREFILTER_MIRROR>(in, n, h, w, pad, coef, st);
    if (rc != UAD_OK) return rc;
    const dim3 grid((W + 15) / 16, (H + 15) / 16, n < 65535 ? n : 65535);
    hipLaunchKernelGGL(affine_interp_kernel, grid, dim3(16, 16), 0, st, (const double*)coef, n, K, pad, h, w, H, W, tab, out_kind, out);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
