// 8-bit rendering of the evaluation sample images on the device (utils/Evaluation.py:302-321, 501-507: the grey PNGs through
// normalize_and_squeeze = cv2.normalize(NORM_MINMAX) + astype('uint8'), the squashed jet heat map with its colour bar, the TP / FP / FN
// overlay of image_utils.augment_prediction_and_groundtruth_to_image), so that one to four bytes per pixel go back to the host instead of
// fp32 volumes.  The arithmetic is utils/render.py's, operation for operation: fp64 scale and shift and an fp32 two-rounding map for the
// grey images, an fp64 chain for the heat map; this file is compiled with -ffp-contract=off (build.py) and carries the pragma below, so no
// multiply-add is fused and host and device agree bit for bit -- except through exp(), the one function whose last place may differ
// between the device library and the host's.  The min-max statement restates OpenCV's documented arithmetic and has not been compared with
// OpenCV's own output (OpenCV is not a dependency).
//
// minmax_u8_kernel / heatmap_kernel: both need a slice's minimum and maximum before its first pixel can be written.  One
//   workgroup owns a slice (grid = min(n, RN_MAX_GRID), further slices in a loop).  A thread owns the quads (four consecutive pixels)
//   i * THREADS + tid.  Where the slice fits -- hw <= THREADS * RN_Q * 4 -- the quads stay in registers between the two sweeps and the
//   slice is read from HBM once: 256 threads hold up to 128 x 128, 1024 threads up to 256 x 256 (64 data registers a lane).  Larger slices
//   are read twice by their workgroup; the second read is expected to hit L2.  Loads are 16 bytes where the base is 16-byte aligned and hw
//   a multiple of four, single floats otherwise; grey stores are one dword of four pixels (bytes where hw is no multiple of four or out not
//   4-byte aligned), heat-map stores 16 bytes of four RGBA pixels (dwords otherwise).  The reduction is two barriers: every thread's partial
//   to LDS, RN_FAN threads fold THREADS / RN_FAN of them each, every thread folds the RN_FAN results -- min and max are exact, the order
//   does not matter.  The heat map keeps the fp32 residual and evaluates the fp64 squash twice rather than keeping doubles; its inlined
//   fp64 exp() next to 64 resident registers fits the 512 registers a lane of a 256-thread workgroup may have (256 allocated, no scratch)
//   but not the 128 of a 1024-thread one (the compiler spills 1.1 KB a lane), so the heat map is single-read up to 128 x 128 only and takes
//   the two-sweep form above that: the kernel is bound by the exp() there, not by the second read.
// overlay_kernel: no reduction; the batch is one flat array, a thread owns four pixels: 16-byte loads of image and prediction, one dword of
//   labels, three dwords of RGB (bytes for the last total % 4 pixels, or everywhere when a pointer is not aligned).
// tests/native/render_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co.,
// the launch layer at the end of the file is left out).
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int RN_PX = 4;            // pixels of a quad: one 16-byte load, one dword of grey, 16 bytes of RGBA, three dwords of RGB
constexpr int RN_Q = 16;            // quads a thread keeps in registers on the single-read path (64 fp32 registers)
constexpr int RN_SMALL = 256;       // workgroup of the slices up to RN_SMALL_HW pixels (128 x 128)
constexpr int RN_LARGE = 1024;      // workgroup of the slices up to RN_LARGE_HW pixels (256 x 256) and of the two-sweep path
constexpr int RN_SMALL_HW = RN_SMALL * RN_Q * RN_PX;
constexpr int RN_LARGE_HW = RN_LARGE * RN_Q * RN_PX;
constexpr int RN_FAN = 32;          // second-level fan of the workgroup reduction
constexpr int RN_MAX_GRID = 1024;   // workgroups of one launch: four per CU; slice k is rendered by workgroup k % RN_MAX_GRID
constexpr int OV_THREADS = 256;
static_assert(RN_SMALL >= 256 && RN_SMALL % RN_FAN == 0 && RN_LARGE % RN_FAN == 0, "the colour table is loaded by 256 threads");

// the reduction scratch.  At namespace scope so that the host emulation can poison it between workgroups.
struct GreyLds {
    float lo[RN_LARGE], hi[RN_LARGE];
    float lo2[RN_FAN], hi2[RN_FAN];
};
struct HeatLds {
    double lo[RN_LARGE], hi[RN_LARGE];
    double lo2[RN_FAN], hi2[RN_FAN];
    unsigned lut[256];              // the colour table, one little-endian RGBA dword per entry
};
__shared__ GreyLds rn_grey_lds;
__shared__ HeatLds rn_heat_lds;

// minimum and maximum over the workgroup's threads; every thread gets both.  Two barriers; the first also publishes what the threads wrote
// to LDS before the call.  A second call may follow at once: its first-level writes come after this call's last first-level read (barrier
// two), its second-level writes after its own barrier one, which every thread reaches only after its second-level reads here.
template <int THREADS, class T>
__device__ __forceinline__ void rn_block_minmax(T* lo1, T* hi1, T* lo2, T* hi2, T& lo, T& hi) {
    const int tid = threadIdx.x;
    lo1[tid] = lo;
    hi1[tid] = hi;
    __syncthreads();
    if (tid < RN_FAN) {
        T a = lo1[tid], b = hi1[tid];
        for (int k = 1; k < THREADS / RN_FAN; ++k) {
            const T u = lo1[tid + k * RN_FAN], v = hi1[tid + k * RN_FAN];
            a = u < a ? u : a;
            b = v > b ? v : b;
        }
        lo2[tid] = a;
        hi2[tid] = b;
    }
    __syncthreads();
    T a = lo2[0], b = hi2[0];
    for (int k = 1; k < RN_FAN; ++k) {
        const T u = lo2[k], v = hi2[k];
        a = u < a ? u : a;
        b = v > b ? v : b;
    }
    lo = a;
    hi = b;
}

// quad q of a slice of hw pixels; without vec the pixels past the slice's end repeat the quad's first pixel
__device__ __forceinline__ float4 rn_load4(const float* __restrict__ s, int hw, int q, int vec) {
    const int p = q * RN_PX;
    if (vec) return *reinterpret_cast<const float4*>(s + p);
    float4 v;
    v.x = s[p];
    v.y = p + 1 < hw ? s[p + 1] : v.x;
    v.z = p + 2 < hw ? s[p + 2] : v.x;
    v.w = p + 3 < hw ? s[p + 3] : v.x;
    return v;
}

__device__ __forceinline__ void rn_fold(const float4 v, float& lo, float& hi) {
    lo = v.x < lo ? v.x : lo; hi = v.x > hi ? v.x : hi;
    lo = v.y < lo ? v.y : lo; hi = v.y > hi ? v.y : hi;
    lo = v.z < lo ? v.z : lo; hi = v.z > hi ? v.z : hi;
    lo = v.w < lo ? v.w : lo; hi = v.w > hi ? v.w : hi;
}

// float32 -> byte: truncated toward zero, clamped to 0 .. 255 (utils/render.py: _trunc_u8)
__device__ __forceinline__ unsigned rn_u8(float v) {
    const int t = (int)v;
    return (unsigned)(t < 0 ? 0 : (t > 255 ? 255 : t));
}

__device__ __forceinline__ void rn_store_grey(unsigned char* __restrict__ o, int hw, int q, int vec_out, const float4 v, float scale, float shift) {
    const int p = q * RN_PX;
    const unsigned b0 = rn_u8(v.x * scale + shift), b1 = rn_u8(v.y * scale + shift), b2 = rn_u8(v.z * scale + shift), b3 = rn_u8(v.w * scale + shift);
    if (vec_out) {
        *reinterpret_cast<unsigned*>(o + p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
        o[p] = (unsigned char)b0;
        if (p + 1 < hw) o[p + 1] = (unsigned char)b1;
        if (p + 2 < hw) o[p + 2] = (unsigned char)b2;
        if (p + 3 < hw) o[p + 3] = (unsigned char)b3;
    }
}

template <int THREADS, bool RESIDENT>
__global__ __launch_bounds__(THREADS) void minmax_u8_kernel(const float* __restrict__ x, int n, int hw, int vec_in, int vec_out, unsigned char* __restrict__ out) {
    const int tid = threadIdx.x;
    const int quads = (hw + RN_PX - 1) / RN_PX;
    for (long long slice = blockIdx.x; slice < n; slice += gridDim.x) {
        const float* __restrict__ s = x + (size_t)slice * (size_t)hw;
        unsigned char* __restrict__ o = out + (size_t)slice * (size_t)hw;
        float4 r[RESIDENT ? RN_Q : 1];
        float lo = INFINITY, hi = -INFINITY;
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < RN_Q; ++i) {
                const int q = i * THREADS + tid;
                if (q < quads) {
                    r[i] = rn_load4(s, hw, q, vec_in);
                    rn_fold(r[i], lo, hi);
                }
            }
        } else {
            for (int q = tid; q < quads; q += THREADS) rn_fold(rn_load4(s, hw, q, vec_in), lo, hi);
        }
        rn_block_minmax<THREADS>(rn_grey_lds.lo, rn_grey_lds.hi, rn_grey_lds.lo2, rn_grey_lds.hi2, lo, hi);
        // cv2.normalize's scale and shift in fp64, the map in fp32 (utils/render.py: minmax_u8)
        const double diff = (double)hi - (double)lo;
        const double dscale = diff > DBL_EPSILON ? 255.0 / diff : 0.0;
        const double dshift = -(double)lo * dscale;
        const float scale = (float)dscale, shift = (float)dshift;
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < RN_Q; ++i) {
                const int q = i * THREADS + tid;
                if (q < quads) rn_store_grey(o, hw, q, vec_out, r[i], scale, shift);
            }
        } else {
            for (int q = tid; q < quads; q += THREADS) rn_store_grey(o, hw, q, vec_out, rn_load4(s, hw, q, vec_in), scale, shift);
        }
    }
}

// pixel p of an [h,w] slice before the colour map's normalisation: the colour bar i / h in the last column, elsewhere the squash
// 2 * (1 / (1 + exp(-100 d)) - 0.5), in fp64 (utils/render.py: heatmap_index)
__device__ __forceinline__ double rn_heat_q(float d, int p, int h, int w) {
    const int row = p / w;
    if (p - row * w == w - 1) return (double)row / (double)h;
    const double t = -100.0 * (double)d;
    return 2.0 * (1.0 / (1.0 + exp(t)) - 0.5);
}

__device__ __forceinline__ void rn_heat_fold(const float4 v, int hw, int q, int h, int w, double& lo, double& hi) {
    const int p = q * RN_PX;
    const float d[RN_PX] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < RN_PX; ++k) {
        if (p + k < hw) {
            const double t = rn_heat_q(d[k], p + k, h, w);
            lo = t < lo ? t : lo;
            hi = t > hi ? t : hi;
        }
    }
}

__device__ __forceinline__ void rn_store_heat(unsigned char* __restrict__ o, int hw, int q, int h, int w, int vec_out, const float4 v, double lo, double range,
                                              const unsigned* lut) {
    const int p = q * RN_PX;
    const float d[RN_PX] = {v.x, v.y, v.z, v.w};
    unsigned c[RN_PX];
#pragma unroll
    for (int k = 0; k < RN_PX; ++k) {
        c[k] = 0;
        if (p + k < hw) {
            double t = rn_heat_q(d[k], p + k, h, w) - lo;
            if (range != 0.0) t = t / range;
            const int idx = (int)(t * 256.0);                     // matplotlib's Colormap.__call__, N = 256
            c[k] = lut[idx > 255 ? 255 : (idx < 0 ? 0 : idx)];              // (idx < 0: a NaN only; the table is never left)
        }
    }
    if (vec_out) {
        uint4 u;
        u.x = c[0]; u.y = c[1]; u.z = c[2]; u.w = c[3];
        *reinterpret_cast<uint4*>(o + (size_t)p * 4) = u;
    } else {
#pragma unroll
        for (int k = 0; k < RN_PX; ++k)
            if (p + k < hw) *reinterpret_cast<unsigned*>(o + (size_t)(p + k) * 4) = c[k];
    }
}

template <int THREADS, bool RESIDENT>
__global__ __launch_bounds__(THREADS) void heatmap_kernel(const float* __restrict__ d, int n, int h, int w, const unsigned char* __restrict__ lut256x4, int vec_in,
                                                           int vec_out, unsigned char* __restrict__ out) {
    const int tid = threadIdx.x;
    const int hw = h * w;
    const int quads = (hw + RN_PX - 1) / RN_PX;
    unsigned* lut = rn_heat_lds.lut;
    if (tid < 256)                                                // published by the first barrier of the first reduction
        lut[tid] = (unsigned)lut256x4[4 * tid] | ((unsigned)lut256x4[4 * tid + 1] << 8) | ((unsigned)lut256x4[4 * tid + 2] << 16) | ((unsigned)lut256x4[4 * tid + 3] << 24);
    for (long long slice = blockIdx.x; slice < n; slice += gridDim.x) {
        const float* __restrict__ s = d + (size_t)slice * (size_t)hw;
        unsigned char* __restrict__ o = out + (size_t)slice * (size_t)hw * 4;
        float4 r[RESIDENT ? RN_Q : 1];
        double lo = (double)INFINITY, hi = -(double)INFINITY;
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < RN_Q; ++i) {
                const int q = i * THREADS + tid;
                if (q < quads) {
                    r[i] = rn_load4(s, hw, q, vec_in);
                    rn_heat_fold(r[i], hw, q, h, w, lo, hi);
                }
            }
        } else {
            for (int q = tid; q < quads; q += THREADS) rn_heat_fold(rn_load4(s, hw, q, vec_in), hw, q, h, w, lo, hi);
        }
        rn_block_minmax<THREADS>(rn_heat_lds.lo, rn_heat_lds.hi, rn_heat_lds.lo2, rn_heat_lds.hi2, lo, hi);
        const double range = hi - lo;                             // the maximum of q - q.min(): subtraction is monotone
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < RN_Q; ++i) {
                const int q = i * THREADS + tid;
                if (q < quads) rn_store_heat(o, hw, q, h, w, vec_out, r[i], lo, range, lut);
            }
        } else {
            for (int q = tid; q < quads; q += THREADS) rn_store_heat(o, hw, q, h, w, vec_out, rn_load4(s, hw, q, vec_in), lo, range, lut);
        }
    }
}

// one pixel of the overlay as R | G << 8 | B << 16 (utils/render.py: overlay_rgb; 0.5f * 255.0f truncates to 127)
__device__ __forceinline__ unsigned rn_overlay_px(float x, float pred, unsigned gt) {
    const bool p = pred != 0.0f, g = gt != 0u;
    if (p && g) return 255u << 8;                                 // TP (0, 1, 0)
    if (p) return 255u | (127u << 8);                             // FP (1, 0.5, 0)
    if (g) return 255u;                                           // FN (1, 0, 0)
    float v = x < 0.0f ? 0.0f : x;
    v = v > 1.0f ? 1.0f : v;
    const unsigned c = rn_u8(v * 255.0f);
    return c | (c << 8) | (c << 16);
}

// vec != 0: x, pred allow 16-byte loads, gt and out dword accesses; the last total % 4 pixels go byte by byte
__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(const float* __restrict__ x, const float* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                             long long total, int vec, unsigned char* __restrict__ out) {
    const long long stride = (long long)gridDim.x * OV_THREADS;
    const long long first = (long long)blockIdx.x * OV_THREADS + threadIdx.x;
    const long long quads = vec ? total / RN_PX : 0;
    for (long long q = first; q < quads; q += stride) {
        const float4 xv = reinterpret_cast<const float4*>(x)[q];
        const float4 pv = reinterpret_cast<const float4*>(pred)[q];
        const unsigned g = reinterpret_cast<const unsigned*>(gt)[q];
        const unsigned c0 = rn_overlay_px(xv.x, pv.x, g & 0xffu), c1 = rn_overlay_px(xv.y, pv.y, (g >> 8) & 0xffu);
        const unsigned c2 = rn_overlay_px(xv.z, pv.z, (g >> 16) & 0xffu), c3 = rn_overlay_px(xv.w, pv.w, g >> 24);
        unsigned* __restrict__ o = reinterpret_cast<unsigned*>(out) + 3 * q;
        o[0] = c0 | (c1 << 24);                                   // R0 G0 B0 R1
        o[1] = (c1 >> 8) | (c2 << 16);                            // G1 B1 R2 G2
        o[2] = (c2 >> 16) | (c3 << 8);                            // B2 R3 G3 B3
    }
    for (long long i = quads * RN_PX + first; i < total; i += stride) {
        const unsigned c = rn_overlay_px(x[i], pred[i], gt[i]);
        out[3 * i] = (unsigned char)(c & 0xffu);
        out[3 * i + 1] = (unsigned char)((c >> 8) & 0xffu);
        out[3 * i + 2] = (unsigned char)(c >> 16);
    }
}

// the launch geometry (shared with the host emulation)
enum { RN_PATH_SMALL = 0, RN_PATH_LARGE = 1, RN_PATH_SWEEP = 2 };
inline int render_path(long long hw) { return hw <= RN_SMALL_HW ? RN_PATH_SMALL : (hw <= RN_LARGE_HW ? RN_PATH_LARGE : RN_PATH_SWEEP); }
inline int heat_path(long long hw) { return hw <= RN_SMALL_HW ? RN_PATH_SMALL : RN_PATH_SWEEP; }
inline dim3 render_block(int path) { return dim3(path == RN_PATH_SMALL ? RN_SMALL : RN_LARGE); }
inline dim3 render_grid(int n) { return dim3((unsigned)(n < RN_MAX_GRID ? n : RN_MAX_GRID)); }
inline int render_vec_in(const void* x, long long hw) { return (uintptr_t)x % 16 == 0 && hw % RN_PX == 0; }
inline int grey_vec_out(const void* out, long long hw) { return (uintptr_t)out % 4 == 0 && hw % RN_PX == 0; }
inline int heat_vec_out(const void* out, long long hw) { return (uintptr_t)out % 16 == 0 && hw % RN_PX == 0; }
inline int overlay_vec(const void* x, const void* pred, const void* gt, const void* out) {
    return (uintptr_t)x % 16 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)gt % 4 == 0 && (uintptr_t)out % 4 == 0;
}
inline dim3 overlay_grid(long long total) {
    const long long blocks = (total / RN_PX + OV_THREADS - 1) / OV_THREADS;
    return dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
}

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

extern "C" {

int uad_render_minmax_u8(const float* x, int n, int hw, uint8_t* out, void* stream) {
    if (n < 0 || hw <= 0) return fail(UAD_ERR_INVALID, "render_minmax_u8: n must not be negative and hw positive, got n = %d, hw = %d", n, hw);
    if (n == 0) return UAD_OK;
    if (!x || !out) return fail(UAD_ERR_INVALID, "render_minmax_u8: x / out is NULL");
    if ((const void*)out == (const void*)x) return fail(UAD_ERR_INVALID, "render_minmax_u8: out may not alias x");
    if (hw > INT_MAX - RN_PX) return fail(UAD_ERR_UNSUPPORTED, "render_minmax_u8: a slice of %d pixels is too large", hw);
    const int path = render_path(hw), vi = render_vec_in(x, hw), vo = grey_vec_out(out, hw);
    const dim3 grid = render_grid(n), block = render_block(path);
    const hipStream_t st = (hipStream_t)stream;
    if (path == RN_PATH_SMALL) hipLaunchKernelGGL((minmax_u8_kernel<RN_SMALL, true>), grid, block, 0, st, x, n, hw, vi, vo, out);
    else if (path == RN_PATH_LARGE) hipLaunchKernelGGL((minmax_u8_kernel<RN_LARGE, true>), grid, block, 0, st, x, n, hw, vi, vo, out);
    else hipLaunchKernelGGL((minmax_u8_kernel<RN_LARGE, false>), grid, block, 0, st, x, n, hw, vi, vo, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "render_minmax_u8 launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

int uad_render_heatmap(const float* d, int n, int h, int w, const uint8_t* lut256x4, uint8_t* out_rgba, void* stream) {
    if (n < 0 || h <= 0 || w <= 0) return fail(UAD_ERR_INVALID, "render_heatmap: n must not be negative and h, w positive, got [%d,%d,%d]", n, h, w);
    if (n == 0) return UAD_OK;
    if (!d || !lut256x4 || !out_rgba) return fail(UAD_ERR_INVALID, "render_heatmap: d / lut256x4 / out_rgba is NULL");
    if ((const void*)out_rgba == (const void*)d) return fail(UAD_ERR_INVALID, "render_heatmap: out_rgba may not alias d");
    if ((uintptr_t)out_rgba % 4 != 0) return fail(UAD_ERR_INVALID, "render_heatmap: out_rgba must be 4-byte aligned");
    const long long hw = (long long)h * (long long)w;
    if (hw > INT_MAX - RN_PX) return fail(UAD_ERR_UNSUPPORTED, "render_heatmap: a slice of %d x %d pixels is too large", h, w);
    const int path = heat_path(hw), vi = render_vec_in(d, hw), vo = heat_vec_out(out_rgba, hw);
    const dim3 grid = render_grid(n), block = render_block(path);
    const hipStream_t st = (hipStream_t)stream;
    if (path == RN_PATH_SMALL) hipLaunchKernelGGL((heatmap_kernel<RN_SMALL, true>), grid, block, 0, st, d, n, h, w, lut256x4, vi, vo, out_rgba);
    else hipLaunchKernelGGL((heatmap_kernel<RN_LARGE, false>), grid, block, 0, st, d, n, h, w, lut256x4, vi, vo, out_rgba);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "render_heatmap launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

int uad_render_overlay(const float* x, const float* pred, const uint8_t* gt, int n, int hw, uint8_t* out_rgb, void* stream) {
    if (n < 0 || hw <= 0) return fail(UAD_ERR_INVALID, "render_overlay: n must not be negative and hw positive, got n = %d, hw = %d", n, hw);
    if (n == 0) return UAD_OK;
    if (!x || !pred || !gt || !out_rgb) return fail(UAD_ERR_INVALID, "render_overlay: x / pred / gt / out_rgb is NULL");
    if ((const void*)out_rgb == (const void*)x || (const void*)out_rgb == (const void*)pred || (const void*)out_rgb == (const void*)gt)
        return fail(UAD_ERR_INVALID, "render_overlay: out_rgb may not alias an input");
    const long long total = (long long)n * (long long)hw;
    hipLaunchKernelGGL(overlay_kernel, overlay_grid(total), dim3(OV_THREADS), 0, (hipStream_t)stream, x, pred, gt, total, overlay_vec(x, pred, gt, out_rgb), out_rgb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "render_overlay launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
