// Bilinear and nearest-neighbour resize of slices on the device, and the tissue-class masking of a volume: the device pieces of the
// reference's BrainWeb ingestion (dataloaders/BRAINWEB.py:140-142: cv2.resize with the default INTER_LINEAR for the image and INTER_NEAREST
// for the label map of a slice larger than sliceResolution; :266-289: the skull map built from the tissue classes, its multiply and the
// lesion binarisation).
// The resize arithmetic is OpenCV 4.2's resize.cpp for float32 as utils/resize.py states it; that statement has not been compared with
// OpenCV's own output (OpenCV is not a dependency).  Every operation is one IEEE add, multiply or divide in the order of the host
// statement; this file is compiled with -ffp-contract=off (build.py) and carries the pragma below, so that no multiply-add is fused --
// neither in the fp64 coordinate (d + 0.5) * scale - 0.5 nor in the fp32 passes -- and host and device agree bit for bit.
//
// resize_kernel, one launch: a workgroup of RS_THREADS threads owns a tile of RS_TH output rows x RS_TW output columns of
//   one output slice (grid = column tiles x row tiles x n).  Its first RS_TW + RS_TH threads form the per-axis tables of the tile -- tap
//   indices and the fraction -- in LDS with the statement's fp64 divide, multiply, subtract and floor, so that the op needs no upload and
//   no second launch; after one barrier a thread owns four consecutive output pixels of one row: its lanes walk the two source rows in
//   ascending address order (32 lanes cover one tile row, a wave two rows) and it stores 16 bytes where W is a multiple of four and `out`
//   is 16-byte aligned, single floats otherwise.  The horizontal pass of the statement comes first (t = a[x0] w0 + a[x1] w1 on the two
//   source rows), then the vertical one; recomputing t per output row instead of keeping it gives the same bits.  The optional slice
//   gather reads slice_idx[blockIdx.z]; no atomics, a slice's bits depend on neither n nor its place in the batch.
// mask_label_kernel: out = lut256[label] ? vol : 0 and lesion = label == lesion_label in one pass, four elements a thread where the
//   pointers allow 16-byte accesses.
// tests/native/resize_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co.,
// the launch layer at the end of the file is left out).
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS_TW = 128;         // tile width in output columns: 32 lanes x 4 pixels, one 512-byte run of an output row
constexpr int RS_TH = 8;           // tile height in output rows
constexpr int RS_PX = 4;           // output pixels a thread owns (one 16-byte store)
constexpr int RS_THREADS = (RS_TW / RS_PX) * RS_TH;
static_assert(RS_TW + RS_TH <= RS_THREADS, "one thread per table entry");

// one axis of the statement, output sample d of src -> dst: tap indices and the fraction (utils/resize.py: linear_table / nearest_table)
__device__ __forceinline__ void rs_axis(int mode, int d, int src, int dst, int& s0, int& s1, float& frac) {
    const double scale = 1.0 / ((double)dst / (double)src);
    if (mode == UAD_RESIZE_NEAREST) {
        double s = floor((double)d * scale);
        const double top = (double)(src - 1);
        s = s < top ? s : top;
        s0 = s1 = (int)s;
        frac = 0.0f;
        return;
    }
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    long long s = (long long)fl;                   // |f| < 2^32: src, dst are ints
    f = f - fl;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= (long long)src - 1) { s = (long long)src - 1; f = 0.0f; }
    s0 = (int)s;
    s1 = s + 1 < (long long)src - 1 ? (int)(s + 1) : src - 1;
    frac = f;
}

// the per-axis tables of one workgroup's tile.  At namespace scope so that the host emulation can poison them between workgroups: a table
// entry that its own workgroup did not write must never be used.  16-byte aligned: a thread's four entries are one vector LDS read.
struct ResizeTables {
    alignas(16) int x0[RS_TW];
    alignas(16) int x1[RS_TW];
    alignas(16) float fx[RS_TW];
    alignas(16) int y0[RS_TH];
    int y1[RS_TH];
    float fy[RS_TH];
};
__shared__ ResizeTables rs_lds;

__global__ __launch_bounds__(RS_THREADS) void resize_kernel(const float* __restrict__ in, int h, int w, const int* __restrict__ slice_idx, int H, int W,
                                                            int mode, int vec4, float* __restrict__ out) {
    int (&tx0)[RS_TW] = rs_lds.x0, (&tx1)[RS_TW] = rs_lds.x1, (&ty0)[RS_TH] = rs_lds.y0, (&ty1)[RS_TH] = rs_lds.y1;
    float (&tfx)[RS_TW] = rs_lds.fx, (&tfy)[RS_TH] = rs_lds.fy;
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * RS_TW, Y0 = blockIdx.y * RS_TH;
    if (tid < RS_TW) {
        const int X = X0 + tid;
        if (X < W) rs_axis(mode, X, w, W, tx0[tid], tx1[tid], tfx[tid]);
    } else if (tid < RS_TW + RS_TH) {
        const int k = tid - RS_TW, Y = Y0 + k;
        if (Y < H) rs_axis(mode, Y, h, H, ty0[k], ty1[k], tfy[k]);
    }
    __syncthreads();
    const int ly = tid / (RS_TW / RS_PX), lx = (tid - ly * (RS_TW / RS_PX)) * RS_PX;
    const int Y = Y0 + ly, X = X0 + lx;
    if (Y >= H || X >= W) return;
    const size_t src_slice = slice_idx ? (size_t)slice_idx[blockIdx.z] : (size_t)blockIdx.z;
    const float* __restrict__ a = in + src_slice * (size_t)h * (size_t)w;
    const float* __restrict__ r0 = a + (size_t)ty0[ly] * (size_t)w;
    const float* __restrict__ r1 = a + (size_t)ty1[ly] * (size_t)w;
    float* __restrict__ o = out + ((size_t)blockIdx.z * (size_t)H + (size_t)Y) * (size_t)W + (size_t)X;
    float v[RS_PX];
    const int count = W - X < RS_PX ? W - X : RS_PX;
    // the thread's four table entries, one 16-byte LDS read each (entries of columns >= W were never written and are not used)
    const int4 q0 = *reinterpret_cast<const int4*>(&tx0[lx]);
    const int x0[RS_PX] = {q0.x, q0.y, q0.z, q0.w};
    if (mode == UAD_RESIZE_NEAREST) {
#pragma unroll
        for (int k = 0; k < RS_PX; ++k) v[k] = k < count ? r0[x0[k]] : 0.0f;
    } else {
        const int4 q1 = *reinterpret_cast<const int4*>(&tx1[lx]);
        const float4 qf = *reinterpret_cast<const float4*>(&tfx[lx]);
        const int x1[RS_PX] = {q1.x, q1.y, q1.z, q1.w};
        const float fx[RS_PX] = {qf.x, qf.y, qf.z, qf.w};
        const float fy = tfy[ly], wy0 = 1.0f - fy;
#pragma unroll
        for (int k = 0; k < RS_PX; ++k) {
            if (k < count) {
                const float wx0 = 1.0f - fx[k];
                const float t0 = r0[x0[k]] * wx0 + r0[x1[k]] * fx[k];      // the horizontal pass on the two source rows
                const float t1 = r1[x0[k]] * wx0 + r1[x1[k]] * fx[k];
                v[k] = t0 * wy0 + t1 * fy;                          // the vertical pass
            } else {
                v[k] = 0.0f;
            }
        }
    }
    if (vec4) {                                                   // W % 4 == 0: count == 4 and the address is 16-byte aligned
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < RS_PX; ++k)
            if (k < count) o[k] = v[k];
    }
}

constexpr int ML_THREADS = 256;

__shared__ unsigned char ml_lut[256];   // namespace scope for the same reason as rs_lds

// vec4 != 0: all pointers allow 4-element accesses (16 B fp32, 4 B labels); the last n % 4 elements go one by one
__global__ __launch_bounds__(ML_THREADS) void mask_label_kernel(const float* vol, const unsigned char* __restrict__ labels, long long n,
                                                                const unsigned char* __restrict__ lut256, float* out, float* __restrict__ lesion_out,
                                                                int lesion_label, int vec4) {
    unsigned char (&lut)[256] = ml_lut;
    lut[threadIdx.x] = lut256[threadIdx.x];
    __syncthreads();
    const long long stride = (long long)gridDim.x * ML_THREADS;
    const long long first = (long long)blockIdx.x * ML_THREADS + threadIdx.x;
    const long long quads = vec4 ? n / 4 : 0;
    for (long long q = first; q < quads; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(vol)[q];
        const uchar4 l = reinterpret_cast<const uchar4*>(labels)[q];
        reinterpret_cast<float4*>(out)[q] = make_float4(lut[l.x] ? v.x : 0.0f, lut[l.y] ? v.y : 0.0f, lut[l.z] ? v.z : 0.0f, lut[l.w] ? v.w : 0.0f);
        if (lesion_out)
            reinterpret_cast<float4*>(lesion_out)[q] = make_float4(l.x == lesion_label ? 1.0f : 0.0f, l.y == lesion_label ? 1.0f : 0.0f,
                                                                   l.z == lesion_label ? 1.0f : 0.0f, l.w == lesion_label ? 1.0f : 0.0f);
    }
    for (long long i = quads * 4 + first; i < n; i += stride) {
        const int l = labels[i];
        out[i] = lut[l] ? vol[i] : 0.0f;
        if (lesion_out) lesion_out[i] = l == lesion_label ? 1.0f : 0.0f;
    }
}

// the launch geometry (shared with the host emulation)
inline dim3 resize_grid(int n, int H, int W) { return dim3((W + RS_TW - 1) / RS_TW, (H + RS_TH - 1) / RS_TH, n); }
inline dim3 resize_block() { return dim3(RS_THREADS); }
inline int resize_vec4(int W, const void* out) { return W % RS_PX == 0 && (uintptr_t)out % 16 == 0; }
inline dim3 mask_label_grid(long long n) {
    const long long blocks = (n / 4 + ML_THREADS - 1) / ML_THREADS;
    return dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
}
inline int mask_label_vec4(const void* vol, const void* labels, const void* out, const void* lesion_out) {
    return (uintptr_t)vol % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)lesion_out % 16 == 0;
}

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

extern "C" {

int uad_resize2d(const float* in, int n_in, int h, int w, const int* slice_idx, int n, int H, int W, int mode, float* out, void* stream) {
    if (n_in <= 0 || h <= 0 || w <= 0 || n <= 0 || H <= 0 || W <= 0)
        return fail(UAD_ERR_INVALID, "resize2d: sizes must be positive, got [%d,%d,%d] -> [%d,%d,%d]", n_in, h, w, n, H, W);
    if (mode != UAD_RESIZE_LINEAR && mode != UAD_RESIZE_NEAREST) return fail(UAD_ERR_INVALID, "resize2d: unknown mode %d", mode);
    if (!in || !out) return fail(UAD_ERR_INVALID, "resize2d: in / out is NULL");
    if ((const float*)out == in) return fail(UAD_ERR_INVALID, "resize2d: out may not alias in");
    if (!slice_idx && n != n_in) return fail(UAD_ERR_INVALID, "resize2d: without slice_idx n (%d) must equal n_in (%d)", n, n_in);
    const dim3 grid = resize_grid(n, H, W);
    if (grid.y > 65535u || grid.z > 65535u) return fail(UAD_ERR_UNSUPPORTED, "resize2d: [%d,%d,%d] is too large for one grid", n, H, W);
    hipLaunchKernelGGL(resize_kernel, grid, resize_block(), 0, (hipStream_t)stream, in, h, w, slice_idx, H, W, mode, resize_vec4(W, out), out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "resize2d launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

int uad_mask_by_label(const float* vol, const unsigned char* labels, long long n, const unsigned char* lut256, float* out, float* lesion_out,
                      int lesion_label, void* stream) {
    if (n <= 0) return fail(UAD_ERR_INVALID, "mask_by_label: n must be positive, got %lld", n);
    if (!vol || !labels || !lut256 || !out) return fail(UAD_ERR_INVALID, "mask_by_label: vol / labels / lut256 / out is NULL");
    if (lesion_out && (lesion_out == out || (const float*)lesion_out == vol)) return fail(UAD_ERR_INVALID, "mask_by_label: lesion_out may not alias vol / out");
    hipLaunchKernelGGL(mask_label_kernel, mask_label_grid(n), dim3(ML_THREADS), 0, (hipStream_t)stream, vol, labels, n, lut256, out, lesion_out, lesion_label,
                       mask_label_vec4(vol, labels, out, lesion_out));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "mask_by_label launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
