// Batch assembly with its two per-batch host stages on the device: the context-encoder masking of trainers/CE.py:123-139 (called by CE.py:77
// and ceVAE.py:93 on every step of every phase) and the instance noise of the loaders' next_batch (dataloaders/BRAINWEB.py:459, MSLUB.py:468:
// batch + numpy.random.normal(0, 0.01, shape) under Options.addInstanceNoise).  The draw of the squares stays on the host (Python's
// `random`, as the reference draws them); what moves is everything that touched the pixels.
//
// brain_boxes_kernel<T>: the bounding box of the non-zero pixels of each slice -- the numbers CE.py:124-126 takes from np.argwhere --
//   as int32 (row_min, row_max, col_min, col_max), both ends inclusive, (-1, -1, -1, -1) for a slice without a non-zero pixel.  T = unsigned
//   char: a label store [N, H*W] read through a 256-entry LUT in LDS (the uad_gather_mask convention, LUT NULL = the label value); T = float:
//   a mask [N, H, W] (non-zero = set, so a NaN counts and -0.0 does not, as numpy's truth value).  One workgroup of BB_THREADS threads per
//   slice: scalar reads up to the first 16-byte boundary of the slice, 16-byte reads over its aligned middle, scalar reads over the rest --
//   nothing is read past the slice, whatever its base and length; a thread keeps four integers, which are reduced through LDS.  Integer
//   min / max: the result does not depend on the order.  Run once over a whole label store (utils/slice_cache.DeviceDataset.brain_boxes).
// assemble_kernel, one launch: out_x[b] = src[idx ? idx[b] : b] (+ sigma * N(0,1)), out_ce[b] = out_x[b] * m_b with m_b = 0 inside any of
//   sample b's up to three windows (r, c, h, w; h == 0 = unused; all channels) and 1 elsewhere.  grid.y = sample, a bounded grid.x with a
//   stride loop over the sample's element quads (gather_slices_kernel's geometry): one 16-byte read of each source quad, one 16-byte store
//   per output.  A quad may straddle a window edge or a row end, so the mask is decided per element.  The product is an fp32 multiply by
//   0.0f / 1.0f -- the host statement is batch * mask: a negative pixel under a square becomes -0.0, a NaN stays a NaN -- and without noise
//   out_x holds the source words.  The noise is uad_rng_fill's, kind UAD_RNG_NORMAL (uad_kernels.h: uad_rng_quad, uad_box_muller): the
//   value at element e of sample b is what uad_rng_fill writes there for the same (seed, step, sample0, stream id), added as
//   x + (sigma * n) in fp32; this file is compiled with -ffp-contract=off (build.py) and carries the pragma below, so nothing is fused.
// tests/native/batch_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co.,
// the launch layer at the end of the file is left out).
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "uad_kernels.h"      // under UAD_HOST_EMULATION: the generator alone
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int BB_THREADS = 256;        // four waves; also the size of the LUT, one entry a thread
constexpr int AB_THREADS = 256;
constexpr int AB_MAX_BLOCKS_X = 64;    // gather_slices_kernel's bound
constexpr int AB_WINDOWS = 3;          // CE.py:131: rng.randint(1, 3) squares a sample

// LDS of brain_boxes_kernel.  At namespace scope so that the host emulation can poison it between workgroups.
struct BoxesLds {
    int red[4][BB_THREADS];
    unsigned char lut[256];
};
__shared__ BoxesLds bb_lds;

struct Box { int r0, r1, c0, c1; };

template <class T> __device__ __forceinline__ bool bb_set(T v);
template <> __device__ __forceinline__ bool bb_set<unsigned char>(unsigned char v) { return bb_lds.lut[v] != 0; }
template <> __device__ __forceinline__ bool bb_set<float>(float v) { return v != 0.0f; }

__device__ __forceinline__ void bb_take(Box& b, int r, int c) {
    b.r0 = r < b.r0 ? r : b.r0; b.r1 = r > b.r1 ? r : b.r1;
    b.c0 = c < b.c0 ? c : b.c0; b.c1 = c > b.c1 ? c : b.c1;
}

template <class T>
__global__ __launch_bounds__(BB_THREADS) void brain_boxes_kernel(const T* __restrict__ in, int H, int W, const unsigned char* __restrict__ lut256,
                                                                 int* __restrict__ boxes) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    if (sizeof(T) == 1) bb_lds.lut[tid] = lut256 ? lut256[tid] : (unsigned char)tid;
    __syncthreads();
    const int px = H * W;                                           // < 2^31: the entry point checks
    const T* __restrict__ s = in + (size_t)blockIdx.x * (size_t)px;
    const int mis = (int)((uintptr_t)s % 16);
    int head = mis ? (16 - mis) / (int)sizeof(T) : 0;               // elements in front of the first 16-byte boundary
    head = head < px ? head : px;
    const int nvec = (px - head) / VEC;
    const int tail0 = head + nvec * VEC;
    Box b{INT_MAX, -1, INT_MAX, -1};
    for (int v = tid; v < nvec; v += BB_THREADS) {
        const int p0 = head + v * VEC;
        const uint4 q = *reinterpret_cast<const uint4*>(s + p0);
        if (sizeof(T) == 4 && (q.x | q.y | q.z | q.w) == 0u) continue;   // four +0.0 floats (a label of 0 may be set under a LUT)
        T e[VEC];
        __builtin_memcpy(e, &q, 16);
        int r = p0 / W, c = p0 - r * W;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (bb_set<T>(e[k])) bb_take(b, r, c);
            if (++c == W) { c = 0; ++r; }
        }
    }
    const int loose = head + (px - tail0);
    for (int i = tid; i < loose; i += BB_THREADS) {
        const int p = i < head ? i : tail0 + (i - head);
        if (bb_set<T>(s[p])) { const int r = p / W; bb_take(b, r, p - r * W); }
    }
    int (&red)[4][BB_THREADS] = bb_lds.red;
    red[0][tid] = b.r0; red[1][tid] = b.r1; red[2][tid] = b.c0; red[3][tid] = b.c1;
    __syncthreads();
    for (int off = BB_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] = red[0][tid + off] < red[0][tid] ? red[0][tid + off] : red[0][tid];
            red[1][tid] = red[1][tid + off] > red[1][tid] ? red[1][tid + off] : red[1][tid];
            red[2][tid] = red[2][tid + off] < red[2][tid] ? red[2][tid + off] : red[2][tid];
            red[3][tid] = red[3][tid + off] > red[3][tid] ? red[3][tid + off] : red[3][tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int* o = boxes + (size_t)blockIdx.x * 4;
        const bool any = red[1][0] >= 0;
        o[0] = any ? red[0][0] : -1; o[1] = any ? red[1][0] : -1; o[2] = any ? red[2][0] : -1; o[3] = any ? red[3][0] : -1;
    }
}

struct AssembleArgs {
    const float* src; const int* idx; const int* rects;
    long long quads;                       // H * W * C / 4
    int W, C;
    float sigma;
    unsigned k0, k1, step_lo, step_hi;
    long long sample0;
    int rng_stream;
    float* out_x; float* out_ce;
};

__global__ __launch_bounds__(AB_THREADS) void assemble_kernel(AssembleArgs a) {
    const int b = blockIdx.y;
    const size_t from = a.idx ? (size_t)a.idx[b] : (size_t)b;
    const float4* __restrict__ s = reinterpret_cast<const float4*>(a.src) + from * (size_t)a.quads;
    float4* __restrict__ ox = a.out_x ? reinterpret_cast<float4*>(a.out_x) + (size_t)b * (size_t)a.quads : nullptr;
    float4* __restrict__ oc = a.out_ce ? reinterpret_cast<float4*>(a.out_ce) + (size_t)b * (size_t)a.quads : nullptr;
    int wr[AB_WINDOWS], wc[AB_WINDOWS], wh[AB_WINDOWS], ww[AB_WINDOWS];
#pragma unroll
    for (int k = 0; k < AB_WINDOWS; ++k) {
        const int* r = a.rects ? a.rects + ((size_t)b * AB_WINDOWS + k) * 4 : nullptr;
        wr[k] = r ? r[0] : 0; wc[k] = r ? r[1] : 0; wh[k] = r ? r[2] : 0; ww[k] = r ? r[3] : 0;
    }
    const unsigned long long gs = (unsigned long long)(a.sample0 + b);
    const long long rowlen = (long long)a.W * a.C;
    for (long long q = (long long)blockIdx.x * AB_THREADS + threadIdx.x; q < a.quads; q += (long long)gridDim.x * AB_THREADS) {
        const float4 in = s[q];
        float v[4] = {in.x, in.y, in.z, in.w};
        if (a.sigma != 0.0f) {
            unsigned r[4];
            float n[4];
            uad_rng_quad((unsigned)q, gs, a.step_lo, a.step_hi, a.rng_stream, a.k0, a.k1, r);
            uad_box_muller(r[0], r[1], n[0], n[1]);
            uad_box_muller(r[2], r[3], n[2], n[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v[k] + a.sigma * n[k];
            if (ox) ox[q] = make_float4(v[0], v[1], v[2], v[3]);
        } else if (ox) {
            ox[q] = in;                                             // the source words
        }
        if (oc) {
            const long long e = q * 4;
            int row = (int)(e / rowlen);
            const int rem = (int)(e - (long long)row * rowlen);
            int col = rem / a.C, ch = rem - col * a.C;
            float m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool in_window = false;
#pragma unroll
                for (int j = 0; j < AB_WINDOWS; ++j)
                    in_window = in_window || (wh[j] > 0 && row >= wr[j] && row < wr[j] + wh[j] && col >= wc[j] && col < wc[j] + ww[j]);
                m[k] = in_window ? 0.0f : 1.0f;
                if (++ch == a.C) { ch = 0; if (++col == a.W) { col = 0; ++row; } }
            }
            oc[q] = make_float4(v[0] * m[0], v[1] * m[1], v[2] * m[2], v[3] * m[3]);
        }
    }
}

// the launch geometry (shared with the host emulation)
inline dim3 boxes_grid(int n) { return dim3((unsigned)n); }
inline dim3 boxes_block() { return dim3(BB_THREADS); }
inline dim3 assemble_grid(int n, long long quads) {
    long long bx = (quads + AB_THREADS - 1) / AB_THREADS;
    bx = bx < 1 ? 1 : (bx > AB_MAX_BLOCKS_X ? AB_MAX_BLOCKS_X : bx);
    return dim3((unsigned)bx, (unsigned)n);
}
inline dim3 assemble_block() { return dim3(AB_THREADS); }
inline AssembleArgs assemble_args(const float* src, const int* idx, int H, int W, int C, const int* rects, float sigma, unsigned long long seed,
                                  unsigned long long step, long long sample0, int rng_stream, float* out_x, float* out_ce) {
    AssembleArgs a;
    a.src = src; a.idx = idx; a.rects = rects;
    a.quads = (long long)H * W * C / 4;
    a.W = W; a.C = C;
    a.sigma = sigma;
    a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32); a.step_lo = (unsigned)step; a.step_hi = (unsigned)(step >> 32);
    a.sample0 = sample0; a.rng_stream = rng_stream;
    a.out_x = out_x; a.out_ce = out_ce;
    return a;
}

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

namespace {
template <class T>
int launch_boxes(const char* what, const T* in, int n, int H, int W, const unsigned char* lut256, int* boxes, void* stream) {
    if (n <= 0 || H <= 0 || W <= 0) return fail(UAD_ERR_INVALID, "%s: sizes must be positive, got [%d,%d,%d]", what, n, H, W);
    if ((long long)H * W > INT_MAX) return fail(UAD_ERR_UNSUPPORTED, "%s: a slice of %d x %d has more than 2^31 - 1 pixels", what, H, W);
    if (!in || !boxes) return fail(UAD_ERR_INVALID, "%s: input / boxes is NULL", what);
    hipLaunchKernelGGL(brain_boxes_kernel<T>, boxes_grid(n), boxes_block(), 0, (hipStream_t)stream, in, H, W, lut256, boxes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
    return UAD_OK;
}
}  // namespace

extern "C" {

int uad_brain_boxes(const unsigned char* labels, int n, int H, int W, const unsigned char* lut256, int* boxes, void* stream) {
    return launch_boxes<unsigned char>("brain_boxes", labels, n, H, W, lut256, boxes, stream);
}

int uad_brain_boxes_f32(const float* masks, int n, int H, int W, int* boxes, void* stream) {
    return launch_boxes<float>("brain_boxes_f32", masks, n, H, W, nullptr, boxes, stream);
}

int uad_assemble_batch(const float* src, const int* idx, int n, int H, int W, int C, const int* rects, float sigma, unsigned long long seed,
                       unsigned long long step, long long sample0, int rng_stream, float* out_x, float* out_ce, void* stream) {
    if (n <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(UAD_ERR_INVALID, "assemble_batch: sizes must be positive, got [%d,%d,%d,%d]", n, H, W, C);
    if (((long long)H * W * C) % 4) return fail(UAD_ERR_INVALID, "assemble_batch: H * W * C (%lld) must be a multiple of 4", (long long)H * W * C);
    if (!(sigma >= 0.0f) || std::isinf(sigma)) return fail(UAD_ERR_INVALID, "assemble_batch: sigma must be finite and >= 0, got %g", (double)sigma);
    if (sample0 < 0) return fail(UAD_ERR_INVALID, "assemble_batch: sample0 must be >= 0");
    if (!src || (!out_x && !out_ce)) return fail(UAD_ERR_INVALID, "assemble_batch: src is NULL, or neither out_x nor out_ce is given");
    if ((out_ce != nullptr) != (rects != nullptr)) return fail(UAD_ERR_INVALID, "assemble_batch: out_ce and rects go together");
    if (out_x == src || out_ce == src || (out_x && out_x == out_ce)) return fail(UAD_ERR_INVALID, "assemble_batch: the outputs may alias neither src nor each other");
    if (n > 65535) return fail(UAD_ERR_UNSUPPORTED, "assemble_batch: at most 65535 samples per call");
    const AssembleArgs a = assemble_args(src, idx, H, W, C, rects, sigma, seed, step, sample0, rng_stream, out_x, out_ce);
    hipLaunchKernelGGL(assemble_kernel, assemble_grid(n, a.quads), assemble_block(), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "assemble_batch launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
