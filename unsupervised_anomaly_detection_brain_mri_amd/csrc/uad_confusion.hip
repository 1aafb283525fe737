// Per-segment voxel confusion counts (trainers/Metrics.py: confusion_matrix / dice / precision / recall / tpr / vd, called per patient and over the
// whole test set at utils/Evaluation.py:452-500): for each of P contiguous segments of a flat voxel array, the confusion of pred[i] > thr
// against gt[i] != 0 -- {TP, FP, FN, TN} as int64.  Every scalar of the voxel-wise half of the result dictionary is a function of these four.
//   1. confusion_zero_kernel  counts = 0, in-stream: the call needs no prepared output.
//   2. confusion_kernel     blockIdx.y = segment, blockIdx.x strides over the segment's tiles of CF_TILE values (16-byte loads of the values, dword
//                           loads of the u8 labels where the segment's start allows, guarded scalar head and tail).  Three 32-bit counters per thread
//                           in registers, one tree reduction in LDS per workgroup in a fixed order, three 64-bit integer atomics per workgroup.
//   3. confusion_tn_kernel  one thread a segment: TN = length - TP - FP - FN.
// Integer atomics only: the counts do not depend on the order of arrival, on the grid or on what else runs.  No floating-point atomic, no
// workgroup waits for another, no flags.
// Bytes: one launch reads 4 B (value) + 1 B (label) per voxel of a segment and nothing twice; 16 B of offsets per workgroup, 32 B of counters per segment.
// tests/native/confusion_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co., the
// launch layer at the end of the file is left out).
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

namespace {

constexpr int CF_THREADS = 256, CF_ROUNDS = 8, CF_RUN = 4 * CF_ROUNDS;     // 32 values per thread and tile
constexpr int CF_TILE = CF_THREADS * CF_RUN;                                // 8192 values per tile
constexpr int CF_MAX_BLOCKS = 2048, CF_TILES_PER_BLOCK = 4, CF_MAX_SEGMENTS = 65535;
constexpr long long CF_MAX_N = 0x7fffffffLL;
static_assert(CF_TILE == UAD_SELECT_TILE, "include/uad_hip.h states the tile");

struct CfLds {
    unsigned red[3][CF_THREADS];
};

__shared__ CfLds cf_lds;

// one voxel: v > thr is an ordered comparison (a NaN is not a prediction), a non-zero label byte is lesion
__device__ __forceinline__ void cf_count(float v, unsigned label, float thr, unsigned& tp, unsigned& fp, unsigned& fn) {
    const unsigned p = v > thr ? 1u : 0u, g = label != 0u ? 1u : 0u;
    tp += p & g;
    fp += p & (g ^ 1u);
    fn += (p ^ 1u) & g;
}

// the four labels of a chunk as one word: a dword load where the chunk's address is 4-byte aligned, else four byte loads
__device__ __forceinline__ unsigned cf_labels4(const uint8_t* p, int vec) {
    if (vec) return *reinterpret_cast<const unsigned*>(p);
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

// one thread a counter
__global__ void __launch_bounds__(CF_THREADS) confusion_zero_kernel(int n_segments, unsigned long long* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < (long long)n_segments * 4) counts[i] = 0ull;
}

// pred, gt: n values / label bytes; segment s = [seg_offsets[s], seg_offsets[s + 1]), cut to [0, n] so that a bad table cannot send a load out of
// the arrays.  The tiles of a segment are taken relative to the 16-byte boundary at or below its first value (off = the elements between), so a
// chunk of four that lies wholly inside the segment is one 16-byte load; its labels are one dword where gt + start - off is 4-byte aligned.  A
// segment starts anywhere, so both are decided per segment here, not by the host.  counts [P, 4], zeroed by confusion_zero_kernel.
// A thread sees at most ceil((2^31 + 2) / 8192) * 32 < 2^23 voxels, a workgroup at most 2^31 + 2: the 32-bit counters cannot wrap.
__global__ void __launch_bounds__(CF_THREADS) confusion_kernel(const float* __restrict__ pred, float thr, const uint8_t* __restrict__ gt, long long n,
                                                               const long long* __restrict__ seg_offsets, unsigned long long* __restrict__ counts) {
    CfLds& s = cf_lds;
    const int t = threadIdx.x;
    const unsigned seg = blockIdx.y;
    long long a = seg_offsets[seg], b = seg_offsets[seg + 1];
    if (a < 0) a = 0;
    if (b > n) b = n;
    if (b <= a) return;                                  // an empty segment: uniform over the workgroup, before any barrier
    const float* first = pred + a;
    const unsigned long long off = ((uintptr_t)first >> 2) & 3u;
    const float* aligned = first - off;
    const uint8_t* lab_aligned = gt + a - off;
    const int lab_vec = ((uintptr_t)lab_aligned & 3u) == 0 ? 1 : 0;
    const unsigned long long end = off + (unsigned long long)(b - a);
    const unsigned long long tiles = (end + CF_TILE - 1) / CF_TILE;
    unsigned tp = 0u, fp = 0u, fn = 0u;
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const unsigned long long base = tile * CF_TILE;
        if (base >= off && base + CF_TILE <= end) {      // a tile inside the segment (uniform): the eight loads of a thread are issued together
            float4 x[CF_ROUNDS];
            unsigned w[CF_ROUNDS];
#pragma unroll
            for (int r = 0; r < CF_ROUNDS; ++r) {
                const unsigned long long j0 = base + ((unsigned long long)r * CF_THREADS + t) * 4ull;
                x[r] = *reinterpret_cast<const float4*>(aligned + j0);
                w[r] = cf_labels4(lab_aligned + j0, lab_vec);
            }
#pragma unroll
            for (int r = 0; r < CF_ROUNDS; ++r) {
                cf_count(x[r].x, w[r] & 255u, thr, tp, fp, fn);
                cf_count(x[r].y, (w[r] >> 8) & 255u, thr, tp, fp, fn);
                cf_count(x[r].z, (w[r] >> 16) & 255u, thr, tp, fp, fn);
                cf_count(x[r].w, w[r] >> 24, thr, tp, fp, fn);
            }
            continue;
        }
        for (int r = 0; r < CF_ROUNDS; ++r) {            // the first and the last tile: chunks that leave the segment are read value by value
            const unsigned long long j0 = base + ((unsigned long long)r * CF_THREADS + t) * 4ull;
            if (j0 >= end || j0 + 4 <= off) continue;
            if (j0 >= off && j0 + 4 <= end) {
                const float4 x = *reinterpret_cast<const float4*>(aligned + j0);
                const unsigned w = cf_labels4(lab_aligned + j0, lab_vec);
                cf_count(x.x, w & 255u, thr, tp, fp, fn);
                cf_count(x.y, (w >> 8) & 255u, thr, tp, fp, fn);
                cf_count(x.z, (w >> 16) & 255u, thr, tp, fp, fn);
                cf_count(x.w, w >> 24, thr, tp, fp, fn);
            } else {
                for (int e = 0; e < 4; ++e)
                    if (j0 + e >= off && j0 + e < end) cf_count(aligned[j0 + e], lab_aligned[j0 + e], thr, tp, fp, fn);
            }
        }
    }
    // the 256 runs added as a tree: level d adds run t + d to run t for t < d, d = 128, 64, ... 1
    s.red[0][t] = tp; s.red[1][t] = fp; s.red[2][t] = fn;
    for (int d = CF_THREADS / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (t < d)
            for (int c = 0; c < 3; ++c) s.red[c][t] += s.red[c][t + d];
    }
    __syncthreads();
    if (t < 3 && s.red[t][0]) atomicAdd(&counts[(size_t)seg * 4 + t], (unsigned long long)s.red[t][0]);
}

// one thread a segment, after confusion_kernel: TN = length - TP - FP - FN
__global__ void __launch_bounds__(CF_THREADS) confusion_tn_kernel(long long n, const long long* __restrict__ seg_offsets, int n_segments,
                                                                  unsigned long long* __restrict__ counts) {
    const long long seg = (long long)blockIdx.x * CF_THREADS + threadIdx.x;
    if (seg >= n_segments) return;
    long long a = seg_offsets[seg], b = seg_offsets[seg + 1];
    if (a < 0) a = 0;
    if (b > n) b = n;
    const unsigned long long len = b > a ? (unsigned long long)(b - a) : 0ull;
    counts[seg * 4 + 3] = len - counts[seg * 4] - counts[seg * 4 + 1] - counts[seg * 4 + 2];
}

// workgroups per segment: one per CF_TILES_PER_BLOCK tiles of the longest segment (+ 3: the alignment head), so that a workgroup's tree and its
// three atomics stand behind 128 KB of reads, held to CF_MAX_BLOCKS workgroups over all segments but one per segment at least (more than CF_MAX_BLOCKS
// segments: one workgroup each); the tile loop strides, so a max_seg_len that is too small costs time, not counts
inline unsigned cf_grid_x(long long max_seg_len, int n_segments) {
    const unsigned long long tiles = (((unsigned long long)max_seg_len + 3 + CF_TILE - 1) / CF_TILE + CF_TILES_PER_BLOCK - 1) / CF_TILES_PER_BLOCK;
    const unsigned long long cap = (unsigned long long)(CF_MAX_BLOCKS / n_segments > 0 ? CF_MAX_BLOCKS / n_segments : 1);
    const unsigned long long g = tiles < cap ? tiles : cap;
    return (unsigned)(g > 0 ? g : 1);
}
inline unsigned cf_grid_tn(int n_segments) { return (unsigned)((n_segments + CF_THREADS - 1) / CF_THREADS); }
inline unsigned cf_grid_zero(int n_segments) { return (unsigned)((4 * n_segments + CF_THREADS - 1) / CF_THREADS); }

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

extern "C" {

int uad_confusion_by_segment(const float* pred, float thr, const uint8_t* gt, long long n, const long long* seg_offsets, int n_segments,
                             long long max_seg_len, long long* counts, void* stream) {
    if (n < 0 || n_segments < 0 || max_seg_len < 0)
        return fail(UAD_ERR_INVALID, "confusion_by_segment: negative size (n = %lld, n_segments = %d, max_seg_len = %lld)", n, n_segments, max_seg_len);
    if (n_segments > CF_MAX_SEGMENTS) return fail(UAD_ERR_INVALID, "confusion_by_segment: at most %d segments a call, got %d", CF_MAX_SEGMENTS, n_segments);
    if (n_segments == 0) return UAD_OK;
    if (!counts) return fail(UAD_ERR_INVALID, "confusion_by_segment: bad arguments");
    if (((uintptr_t)counts & 7) != 0) return fail(UAD_ERR_INVALID, "confusion_by_segment: counts must be 8-byte aligned");
    if (n > CF_MAX_N) return fail(UAD_ERR_UNSUPPORTED, "confusion_by_segment: at most 2^31 - 1 values, got %lld", n);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_segments * 4 * sizeof(long long), st));
        return UAD_OK;
    }
    if (!pred || !gt || !seg_offsets) return fail(UAD_ERR_INVALID, "confusion_by_segment: bad arguments");
    if (((uintptr_t)pred & 3) != 0) return fail(UAD_ERR_INVALID, "confusion_by_segment: pred must be 4-byte aligned");
    if (((uintptr_t)seg_offsets & 7) != 0) return fail(UAD_ERR_INVALID, "confusion_by_segment: seg_offsets must be 8-byte aligned");
    hipLaunchKernelGGL(confusion_zero_kernel, dim3(cf_grid_zero(n_segments)), dim3(CF_THREADS), 0, st, n_segments, (unsigned long long*)counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(confusion_kernel, dim3(cf_grid_x(max_seg_len, n_segments), (unsigned)n_segments), dim3(CF_THREADS), 0, st, pred, thr, gt, n,
                       seg_offsets, (unsigned long long*)counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(confusion_tn_kernel, dim3(cf_grid_tn(n_segments)), dim3(CF_THREADS), 0, st, n, seg_offsets, n_segments, (unsigned long long*)counts);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
