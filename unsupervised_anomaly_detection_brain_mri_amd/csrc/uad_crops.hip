// Per-component measurements of a label volume and the window gather of the crop modes, on the device: the `regionprops` half of the
// reference's cropType 'lesions' (dataloaders/MSLUB.py:200-222, the same lines in MSISBI2015.py / MSSEG2008.py: skimage label + regionprops,
// one crop per component centred on its centroid) and the crop() of cropType 'lesions' / 'random' (dataloaders/BRAINWEB.py:166-173,
// utils/image_utils.py:15-16) for all windows of a resident slice batch at once.  utils/crops.py is the host statement of both; skimage is
// not a dependency and that statement has not been compared with skimage's own output.
//
// uad_cc_props works on the output of uad_cc_label (csrc/uad_cc.hip): label = 1 + the smallest linear index of the component, so the ROOTS
// are the voxels with labels[v] == v + 1 and their index order is the row order of the host statement.  Four kernels, ordered by kernel
// boundary on the caller's stream; a workgroup of PR_THREADS threads owns PR_TILE consecutive voxels:
//   props_count_kernel       roots per tile -> tile_count[tile]
//   props_scan_kernel        ONE workgroup: exclusive scan of the tile counts in place, total -> *n_components
//   props_rank_kernel        root flags of the tile into LDS in index order, workgroup scan, rank = tile offset + local rank -> rank[v] at the
//                            root's own voxel; the root writes its row (first = v, the four sums 0) when rank < max_components
//   props_accumulate_kernel  every foreground voxel adds (1, z, y, x) to the row rank[labels[v] - 1]: first into a PR_SLOTS-entry LDS table keyed
//                            by label (64-bit LDS atomics; a tile of 1024 consecutive voxels meets few components), on a slot collision
//                            straight into the row with 64-bit global atomics; the table is flushed with one global atomic per entry and
//                            column.  Integer adds commute: the result does not depend on the order of execution.
// No floating point, no host synchronisation, nothing is written past row max_components - 1.
//
// crop_kernel, one launch: a thread owns four consecutive pixels of one window row (grid = quads of a window x k); lanes walk a row in
// ascending address order; 16-byte stores where the crop width is a multiple of four and `out` is 16-byte aligned, the loads are single words
// because `left` is arbitrary.  Words are moved as uint32: every bit pattern survives.
// tests/native/crops_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co. and the
// atomics, the launch layer at the end of the file is left out).
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

namespace {

constexpr int PR_THREADS = 256;                     // four waves
constexpr int PR_ITEMS = 4;                         // voxels a thread owns, PR_THREADS apart: a wave reads 256 consecutive bytes per item
constexpr int PR_TILE = PR_THREADS * PR_ITEMS;      // 1024 consecutive voxels a workgroup
constexpr int PR_SLOTS = 64;                        // entries of the per-tile aggregation table
constexpr int PR_COLS = 5;                          // first, area, sum_z, sum_y, sum_x

// LDS of the three kernels that use any (7.3 KiB: occupancy is bounded by the 256 threads, not by LDS).  At namespace scope so that the
// host emulation can poison it between workgroups: an entry its own workgroup did not write must never be used.
struct PropsLds {
    int flag[PR_TILE];
    int part[PR_THREADS];
    int count;
    int key[PR_SLOTS];
    unsigned long long acc[PR_SLOTS][4];
};
__shared__ PropsLds pr_lds;

__device__ __forceinline__ bool pr_is_root(const int* __restrict__ labels, long long v, long long total) { return v < total && labels[v] == (int)v + 1; }

// inclusive Hillis-Steele scan of pr_lds.part over the workgroup; every thread calls it, returns the thread's inclusive value
__device__ __forceinline__ int pr_block_scan(int tid) {
    int (&part)[PR_THREADS] = pr_lds.part;
    for (int off = 1; off < PR_THREADS; off <<= 1) {
        const int t = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    return part[tid];
}

__global__ __launch_bounds__(PR_THREADS) void props_count_kernel(const int* __restrict__ labels, long long total, int* __restrict__ tile_count) {
    const int tid = threadIdx.x;
    if (tid == 0) pr_lds.count = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * PR_TILE;
    int c = 0;
#pragma unroll
    for (int i = 0; i < PR_ITEMS; ++i) c += pr_is_root(labels, base + i * PR_THREADS + tid, total) ? 1 : 0;
    if (c) atomicAdd(&pr_lds.count, c);
    __syncthreads();
    if (tid == 0) tile_count[blockIdx.x] = pr_lds.count;
}

__global__ __launch_bounds__(PR_THREADS) void props_scan_kernel(int* tile_count, int tiles, int* __restrict__ n_components) {
    const int tid = threadIdx.x;
    int carry = 0;                                                // the same in every thread
    for (int base = 0; base < tiles; base += PR_THREADS) {
        const int i = base + tid;
        const int c = i < tiles ? tile_count[i] : 0;
        pr_lds.part[tid] = c;
        __syncthreads();
        const int incl = pr_block_scan(tid);
        if (i < tiles) tile_count[i] = carry + incl - c;
        carry += pr_lds.part[PR_THREADS - 1];
        __syncthreads();                                          // part is overwritten by the next round
    }
    if (tid == 0) *n_components = carry;
}

__global__ __launch_bounds__(PR_THREADS) void props_rank_kernel(const int* __restrict__ labels, long long total, const int* __restrict__ tile_offset,
                                                                int* __restrict__ rank, long long* __restrict__ props, int max_components) {
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * PR_TILE;
#pragma unroll
    for (int i = 0; i < PR_ITEMS; ++i) pr_lds.flag[i * PR_THREADS + tid] = pr_is_root(labels, base + i * PR_THREADS + tid, total) ? 1 : 0;
    __syncthreads();
    int f[PR_ITEMS], mine = 0;                                    // the thread now owns entries 4 tid .. 4 tid + 3 of the tile: index order
#pragma unroll
    for (int k = 0; k < PR_ITEMS; ++k) { f[k] = pr_lds.flag[PR_ITEMS * tid + k]; mine += f[k]; }
    pr_lds.part[tid] = mine;
    __syncthreads();
    int r = tile_offset[blockIdx.x] + pr_block_scan(tid) - mine;
#pragma unroll
    for (int k = 0; k < PR_ITEMS; ++k) {
        if (!f[k]) continue;
        const long long v = base + PR_ITEMS * tid + k;
        rank[v] = r;
        if (r < max_components) {
            long long* __restrict__ row = props + (size_t)r * PR_COLS;
            row[0] = v; row[1] = 0; row[2] = 0; row[3] = 0; row[4] = 0;
        }
        ++r;
    }
}

__device__ __forceinline__ void pr_add_row(long long* props, int k, int max_components, unsigned long long area, unsigned long long sz, unsigned long long sy,
                                           unsigned long long sx) {
    if ((unsigned)k >= (unsigned)max_components) return;          // past the cap (or the rank of a voxel that is no root: malformed labels)
    unsigned long long* row = reinterpret_cast<unsigned long long*>(props) + (size_t)k * PR_COLS;
    atomicAdd(&row[1], area); atomicAdd(&row[2], sz); atomicAdd(&row[3], sy); atomicAdd(&row[4], sx);
}

__global__ __launch_bounds__(PR_THREADS) void props_accumulate_kernel(const int* __restrict__ labels, long long total, int H, int W, const int* __restrict__ rank,
                                                                      long long* props, int max_components) {
    const int tid = threadIdx.x;
    if (tid < PR_SLOTS) {
        pr_lds.key[tid] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) pr_lds.acc[tid][c] = 0ull;
    }
    __syncthreads();
    const long long base = (long long)blockIdx.x * PR_TILE, HW = (long long)H * W;
#pragma unroll
    for (int i = 0; i < PR_ITEMS; ++i) {
        const long long v = base + i * PR_THREADS + tid;
        if (v >= total) continue;
        const int lab = labels[v];
        if (lab <= 0 || (long long)lab > total) continue;         // background (a label outside the volume is the caller's error: ignored)
        const unsigned long long z = (unsigned long long)(v / HW), rem = (unsigned long long)(v - (long long)z * HW), y = rem / (unsigned)W, x = rem - y * (unsigned)W;
        const int slot = (int)(((unsigned)lab * 2654435761u) >> 26);
        const int old = atomicCAS(&pr_lds.key[slot], 0, lab);
        if (old == 0 || old == lab) {
            atomicAdd(&pr_lds.acc[slot][0], 1ull); atomicAdd(&pr_lds.acc[slot][1], z); atomicAdd(&pr_lds.acc[slot][2], y); atomicAdd(&pr_lds.acc[slot][3], x);
        } else {
            pr_add_row(props, rank[lab - 1], max_components, 1ull, z, y, x);
        }
    }
    __syncthreads();
    if (tid < PR_SLOTS && pr_lds.key[tid] != 0)
        pr_add_row(props, rank[pr_lds.key[tid] - 1], max_components, pr_lds.acc[tid][0], pr_lds.acc[tid][1], pr_lds.acc[tid][2], pr_lds.acc[tid][3]);
}
static_assert(PR_SLOTS == 64, "the slot hash keeps the top six bits");

constexpr int CR_THREADS = 256;
constexpr int CR_PX = 4;                            // pixels a thread owns (one 16-byte store)

__global__ __launch_bounds__(CR_THREADS) void crop_kernel(const uint32_t* __restrict__ in, int h, int w, const int* __restrict__ origins, int ch, int cw, int quads_per_row,
                                                          int vec4, uint32_t* __restrict__ out) {
    const long long q = (long long)blockIdx.x * CR_THREADS + threadIdx.x;
    if (q >= (long long)ch * quads_per_row) return;
    const int row = (int)(q / quads_per_row), col = (int)(q - (long long)row * quads_per_row) * CR_PX;
    const int j = blockIdx.y;
    const int s = origins[3 * j], top = origins[3 * j + 1], left = origins[3 * j + 2];
    const uint32_t* __restrict__ src = in + ((size_t)s * (size_t)h + (size_t)(top + row)) * (size_t)w + (size_t)(left + col);
    uint32_t* __restrict__ dst = out + ((size_t)j * (size_t)ch + (size_t)row) * (size_t)cw + (size_t)col;
    if (vec4) {                                                   // cw % 4 == 0: four pixels, and the address is 16-byte aligned
        *reinterpret_cast<uint4*>(dst) = make_uint4(src[0], src[1], src[2], src[3]);
    } else {
        const int count = cw - col < CR_PX ? cw - col : CR_PX;
#pragma unroll
        for (int k = 0; k < CR_PX; ++k)
            if (k < count) dst[k] = src[k];
    }
}

// the launch geometry and the workspace layout (shared with the host emulation)
inline long long props_tiles(long long total) { return (total + PR_TILE - 1) / PR_TILE; }
inline size_t props_rank_offset(long long total) { return ((size_t)props_tiles(total) * sizeof(int) + 15) / 16 * 16; }      // tile counts | rank [total]
inline size_t props_workspace_bytes(long long total) { return props_rank_offset(total) + (size_t)total * sizeof(int); }
inline int crop_quads_per_row(int cw) { return (cw + CR_PX - 1) / CR_PX; }
inline long long crop_blocks(int ch, int cw) { return ((long long)ch * crop_quads_per_row(cw) + CR_THREADS - 1) / CR_THREADS; }
inline int crop_vec4(int cw, const void* out) { return cw % CR_PX == 0 && (uintptr_t)out % 16 == 0; }

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

extern "C" {

size_t uad_cc_props_workspace(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return 0;
    const unsigned long long total = (unsigned long long)D * (unsigned long long)H * (unsigned long long)W;
    if (total >= 0x80000000ULL) return 0;
    return props_workspace_bytes((long long)total);
}

int uad_cc_props(const int* labels, int D, int H, int W, long long* props, int max_components, int* n_components, void* workspace, void* stream) {
    if (D <= 0 || H <= 0 || W <= 0 || max_components <= 0)
        return fail(UAD_ERR_INVALID, "cc_props: sizes must be positive, got [%d,%d,%d], max_components %d", D, H, W, max_components);
    if (!labels || !props || !n_components || !workspace) return fail(UAD_ERR_INVALID, "cc_props: labels / props / n_components / workspace is NULL");
    const unsigned long long total_u = (unsigned long long)D * (unsigned long long)H * (unsigned long long)W;
    if (total_u >= 0x80000000ULL) return fail(UAD_ERR_INVALID, "cc_props: D*H*W must be below 2^31, got [%d,%d,%d]", D, H, W);
    const long long total = (long long)total_u;
    hipStream_t st = (hipStream_t)stream;
    int* tile_count = static_cast<int*>(workspace);
    int* rank = reinterpret_cast<int*>(static_cast<char*>(workspace) + props_rank_offset(total));
    const int tiles = (int)props_tiles(total);
    hipLaunchKernelGGL(props_count_kernel, dim3(tiles), dim3(PR_THREADS), 0, st, labels, total, tile_count);
    hipLaunchKernelGGL(props_scan_kernel, dim3(1), dim3(PR_THREADS), 0, st, tile_count, tiles, n_components);
    hipLaunchKernelGGL(props_rank_kernel, dim3(tiles), dim3(PR_THREADS), 0, st, labels, total, (const int*)tile_count, rank, props, max_components);
    hipLaunchKernelGGL(props_accumulate_kernel, dim3(tiles), dim3(PR_THREADS), 0, st, labels, total, H, W, (const int*)rank, props, max_components);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "cc_props launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

int uad_crop2d(const float* in, int n_in, int h, int w, const int* origins, int k, int ch, int cw, float* out, void* stream) {
    if (n_in <= 0 || h <= 0 || w <= 0 || k <= 0 || ch <= 0 || cw <= 0)
        return fail(UAD_ERR_INVALID, "crop2d: sizes must be positive, got [%d,%d,%d] -> [%d,%d,%d]", n_in, h, w, k, ch, cw);
    if (ch > h || cw > w) return fail(UAD_ERR_INVALID, "crop2d: a %d x %d window does not fit a %d x %d slice", ch, cw, h, w);
    if (!in || !origins || !out) return fail(UAD_ERR_INVALID, "crop2d: in / origins / out is NULL");
    if ((const float*)out == in) return fail(UAD_ERR_INVALID, "crop2d: out may not alias in");
    const long long blocks = crop_blocks(ch, cw);
    if (k > 65535 || blocks > 0x7fffffffLL) return fail(UAD_ERR_UNSUPPORTED, "crop2d: [%d,%d,%d] is too large for one grid", k, ch, cw);
    hipLaunchKernelGGL(crop_kernel, dim3((unsigned)blocks, (unsigned)k), dim3(CR_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(in), h, w, origins, ch, cw,
                       crop_quads_per_row(cw), crop_vec4(cw, out), reinterpret_cast<uint32_t*>(out));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "crop2d launch: %s", hipGetErrorString(e));
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
