// Per-class histograms and moments in one pass (reference utils/Evaluation.py:399-411 -> utils/utils.py:44-71, plot_histogram_with_labels:
// the histogram of the residual / epistemic-variance volume split by ground-truth class on class 0's edge array, np.mean / np.var per class).
//   1. hist_class_kernel   a workgroup walks tiles of HC_TILE values (16-byte loads of the values, dword loads of the u8 class ids).  Counts:
//                          binary search of the shared edge table in LDS, one LDS counter array [n_classes][bins] per workgroup (integer
//                          LDS atomics), added to the global int64 counters once at the end (integer atomics).  Moments: every thread adds
//                          its HC_RUN = 32 values of the tile per class in fp64 -- v, or (v - centre[c])^2 --, the workgroup reduces the 256
//                          runs as a tree in LDS in a fixed order and writes ONE partial per TILE; nothing is carried from tile to tile.
//   2. hist_class_finish_kernel  one workgroup: thread t adds the partials t, t + 256, ... in that order, the same tree adds the 256 runs.
// No floating-point atomic anywhere: the sums are bit-identical from run to run and do not depend on the grid or on what else runs.
// The longest chain of dependent fp64 additions is HC_RUN + 8 + ceil(tiles / 256) + 8 <= UAD_HISTOGRAM_SUM_CHAIN for every n the entry accepts.
// Bytes: one launch reads 4 B (value) + 1 B (class id) per voxel and writes 64 B per tile of 8192 (0.008 B per voxel).
// tests/native/hist_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co., the
// launch layer at the end of the file is left out).
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int HC_THREADS = 256, HC_ROUNDS = 8, HC_RUN = 4 * HC_ROUNDS;     // 32 values per thread and tile
constexpr int HC_TILE = HC_THREADS * HC_RUN;                                // 8192 values per tile
constexpr int HC_CLASSES = UAD_HISTOGRAM_MAX_CLASSES;
constexpr int HC_MAX_BLOCKS = 2048;
constexpr long long HC_MAX_N = 0x7fffffffLL;
static_assert(HC_TILE == UAD_SELECT_TILE, "include/uad_hip.h states the tile");
static_assert(HC_RUN + 8 + (int)((HC_MAX_N + 3 + HC_TILE - 1) / HC_TILE + HC_THREADS - 1) / HC_THREADS + 8 <= UAD_HISTOGRAM_SUM_CHAIN,
              "include/uad_hip.h states the longest chain of dependent additions");

// one tile's contribution: written by hist_class_kernel, added by hist_class_finish_kernel
struct HcPartial {
    double sum[HC_CLASSES];
    unsigned long long count[HC_CLASSES];
};
static_assert(sizeof(HcPartial) == 64, "uad_histogram_by_class_workspace counts 64 bytes per tile");

struct HcLds {
    float edges[UAD_HISTOGRAM_MAX_BINS + 4];
    unsigned hist[HC_CLASSES * UAD_HISTOGRAM_MAX_BINS];
    double red_sum[HC_CLASSES][HC_THREADS];
    unsigned long long red_count[HC_CLASSES][HC_THREADS];
};

// bin of v in the edge table e[0 .. bins]: the last i < bins with e[i] <= v, provided v <= e[bins]; -1 otherwise (NaN included) -- the rule
// of uad_histogram_edges (uad_select.hip: edge_bin)
__device__ __forceinline__ int hc_edge_bin(const float* e, int bins, float v) {
    if (!(v >= e[0]) || !(v <= e[bins])) return -1;
    int lo = 0, hi = bins;                 // invariant: e[lo] <= v, and (hi == bins or e[hi] > v)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// the 256 runs of every class added as a tree: level d adds run t + d to run t for t < d, d = 128, 64, ... 1 -- 8 dependent additions
__device__ __forceinline__ void hc_tree(HcLds& s, int n_classes, int t) {
    for (int d = HC_THREADS / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (t < d)
            for (int c = 0; c < n_classes; ++c) {
                s.red_sum[c][t] = s.red_sum[c][t] + s.red_sum[c][t + d];
                s.red_count[c][t] += s.red_count[c][t + d];
            }
    }
    __syncthreads();
}

__shared__ HcLds hc_lds;

// in, labels: n values / class ids; the tiles are taken relative to the 16-byte boundary at or below `in` (off = the elements between), so
// a chunk of four that lies wholly inside the array is one 16-byte load.  lab_vec: labels - off is 4-byte aligned, the chunk's ids are one dword.
// edges / counts: NULL or bins == 0 = no histogram.  partials: NULL = no moments; else [tiles].  centre: NULL = sum of v.
__global__ void __launch_bounds__(HC_THREADS) hist_class_kernel(const float* __restrict__ in, const uint8_t* __restrict__ labels, unsigned long long n,
                                                                int n_classes, const float* __restrict__ edges, int bins,
                                                                const double* __restrict__ centre, unsigned long long* __restrict__ counts,
                                                                HcPartial* __restrict__ partials, unsigned long long tiles, int lab_vec) {
    HcLds& s = hc_lds;
    const int t = threadIdx.x;
    if (bins > 0) {
        for (int i = t; i <= bins; i += HC_THREADS) s.edges[i] = edges[i];
        for (int i = t; i < n_classes * bins; i += HC_THREADS) s.hist[i] = 0u;
    }
    double cen[HC_CLASSES];
#pragma unroll
    for (int c = 0; c < HC_CLASSES; ++c) cen[c] = (centre && c < n_classes) ? centre[c] : 0.0;
    __syncthreads();
    const unsigned long long off = ((uintptr_t)in >> 2) & 3u;
    const float* aligned = in - off;
    const uint8_t* lab_aligned = labels - off;
    const unsigned long long end = off + n;
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        double sum[HC_CLASSES] = {0.0, 0.0, 0.0, 0.0};
        unsigned long long cnt[HC_CLASSES] = {0ull, 0ull, 0ull, 0ull};
        for (int r = 0; r < HC_ROUNDS; ++r) {
            const unsigned long long j0 = (tile * (HC_TILE / 4) + (unsigned long long)r * HC_THREADS + t) * 4ull;
            if (j0 >= end || j0 + 4 <= off) continue;
            float v[4];
            unsigned id[4];
            bool ok[4];
            if (j0 >= off && j0 + 4 <= end) {
                const float4 x = *reinterpret_cast<const float4*>(aligned + j0);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                if (lab_vec) {
                    const unsigned w = *reinterpret_cast<const unsigned*>(lab_aligned + j0);
                    id[0] = w & 255u; id[1] = (w >> 8) & 255u; id[2] = (w >> 16) & 255u; id[3] = w >> 24;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) id[e] = lab_aligned[j0 + e];
                }
                ok[0] = ok[1] = ok[2] = ok[3] = true;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ok[e] = j0 + e >= off && j0 + e < end;
                    v[e] = ok[e] ? aligned[j0 + e] : 0.f;
                    id[e] = ok[e] ? lab_aligned[j0 + e] : 255u;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!ok[e] || id[e] >= (unsigned)n_classes) continue;
                if (bins > 0) {
                    const int b = hc_edge_bin(s.edges, bins, v[e]);
                    if (b >= 0) atomicAdd(&s.hist[id[e] * bins + b], 1u);
                }
                if (partials) {
#pragma unroll
                    for (int c = 0; c < HC_CLASSES; ++c) {
                        if (id[e] != (unsigned)c) continue;
                        const double d = (double)v[e] - cen[c];
                        sum[c] = sum[c] + (centre ? d * d : d);
                        cnt[c] += 1ull;
                    }
                }
            }
        }
        if (partials) {                      // uniform over the workgroup
            for (int c = 0; c < n_classes; ++c) { s.red_sum[c][t] = sum[c]; s.red_count[c][t] = cnt[c]; }
            hc_tree(s, n_classes, t);
            if (t == 0) {                    // thread 0 owns run 0 of every class: it alone writes them again in the next tile
                for (int c = 0; c < HC_CLASSES; ++c) {
                    partials[tile].sum[c] = c < n_classes ? s.red_sum[c][0] : 0.0;
                    partials[tile].count[c] = c < n_classes ? s.red_count[c][0] : 0ull;
                }
            }
        }
    }
    if (bins > 0) {
        __syncthreads();
        for (int i = t; i < n_classes * bins; i += HC_THREADS) {
            const unsigned c = s.hist[i];
            if (c) atomicAdd(&counts[i], (unsigned long long)c);
        }
    }
}

// one workgroup.  class_count [n_classes] int64, sums [n_classes] fp64
__global__ void __launch_bounds__(HC_THREADS) hist_class_finish_kernel(const HcPartial* __restrict__ partials, unsigned long long tiles, int n_classes,
                                                                       long long* __restrict__ class_count, double* __restrict__ sums) {
    HcLds& s = hc_lds;
    const int t = threadIdx.x;
    double sum[HC_CLASSES] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long cnt[HC_CLASSES] = {0ull, 0ull, 0ull, 0ull};
    for (unsigned long long p = t; p < tiles; p += HC_THREADS)
        for (int c = 0; c < n_classes; ++c) {
            sum[c] = sum[c] + partials[p].sum[c];
            cnt[c] += partials[p].count[c];
        }
    for (int c = 0; c < n_classes; ++c) { s.red_sum[c][t] = sum[c]; s.red_count[c][t] = cnt[c]; }
    hc_tree(s, n_classes, t);
    if (t < n_classes) {
        sums[t] = s.red_sum[t][0];
        class_count[t] = (long long)s.red_count[t][0];
    }
}

inline unsigned long long hc_tiles(unsigned long long n) { return (n + 3 + HC_TILE - 1) / HC_TILE; }   // + 3: the alignment head
inline unsigned hc_grid(unsigned long long tiles) { return (unsigned)(tiles < (unsigned long long)HC_MAX_BLOCKS ? tiles : HC_MAX_BLOCKS); }
inline int hc_lab_vec(const float* in, const uint8_t* labels) {
    const uintptr_t off = ((uintptr_t)in >> 2) & 3u;
    return (((uintptr_t)labels - off) & 3u) == 0 ? 1 : 0;
}

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

extern "C" {

size_t uad_histogram_by_class_workspace(long long n) {
    if (n <= 0 || n > HC_MAX_N) return 0;
    return (size_t)hc_tiles((unsigned long long)n) * sizeof(HcPartial);
}

int uad_histogram_by_class(const float* in, const uint8_t* labels, long long n, int n_classes, const float* edges, int bins, const double* centre,
                           long long* counts, long long* class_count, double* sums, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || bins < 0) return fail(UAD_ERR_INVALID, "histogram_by_class: negative size (n = %lld, bins = %d)", n, bins);
    if (n_classes < 1 || n_classes > HC_CLASSES) return fail(UAD_ERR_INVALID, "histogram_by_class: 1 .. %d classes, got %d", HC_CLASSES, n_classes);
    if (bins > UAD_HISTOGRAM_MAX_BINS) return fail(UAD_ERR_INVALID, "histogram_by_class: at most %d bins a call, got %d", UAD_HISTOGRAM_MAX_BINS, bins);
    if ((!in || !labels) && n > 0) return fail(UAD_ERR_INVALID, "histogram_by_class: bad arguments");
    if (bins > 0 && (!edges || !counts)) return fail(UAD_ERR_INVALID, "histogram_by_class: bins without an edge table or counters");
    if ((class_count == nullptr) != (sums == nullptr)) return fail(UAD_ERR_INVALID, "histogram_by_class: class_count and sums go together");
    if (bins == 0 && !sums) return fail(UAD_ERR_INVALID, "histogram_by_class: nothing to compute");
    if (n > HC_MAX_N) return fail(UAD_ERR_UNSUPPORTED, "histogram_by_class: at most 2^31 - 1 values, got %lld", n);
    if (((uintptr_t)in & 3) != 0) return fail(UAD_ERR_INVALID, "histogram_by_class: input must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (bins > 0) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_classes * bins * sizeof(long long), st));
    if (n == 0) {
        if (sums) {
            HIP_TRY(hipMemsetAsync(class_count, 0, (size_t)n_classes * sizeof(long long), st));
            HIP_TRY(hipMemsetAsync(sums, 0, (size_t)n_classes * sizeof(double), st));
        }
        return UAD_OK;
    }
    const unsigned long long tiles = hc_tiles((unsigned long long)n);
    if (sums) {
        const size_t need = uad_histogram_by_class_workspace(n);
        if (!workspace || workspace_bytes < need) return fail(UAD_ERR_INVALID, "histogram_by_class: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        if (((uintptr_t)workspace & 15) != 0) return fail(UAD_ERR_INVALID, "histogram_by_class: workspace must be 16-byte aligned");
    }
    HcPartial* partials = sums ? (HcPartial*)workspace : nullptr;      // every tile's partial is written by the first kernel: no initialisation
    hipLaunchKernelGGL(hist_class_kernel, dim3(hc_grid(tiles)), dim3(HC_THREADS), 0, st, in, labels, (unsigned long long)n, n_classes, edges, bins, centre,
                       (unsigned long long*)counts, partials, tiles, hc_lab_vec(in, labels));
    HIP_TRY(hipGetLastError());
    if (sums) {
        hipLaunchKernelGGL(hist_class_finish_kernel, dim3(1), dim3(HC_THREADS), 0, st, partials, tiles, n_classes, class_count, sums);
        HIP_TRY(hipGetLastError());
    }
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
