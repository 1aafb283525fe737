// Sums of a resident fp32 array in a defined order, and the standardization map on top of them (reference utils/NII.py:53-75,
// normalize(method='standardization'): clamp to the percentiles, subtract the mean, divide by the standard deviation of the centred data).
//   1. shifted_sums_kernel         for u = f32(f32(clamp(v) - shift) - centre): the fp64 sums of u and of f32(u * u), both in ONE pass.  A
//                                  workgroup takes tiles of MS_TILE values.  Thread t of tile T adds, in this order, the values
//                                  T * MS_TILE + (r * 256 + t) * 4 + e for r = 0 .. 7, e = 0 .. 3 that lie below n -- its MS_RUN = 32 values,
//                                  eight 16-byte chunks -- to +0.0 in fp64; the workgroup adds its 256 runs as a tree in LDS (level d = 128,
//                                  64, ... 1: run t + d onto run t) and writes ONE partial per tile; nothing is carried from tile to tile.
//   2. shifted_sums_finish_kernel  one workgroup: thread t adds the partials t, t + 256, ... in that order to +0.0, the same tree adds the 256 runs.
//   3. clamp_standardize_kernel    out = f32(f32(clamp(v) - mean) / std), a true division.
// The order of summation is that of uad_histogram_by_class's sums (uad_hist.hip) with ONE difference: the tiles are counted from `in`, not
// from the 16-byte boundary below it.  The order is therefore a function of n alone; where `in` is only 4-byte aligned a chunk is cut out
// of the two aligned 16-byte words it straddles, and a value goes to the same thread, round and place as with an aligned base.
// No floating-point atomic anywhere: the sums are bit-identical from run to run and do not depend on the grid or on what else runs.
// The longest chain of dependent fp64 additions is MS_RUN + 8 + ceil(tiles / 256) + 8 <= UAD_SHIFTED_SUMS_CHAIN for every n the entry accepts.
// Bytes: a sums launch reads 4 B per value and writes 16 B per tile of 8192; the map reads 4 B and writes 4 B per value.
// All per-element arithmetic is fp32 and unfused (-ffp-contract=off, build.py): utils/standardize.py states it in numpy with the same bits.
// tests/native/moments_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co., the
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

constexpr int MS_THREADS = 256, MS_ROUNDS = 8, MS_RUN = 4 * MS_ROUNDS;     // 32 values per thread and tile
constexpr int MS_TILE = MS_THREADS * MS_RUN;                                // 8192 values per tile
constexpr int MS_MAX_BLOCKS = 2048;
constexpr long long MS_MAX_N = 0x7fffffffLL;
static_assert(MS_TILE == UAD_SELECT_TILE, "include/uad_hip.h states the tile");
static_assert(MS_RUN + 8 + (int)((MS_MAX_N + MS_TILE - 1) / MS_TILE + MS_THREADS - 1) / MS_THREADS + 8 <= UAD_SHIFTED_SUMS_CHAIN,
              "include/uad_hip.h states the longest chain of dependent additions");

// one tile's contribution: written by shifted_sums_kernel, added by shifted_sums_finish_kernel
struct MsPartial {
    double s1, s2;
};
static_assert(sizeof(MsPartial) == 16, "uad_shifted_sums_workspace counts 16 bytes per tile");

struct MsLds {
    double red[2][MS_THREADS];
};

__shared__ MsLds ms_lds;

__device__ __forceinline__ float ms_clamp(float v, float lo, float hi) {
    v = v < lo ? lo : v;            // numpy: v[v < lo] = lo (uad_select.hip: clamp_scale1)
    v = v > hi ? hi : v;
    return v;
}

// the 256 runs of both sums added as a tree: level d adds run t + d to run t for t < d, d = 128, 64, ... 1 -- 8 dependent additions
__device__ __forceinline__ void ms_tree(MsLds& s, int t) {
    for (int d = MS_THREADS / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (t < d) {
            s.red[0][t] = s.red[0][t] + s.red[0][t + d];
            s.red[1][t] = s.red[1][t] + s.red[1][t + d];
        }
    }
    __syncthreads();
}

// the chunk in[j0 .. j0 + 3] (j0 a multiple of 4) that lies wholly inside the array and, where off != 0, has both aligned words it straddles
// inside it too: `aligned` = in - off is 16-byte aligned, the chunk is aligned[j0 + off .. j0 + off + 3]
__device__ __forceinline__ float4 ms_chunk(const float* __restrict__ aligned, unsigned off, unsigned long long j0) {
    const float4 a = *reinterpret_cast<const float4*>(aligned + j0);
    if (off == 0) return a;
    const float4 b = *reinterpret_cast<const float4*>(aligned + j0 + 4);
    if (off == 1) return make_float4(a.y, a.z, a.w, b.x);
    if (off == 2) return make_float4(a.z, a.w, b.x, b.y);
    return make_float4(a.w, b.x, b.y, b.z);
}

// in: n values, 4-byte aligned.  partials [tiles], tiles = ceil(n / MS_TILE): tile T is in[T * MS_TILE ..) whatever the alignment of `in`.
__global__ void __launch_bounds__(MS_THREADS) shifted_sums_kernel(const float* __restrict__ in, unsigned long long n, float lo, float hi, float shift,
                                                                  float centre, MsPartial* __restrict__ partials, unsigned long long tiles) {
    MsLds& s = ms_lds;
    const int t = threadIdx.x;
    const unsigned off = (unsigned)(((uintptr_t)in >> 2) & 3u);
    const float* aligned = in - off;
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const unsigned long long base = tile * MS_TILE;
        double s1 = 0.0, s2 = 0.0;
        // a tile whose chunks can all be loaded as 16-byte words: not the first one of an unaligned array (its first word starts below `in`),
        // and the word behind its last chunk lies inside the array
        const bool whole = off == 0 ? base + MS_TILE <= n : (tile > 0 && base + MS_TILE + 4 <= n + off);
        if (whole) {                         // uniform over the workgroup
            float4 x[MS_ROUNDS];
#pragma unroll
            for (int r = 0; r < MS_ROUNDS; ++r) x[r] = ms_chunk(aligned, off, base + ((unsigned long long)r * MS_THREADS + t) * 4ull);
#pragma unroll
            for (int r = 0; r < MS_ROUNDS; ++r) {
                const float v[4] = {x[r].x, x[r].y, x[r].z, x[r].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float c = ms_clamp(v[e], lo, hi) - shift;
                    const float u = c - centre;
                    const float q = u * u;
                    s1 = s1 + (double)u;
                    s2 = s2 + (double)q;
                }
            }
        } else {
            for (int r = 0; r < MS_ROUNDS; ++r) {
                const unsigned long long j0 = base + ((unsigned long long)r * MS_THREADS + t) * 4ull;
                if (j0 >= n) break;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                int m = 4;
                if (j0 + 4 <= n && (off == 0 || (j0 >= 4 && j0 + 8 <= n + off))) {
                    const float4 x = ms_chunk(aligned, off, j0);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                } else {
                    m = (int)(n - j0 < 4ull ? n - j0 : 4ull);
                    for (int e = 0; e < m; ++e) v[e] = in[j0 + e];
                }
                for (int e = 0; e < m; ++e) {
                    const float c = ms_clamp(v[e], lo, hi) - shift;
                    const float u = c - centre;
                    const float q = u * u;
                    s1 = s1 + (double)u;
                    s2 = s2 + (double)q;
                }
            }
        }
        s.red[0][t] = s1;
        s.red[1][t] = s2;
        ms_tree(s, t);
        if (t == 0) {                        // thread 0 owns run 0: it alone writes it again in the next tile
            partials[tile].s1 = s.red[0][0];
            partials[tile].s2 = s.red[1][0];
        }
    }
}

// one workgroup.  sums [2] fp64
__global__ void __launch_bounds__(MS_THREADS) shifted_sums_finish_kernel(const MsPartial* __restrict__ partials, unsigned long long tiles,
                                                                         double* __restrict__ sums) {
    MsLds& s = ms_lds;
    const int t = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (unsigned long long p = t; p < tiles; p += MS_THREADS) {
        s1 = s1 + partials[p].s1;
        s2 = s2 + partials[p].s2;
    }
    s.red[0][t] = s1;
    s.red[1][t] = s2;
    ms_tree(s, t);
    if (t < 2) sums[t] = s.red[t][0];
}

__device__ __forceinline__ float ms_standardize1(float v, float lo, float hi, float mean, float sd) {
    const float c = ms_clamp(v, lo, hi) - mean;
    return c / sd;
}

// vec: in and out are 16-byte aligned -- n / 4 chunks of four and a scalar tail
__global__ void __launch_bounds__(256) clamp_standardize_kernel(const float* in, unsigned long long n, float lo, float hi, float mean, float sd, float* out,
                                                                int vec) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256, g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const unsigned long long chunks = n / 4;
        for (unsigned long long c = g; c < chunks; c += stride) {
            float4 x = reinterpret_cast<const float4*>(in)[c];
            x.x = ms_standardize1(x.x, lo, hi, mean, sd); x.y = ms_standardize1(x.y, lo, hi, mean, sd);
            x.z = ms_standardize1(x.z, lo, hi, mean, sd); x.w = ms_standardize1(x.w, lo, hi, mean, sd);
            reinterpret_cast<float4*>(out)[c] = x;
        }
        const unsigned long long i = chunks * 4 + g;
        if (i < n) out[i] = ms_standardize1(in[i], lo, hi, mean, sd);
    } else {
        for (unsigned long long i = g; i < n; i += stride) out[i] = ms_standardize1(in[i], lo, hi, mean, sd);
    }
}

inline unsigned long long ms_tiles(unsigned long long n) { return (n + MS_TILE - 1) / MS_TILE; }
inline unsigned ms_grid(unsigned long long tiles) { return (unsigned)(tiles < (unsigned long long)MS_MAX_BLOCKS ? tiles : MS_MAX_BLOCKS); }
inline int ms_map_vec(const float* in, const float* out) { return (((uintptr_t)in | (uintptr_t)out) & 15) == 0 ? 1 : 0; }
inline unsigned ms_map_grid(unsigned long long n, int vec) {
    const unsigned long long items = vec ? n / 4 + 3 : n;
    const unsigned long long blocks = (items + 255) / 256;
    return (unsigned)(blocks < (unsigned long long)MS_MAX_BLOCKS ? blocks : MS_MAX_BLOCKS);
}

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

extern "C" {

size_t uad_shifted_sums_workspace(long long n) {
    if (n <= 0 || n > MS_MAX_N) return 0;
    return (size_t)ms_tiles((unsigned long long)n) * sizeof(MsPartial);
}

int uad_shifted_sums(const float* in, long long n, float clamp_lo, float clamp_hi, float shift, float centre, double* sums_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (n < 0) return fail(UAD_ERR_INVALID, "shifted_sums: negative size (n = %lld)", n);
    if (!sums_out || (!in && n > 0)) return fail(UAD_ERR_INVALID, "shifted_sums: bad arguments");
    if (n > MS_MAX_N) return fail(UAD_ERR_UNSUPPORTED, "shifted_sums: at most 2^31 - 1 values, got %lld", n);
    if (((uintptr_t)in & 3) != 0) return fail(UAD_ERR_INVALID, "shifted_sums: input must be 4-byte aligned");
    if (((uintptr_t)sums_out & 7) != 0) return fail(UAD_ERR_INVALID, "shifted_sums: sums_out must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(sums_out, 0, 2 * sizeof(double), st));
        return UAD_OK;
    }
    const size_t need = uad_shifted_sums_workspace(n);
    if (!workspace || workspace_bytes < need) return fail(UAD_ERR_INVALID, "shifted_sums: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (((uintptr_t)workspace & 15) != 0) return fail(UAD_ERR_INVALID, "shifted_sums: workspace must be 16-byte aligned");
    const unsigned long long tiles = ms_tiles((unsigned long long)n);
    MsPartial* partials = (MsPartial*)workspace;                       // every tile's partial is written by the first kernel: no initialisation
    hipLaunchKernelGGL(shifted_sums_kernel, dim3(ms_grid(tiles)), dim3(MS_THREADS), 0, st, in, (unsigned long long)n, clamp_lo, clamp_hi, shift, centre,
                       partials, tiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(shifted_sums_finish_kernel, dim3(1), dim3(MS_THREADS), 0, st, partials, tiles, sums_out);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_clamp_standardize(const float* in, long long n, float clamp_lo, float clamp_hi, float mean, float std, float* out, void* stream) {
    if (n < 0 || ((!in || !out) && n > 0)) return fail(UAD_ERR_INVALID, "clamp_standardize: bad arguments");
    if ((((uintptr_t)in | (uintptr_t)out) & 3) != 0) return fail(UAD_ERR_INVALID, "clamp_standardize: input and output must be 4-byte aligned");
    if (n == 0) return UAD_OK;
    const int vec = ms_map_vec(in, out);
    hipLaunchKernelGGL(clamp_standardize_kernel, dim3(ms_map_grid((unsigned long long)n, vec)), dim3(256), 0, (hipStream_t)stream, in, (unsigned long long)n,
                       clamp_lo, clamp_hi, mean, std, out, vec);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
