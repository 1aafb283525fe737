// Bandwidth-bound kernels of the AE/VAE hot path for gfx950: first-layer direct conv, fused final 1x1 conv + L1 loss
// (+ its backward), reparameterisation/KL, reductions, TF-form Adam and the residual anomaly map.
// All are HBM-roofline kernels: 16-byte coalesced NHWC accesses, wavefront (64-lane) shuffle reductions,
// deterministic two-level partial sums (no float atomics).
#include "uad_kernels.h"
#include <stdint.h>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------
// Round 6 (late): the same sum with 16-byte streaming loads -- JL lanes of four adjacent columns x SL slab lanes (512 threads), four slabs in flight per thread.  The
// scalar form below keeps four 4-byte loads in flight per thread: a 373-slab reduction (dec3's filter gradient) is 24 dependent round trips, 29 us for 38 MB,
// and the LAST reduction of a step sits in front of the optimizer.  Fixed order (per lane: four interleaved chains over its slabs, then the slab lanes in index
// order): deterministic, not the scalar form's order.  UAD_NO_REDUCE4 keeps the scalar form.
typedef float v4f_nt __attribute__((ext_vector_type(4)));
// (the body of one workgroup, `vb` = its index among the reduction's workgroups: grad_finish_kernel runs the same sum behind its finalize blocks)
template <int JL, int SL>
__device__ __forceinline__ void reduce4_block(v4f_nt (*red)[JL], int vb, const float* __restrict__ partial, int S, int L, float scale, float* __restrict__ out) {
    const int jl = threadIdx.x % JL, sl = threadIdx.x / JL;
    const int j4 = vb * JL + jl, L4 = L >> 2;
    v4f_nt a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    if (j4 < L4) {
        const v4f_nt* p = reinterpret_cast<const v4f_nt*>(partial) + j4;
        int s = sl;
        for (; s + 3 * SL < S; s += 4 * SL) {
            const v4f_nt v0 = __builtin_nontemporal_load(p + (size_t)s * L4), v1 = __builtin_nontemporal_load(p + (size_t)(s + SL) * L4);
            const v4f_nt v2 = __builtin_nontemporal_load(p + (size_t)(s + 2 * SL) * L4), v3 = __builtin_nontemporal_load(p + (size_t)(s + 3 * SL) * L4);
            a0 += v0; a1 += v1; a2 += v2; a3 += v3;
        }
        for (; s < S; s += SL) a0 += __builtin_nontemporal_load(p + (size_t)s * L4);
    }
    red[sl][jl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sl == 0 && j4 < L4) {
        v4f_nt t = red[0][jl];
#pragma unroll
        for (int k = 1; k < SL; ++k) t += red[k][jl];
        reinterpret_cast<v4f_nt*>(out)[j4] = t * scale;
    }
}
template <int JL, int SL>
__global__ void __launch_bounds__(JL * SL) reduce_partials4_kernel(const float* __restrict__ partial, int S, int L, float scale, float* __restrict__ out) {
    __shared__ v4f_nt red[SL][JL];
    reduce4_block<JL, SL>(red, blockIdx.x, partial, S, L, scale, out);
}

// out[j] = scale * sum_s partial[s][j].  Block = JL (64) j-lanes x SL s-lanes; each thread walks s with stride SL and four
// independent accumulators (loads in flight), then the s-lanes are folded through LDS in a fixed order (deterministic: a column's sum depends on SL alone, not on JL).
template <int JL, int SL>
__device__ __forceinline__ void reduce1_block(float (*red)[JL], int vb, const float* __restrict__ partial, int S, int L,
                                              float scale, float* __restrict__ out, int nt) {
    const int jl = threadIdx.x % JL, sl = threadIdx.x / JL;
    const int j = vb * JL + jl;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (j < L) {
        int s = sl;
        if (nt) {      // streaming loads (uad_launch_reduce_partials)
            for (; s + 3 * SL < S; s += 4 * SL) {
                a0 += __builtin_nontemporal_load(partial + (size_t)s * L + j);
                a1 += __builtin_nontemporal_load(partial + (size_t)(s + SL) * L + j);
                a2 += __builtin_nontemporal_load(partial + (size_t)(s + 2 * SL) * L + j);
                a3 += __builtin_nontemporal_load(partial + (size_t)(s + 3 * SL) * L + j);
            }
        }
        for (; s + 3 * SL < S; s += 4 * SL) {
            a0 += partial[(size_t)s * L + j];
            a1 += partial[(size_t)(s + SL) * L + j];
            a2 += partial[(size_t)(s + 2 * SL) * L + j];
            a3 += partial[(size_t)(s + 3 * SL) * L + j];
        }
        for (; s < S; s += SL) a0 += partial[(size_t)s * L + j];
    }
    red[sl][jl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sl == 0 && j < L) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < SL; ++k) t += red[k][jl];
        out[j] = t * scale;
    }
}
template <int SL>
__global__ void __launch_bounds__(64 * SL) reduce_partials_kernel(const float* __restrict__ partial, int S, int L,
                                                                  float scale, float* __restrict__ out, int nt) {
    __shared__ float red[SL][64];
    reduce1_block<64, SL>(red, blockIdx.x, partial, S, L, scale, out, nt);
}

// colpart[T][2][C] -> dgamma, dbeta, dbias.  One block (1024 threads = 32 channels x 32 tile-lanes) per 32 channels.
__global__ void __launch_bounds__(1024) bn_grad_finalize_kernel(const float* __restrict__ colpart, int T, int C,
                                                                const float* __restrict__ gamma, float rstd,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ dbias) {
    __shared__ float red[2][32][33];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s1 = 0.f, s2 = 0.f;
    if (c < C) {
        for (int t = g; t < T; t += 32) {
            s1 += colpart[((size_t)t * 2 + 0) * C + c];
            s2 += colpart[((size_t)t * 2 + 1) * C + c];
        }
    }
    red[0][g][cl] = s1;
    red[1][g][cl] = s2;
    __syncthreads();
    if (g == 0 && c < C) {
        float a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < 32; ++k) { a1 += red[0][k][cl]; a2 += red[1][k][cl]; }
        if (dbeta) dbeta[c] = a1;
        if (dgamma) dgamma[c] = a2 * rstd;
        if (dbias) dbias[c] = gamma[c] * rstd * a1;
    }
}

// The same over a 2-D grid: block (bx, by) sums the tile range `by` of 32 channels, the last block to arrive per channel group (agent-scope
// counter) adds the NB partials in a fixed order and finalizes.  One block walking T = 2048 tiles took 8 us alone and 20-60 us squeezed
// between the heavy kernels on the side stream.  scratch: [64 counters | (C/32) x NB x 64 partials]; partials and counter move through
// relaxed agent-scope atomics (the blocks sit on different XCDs; a release fence would write back the whole L2).
__global__ void __launch_bounds__(1024) bn_grad_finalize2_kernel(const float* __restrict__ colpart, int T, int C,
                                                                 const float* __restrict__ gamma, float rstd,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                 float* __restrict__ dbias, float* scratch) {
    __shared__ float red[2][32][33];
    __shared__ int s_last;
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    const int NB = gridDim.y, by = blockIdx.y;
    const int tper = (T + NB - 1) / NB, t0 = by * tper, t1 = min(t0 + tper, T);
    float s1 = 0.f, s2 = 0.f;
    if (c < C)
        for (int t = t0 + g; t < t1; t += 32) {
            s1 += colpart[((size_t)t * 2 + 0) * C + c];
            s2 += colpart[((size_t)t * 2 + 1) * C + c];
        }
    red[0][g][cl] = s1;
    red[1][g][cl] = s2;
    __syncthreads();
    unsigned* cnt = reinterpret_cast<unsigned*>(scratch) + blockIdx.x;
    float* part = scratch + 64 + ((size_t)blockIdx.x * NB) * 64;
    if (g < 2) {
        float a = 0.f;
        for (int k = 0; k < 32; ++k) a += red[g][k][cl];
        __hip_atomic_store(part + by * 64 + g * 32 + cl, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) s_last = (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(NB - 1));
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    if (g == 0 && c < C) {
        float a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < NB; ++k) {
            a1 += __hip_atomic_load(part + k * 64 + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a2 += __hip_atomic_load(part + k * 64 + 32 + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (dbeta) dbeta[c] = a1;
        if (dgamma) dgamma[c] = a2 * rstd;
        if (dbias) dbias[c] = gamma[c] * rstd * a1;
    }
}

// Last decoder block's parameter gradients from the summed partials of the fused loss epilogue, red[3C+1] = {dwf[C], S1[C], S2[C], dbf}:
// final conv kernel / bias gradients are copies, the block's BN / bias gradients follow bn_grad_finalize's formulas (one launch instead of two
// device copies + a finalize on the side stream).
__global__ void __launch_bounds__(256) final_gradfin_kernel(const float* __restrict__ red, int C, const float* __restrict__ gamma, float rstd,
                                                            float* __restrict__ dwf, float* __restrict__ dbf, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ dbias) {
    for (int c = threadIdx.x; c < C; c += 256) {
        const float s1 = red[C + c], s2 = red[2 * C + c];
        dwf[c] = red[c];
        if (dbeta) dbeta[c] = s1;
        if (dgamma) dgamma[c] = s2 * rstd;
        if (dbias) dbias[c] = gamma[c] * rstd * s1;
    }
    if (threadIdx.x == 0) dbf[0] = red[3 * C];
}

// ------------------------------------------------------------------------------------------------
// One launch for a layer's parameter-gradient tail on the side stream (UadGradFinish, uad_kernels.h).  The small finalize kernels above are not slow in themselves:
// as launches of their own each is a dependent kernel boundary on the side queue, and a 1024-thread workgroup waits for 16 free wave slots on one CU while the main
// queue's kernels hold the CUs.  Here they are workgroups [0, nfin + nbn) of the slab reduction's grid, 512 threads like its own, placed first.
// Every sum keeps the order of the kernel it replaces, so the results have the same bits.
constexpr int kFinishBnFloats = 64 + 16 * 32 * 64;      // = uad_bn_grad_finalize_scratch_floats(512): counters + BN partials, bn_grad_finalize2_kernel's layout
constexpr int kFinishFinCounter = 32;                   // (the BN part counts in words 0 .. 15)
constexpr int kFinishFinCols = 256;                     // >= 3 fin_C + 1

// BN part, workgroup v = (channel group bx, tile range by): bn_grad_finalize_kernel (NB = 1) / bn_grad_finalize2_kernel with a thread for TWO of their 32 tile lanes
// (g and g + 16, separate accumulators, folded in lane order as there).
__device__ __forceinline__ void finish_bn_block(const UadGradFinish& a, int v, float* lds, int* s_last) {
    float (*red)[32][33] = reinterpret_cast<float (*)[32][33]>(lds);
    const int CG = (a.C + 31) >> 5, NB = a.NB, C = a.C;
    const int bx = v % CG, by = v / CG;
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = bx * 32 + cl;
    const int tper = (a.T + NB - 1) / NB, t0 = by * tper, t1 = min(t0 + tper, a.T);
    float s1 = 0.f, s2 = 0.f, u1 = 0.f, u2 = 0.f;
    if (c < C) {
        int t = t0 + g;
        for (; t + 16 < t1; t += 32) {
            s1 += a.colpart[((size_t)t * 2 + 0) * C + c];
            s2 += a.colpart[((size_t)t * 2 + 1) * C + c];
            u1 += a.colpart[((size_t)(t + 16) * 2 + 0) * C + c];
            u2 += a.colpart[((size_t)(t + 16) * 2 + 1) * C + c];
        }
        if (t < t1) {
            s1 += a.colpart[((size_t)t * 2 + 0) * C + c];
            s2 += a.colpart[((size_t)t * 2 + 1) * C + c];
        }
    }
    red[0][g][cl] = s1; red[0][g + 16][cl] = u1;
    red[1][g][cl] = s2; red[1][g + 16][cl] = u2;
    __syncthreads();
    if (NB == 1) {
        if (g == 0 && c < C) {
            float a1 = 0.f, a2 = 0.f;
            for (int k = 0; k < 32; ++k) { a1 += red[0][k][cl]; a2 += red[1][k][cl]; }
            if (a.dbeta) a.dbeta[c] = a1;
            if (a.dgamma) a.dgamma[c] = a2 * a.rstd;
            if (a.dbias) a.dbias[c] = a.gamma[c] * a.rstd * a1;
        }
        return;
    }
    unsigned* cnt = reinterpret_cast<unsigned*>(a.scratch) + bx;
    float* part = a.scratch + 64 + ((size_t)bx * NB) * 64;
    if (g < 2) {
        float s = 0.f;
        for (int k = 0; k < 32; ++k) s += red[g][k][cl];
        __hip_atomic_store(part + by * 64 + g * 32 + cl, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) *s_last = (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(NB - 1));
    __syncthreads();
    if (!*s_last) return;
    if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    if (g == 0 && c < C) {
        float a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < NB; ++k) {
            a1 += __hip_atomic_load(part + k * 64 + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a2 += __hip_atomic_load(part + k * 64 + 32 + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (a.dbeta) a.dbeta[c] = a1;
        if (a.dgamma) a.dgamma[c] = a2 * a.rstd;
        if (a.dbias) a.dbias[c] = a.gamma[c] * a.rstd * a1;
    }
}

// Fused-final part: the column sum reduce_partials_kernel<SL> (SL = nfin = 4 | 16) makes of fin_partial[fin_T][3 C + 1] in one or two workgroups, spread over SL:
// workgroup f is s-lane f of that kernel, thread (k, j) the k-th of the lane's four interleaved chains of column j.  The last workgroup to arrive folds the SL lane
// sums in index order and writes final_gradfin_kernel's outputs.
__device__ __forceinline__ void finish_final_block(const UadGradFinish& a, int f, float* lds, int* s_last) {
    float (*ch)[kFinishFinCols] = reinterpret_cast<float (*)[kFinishFinCols]>(lds);      // [4][256]
    float* sums = lds + 4 * kFinishFinCols;                                                // [256]
    const int SL = a.nfin, S = a.fin_T, C = a.fin_C, L = 3 * C + 1;
    const int tid = threadIdx.x, jl = tid & 127, k = tid >> 7;
    const float* __restrict__ p = a.fin_partial;
    for (int j = jl; j < kFinishFinCols; j += 128) {
        float acc = 0.f;
        if (j < L) {
            int s = f;
#pragma unroll 4
            for (; s + 3 * SL < S; s += 4 * SL) acc += p[(size_t)(s + k * SL) * L + j];
            if (k == 0) for (; s < S; s += SL) acc += p[(size_t)s * L + j];
        }
        ch[k][j] = acc;
    }
    __syncthreads();
    unsigned* cnt = reinterpret_cast<unsigned*>(a.scratch) + kFinishFinCounter;
    float* part = a.scratch + kFinishBnFloats;
    if (tid < L) {
        __hip_atomic_store(part + f * kFinishFinCols + tid, (ch[0][tid] + ch[1][tid]) + (ch[2][tid] + ch[3][tid]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) *s_last = (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(SL - 1));
    __syncthreads();
    if (!*s_last) return;
    if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < L) {
        float t = 0.f;
        for (int q = 0; q < SL; ++q) t += __hip_atomic_load(part + q * kFinishFinCols + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sums[tid] = t;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 512) {
        const float s1 = sums[C + c], s2 = sums[2 * C + c];
        a.dwf[c] = sums[c];
        if (a.fin_dbeta) a.fin_dbeta[c] = s1;
        if (a.fin_dgamma) a.fin_dgamma[c] = s2 * a.rstd;
        if (a.fin_dbias) a.fin_dbias[c] = a.fin_gamma[c] * a.rstd * s1;
    }
    if (tid == 0) a.dbf[0] = sums[3 * C];
}

// SLAB: the form uad_launch_reduce_partials picks for the slabs (reduce_form below); 0: no slab part
enum { RF_NONE = 0, RF_VEC64, RF_VEC32, RF_VEC16, RF_SCALAR4, RF_SCALAR16 };
template <int SLAB>
__global__ void __launch_bounds__(512) grad_finish_kernel(const UadGradFinish a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 32 * 33];      // 8448 bytes: the BN part's fold, >= 512 float4 of the vector slab forms
    __shared__ int s_last;
    const int b = blockIdx.x;
    if (b < a.nfin) { finish_final_block(a, b, lds, &s_last); return; }
    if (b < a.nfin + a.nbn) { finish_bn_block(a, b - a.nfin, lds, &s_last); return; }
    const int vb = b - a.nfin - a.nbn;
    if constexpr (SLAB == RF_VEC64) reduce4_block<64, 8>(reinterpret_cast<v4f_nt (*)[64]>(lds), vb, a.partial, a.S, a.L, 1.0f, a.dW);
    else if constexpr (SLAB == RF_VEC32) reduce4_block<32, 16>(reinterpret_cast<v4f_nt (*)[32]>(lds), vb, a.partial, a.S, a.L, 1.0f, a.dW);
    else if constexpr (SLAB == RF_VEC16) reduce4_block<16, 32>(reinterpret_cast<v4f_nt (*)[16]>(lds), vb, a.partial, a.S, a.L, 1.0f, a.dW);
    else if constexpr (SLAB == RF_SCALAR4) reduce1_block<128, 4>(reinterpret_cast<float (*)[128]>(lds), vb, a.partial, a.S, a.L, 1.0f, a.dW, 1);
    else if constexpr (SLAB == RF_SCALAR16) reduce1_block<32, 16>(reinterpret_cast<float (*)[32]>(lds), vb, a.partial, a.S, a.L, 1.0f, a.dW, 1);
}

// scratch[rchunk][C] partial column sums; block = 32 channels x 8 row-lanes
__global__ void __launch_bounds__(256) colsum_kernel(const float* __restrict__ g, int rows, int C, int rows_per_chunk,
                                                     float* __restrict__ out) {
    __shared__ float red[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    const int r0 = blockIdx.y * rows_per_chunk;
    const int r1 = min(r0 + rows_per_chunk, rows);
    float s = 0.f;
    if (c < C)
        for (int r = r0 + rl; r < r1; r += 8) s += g[(size_t)r * C + c];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        float a = 0.f;
        for (int k = 0; k < 8; ++k) a += red[k][cl];
        out[(size_t)blockIdx.y * C + c] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// First layer: direct conv for a tiny input-channel count (raw image), weights + input rows staged in LDS.
// Each thread produces 8 output channels of one output pixel.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv_first_fwd_kernel(UadConvDesc d, const float* __restrict__ x,
                                                             const float* __restrict__ W,
                                                             const float* __restrict__ bias, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int CS = d.CS, CB = d.CB, KS = d.KS, S = d.S, P = d.P;
    const int tpp = CS / 8;          // threads per output pixel
    const int ppb = 256 / tpp;       // output pixels per block
    const int nwtaps = KS * KS * CB;
    float* ws = sm;                                  // [nwtaps][CS]
    const int xw = S * ppb + KS;                     // staged input columns (pixels)
    float* xs = sm + nwtaps * CS;                    // [KS][xw][CB]
    const int blocks_per_row = (d.WS + ppb - 1) / ppb;
    const int bx = blockIdx.x % blocks_per_row;
    const int row = blockIdx.x / blocks_per_row;     // n*HS + oy
    const int n = row / d.HS, oy = row % d.HS;
    const int ox0 = bx * ppb;
    for (int i = threadIdx.x; i < nwtaps * CS; i += 256) ws[i] = W[i];
    const int ix0 = S * ox0 - P, iy0 = S * oy - P;
    for (int i = threadIdx.x; i < KS * xw * CB; i += 256) {
        const int cb = i % CB;
        const int t = i / CB;
        const int xx = t % xw, ky = t / xw;
        const int iy = iy0 + ky, ix = ix0 + xx;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)d.HB && (unsigned)ix < (unsigned)d.WB)
            v = x[((size_t)(n * d.HB + iy) * d.WB + ix) * CB + cb];
        xs[i] = v;
    }
    __syncthreads();
    const int p = threadIdx.x / tpp, q = threadIdx.x % tpp;
    const int ox = ox0 + p;
    if (ox >= d.WS) return;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = bias ? bias[q * 8 + e] : 0.f;
    for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx)
            for (int cb = 0; cb < CB; ++cb) {
                const float xv = xs[(ky * xw + S * p + kx) * CB + cb];
                const float4 w0 = *reinterpret_cast<const float4*>(ws + ((ky * KS + kx) * CB + cb) * CS + q * 8);
                const float4 w1 = *reinterpret_cast<const float4*>(ws + ((ky * KS + kx) * CB + cb) * CS + q * 8 + 4);
                acc[0] = fmaf(xv, w0.x, acc[0]); acc[1] = fmaf(xv, w0.y, acc[1]);
                acc[2] = fmaf(xv, w0.z, acc[2]); acc[3] = fmaf(xv, w0.w, acc[3]);
                acc[4] = fmaf(xv, w1.x, acc[4]); acc[5] = fmaf(xv, w1.y, acc[5]);
                acc[6] = fmaf(xv, w1.z, acc[6]); acc[7] = fmaf(xv, w1.w, acc[7]);
            }
    float* o = out + ((size_t)(n * d.HS + oy) * d.WS + ox) * CS + q * 8;
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// First-layer filter gradient: dW[tap][cb][cs] = sum x[..tap..,cb] * g[n,oy,ox,cs].
// Block = CS channel lanes x (256/CS) pixel lanes, walks `rows_per_block` output rows; per-thread accumulators
// for all taps; deterministic LDS reduction over the pixel lanes; one partial slab per block.
template <int KS, int CB>
__global__ void __launch_bounds__(256) conv_first_wgrad_kernel(UadConvDesc d, const float* __restrict__ x,
                                                               const float* __restrict__ g, int rows_per_block,
                                                               float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int NTAP = KS * KS * CB;
    const int CS = d.CS, S = d.S, P = d.P;
    const int G = 256 / CS;
    const int co = threadIdx.x % CS, grp = threadIdx.x / CS;
    const int xw = d.WB + KS + S;                 // padded staged row width (pixels)
    float* xs = sm;                               // [KS][xw][CB]
    float acc[NTAP];
#pragma unroll
    for (int t = 0; t < NTAP; ++t) acc[t] = 0.f;
    const int total_rows = d.N * d.HS;
    const int row0 = blockIdx.x * rows_per_block;
    const int row1 = min(row0 + rows_per_block, total_rows);
    // RB output rows per barrier pair, each with its own KS input rows staged (rows of a group may belong to different
    // samples); the gradient values of a whole group are loaded before any is used (8 x RB independent loads in flight).
    constexpr int RB = 4, OXB = 8;
    for (int rb = row0; rb < row1; rb += RB) {
        __syncthreads();
        for (int i = threadIdx.x; i < RB * KS * xw * CB; i += 256) {
            const int cb = i % CB;
            int t = i / CB;
            const int xx = t % xw; t /= xw;
            const int ky = t % KS, r = t / KS;
            const int row = rb + r;
            float v = 0.f;
            if (row < row1) {
                const int n = row / d.HS, oy = row % d.HS;
                const int iy = S * oy - P + ky, ix = xx - P;
                if ((unsigned)iy < (unsigned)d.HB && (unsigned)ix < (unsigned)d.WB)
                    v = x[((size_t)(n * d.HB + iy) * d.WB + ix) * CB + cb];
            }
            xs[i] = v;
        }
        __syncthreads();
        for (int ob = 0; ob < d.WS; ob += OXB * G) {
            float gv[RB][OXB];
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int i = 0; i < OXB; ++i) {
                    const int ox = ob + grp + i * G;
                    const bool ok = (rb + r < row1) && ox < d.WS;
                    gv[r][i] = ok ? g[((size_t)(rb + r) * d.WS + ox) * CS + co] : 0.f;
                }
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int i = 0; i < OXB; ++i) {
                    const int ox = min(ob + grp + i * G, d.WS - 1);
                    const float* xr = xs + (size_t)r * KS * xw * CB;
#pragma unroll
                    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                        for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                            for (int cb = 0; cb < CB; ++cb)
                                acc[(ky * KS + kx) * CB + cb] =
                                    fmaf(xr[(ky * xw + S * ox + kx) * CB + cb], gv[r][i], acc[(ky * KS + kx) * CB + cb]);
                }
        }
    }
    // reduce over the G pixel lanes (reuse LDS): red[G][NTAP][CS]
    __syncthreads();
    float* red = sm;
#pragma unroll
    for (int t = 0; t < NTAP; ++t) red[(grp * NTAP + t) * CS + co] = acc[t];
    __syncthreads();
    for (int i = threadIdx.x; i < NTAP * CS; i += 256) {
        float a = 0.f;
        for (int k = 0; k < G; ++k) a += red[k * NTAP * CS + i];
        partial[(size_t)blockIdx.x * NTAP * CS + i] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// First layer in the shape every graph of the reference has: 1 input channel, k5 s2 SAME (pad 1 before, 2 after), 32 filters
// (models/autoencoder.py:13-14 via customlayers.build_unified_encoder :8-17).  The generic kernels above are LDS-issue-bound there
// (forward: 15 LDS reads per 40 FMAs, 24 us; filter gradient: 1 LDS read per FMA, 26 us -- for 37 MB of traffic each).
typedef float v2f __attribute__((ext_vector_type(2)));

// forward: block = OR output rows x WS pixels x 32 channels; thread = 4 adjacent pixels x 8 channels of one row.  Per kernel row three
// 16-byte reads fetch the 12 input columns the 4 pixels touch and ten fetch the 5 x 8 weights: 13 reads per 160 FMAs (packed pairs).
template <int WS>
__global__ void __launch_bounds__(256) conv_first_fwd32_kernel(UadConvDesc d, const float* __restrict__ x, const float* __restrict__ W,
                                                               const float* __restrict__ bias, float* __restrict__ out) {
    constexpr int OR = 256 / WS, IR = 2 * OR + 3, XW = 2 * WS + 4;
    __shared__ __attribute__((aligned(16))) float ws[25 * 32];
    __shared__ __attribute__((aligned(16))) float xs[IR * XW];      // column xx holds input column xx - 1
    const int tid = threadIdx.x;
    const int q = tid & 3, pg = (tid >> 2) % (WS / 4), rl = tid / WS;
    const int bpi = d.HS / OR;
    const int n = blockIdx.x / bpi, oy0 = (blockIdx.x % bpi) * OR;
    for (int i = tid; i < 25 * 32; i += 256) ws[i] = W[i];
    for (int i = tid; i < IR * XW; i += 256) {
        const int r = i / XW, xx = i % XW;
        const int iy = 2 * oy0 - 1 + r, ix = xx - 1;
        xs[i] = ((unsigned)iy < (unsigned)d.HB && (unsigned)ix < (unsigned)d.WB) ? x[((size_t)n * d.HB + iy) * d.WB + ix] : 0.f;
    }
    __syncthreads();
    v2f acc[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const v2f b = bias ? v2f{bias[q * 8 + 2 * e], bias[q * 8 + 2 * e + 1]} : v2f{0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][e] = b;
    }
    const float* xr0 = xs + (2 * rl) * XW + 8 * pg;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
        float xv[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<float4*>(xv + 4 * k) = *reinterpret_cast<const float4*>(xr0 + ky * XW + 4 * k);
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            const float4 w0 = *reinterpret_cast<const float4*>(ws + (ky * 5 + kx) * 32 + q * 8);
            const float4 w1 = *reinterpret_cast<const float4*>(ws + (ky * 5 + kx) * 32 + q * 8 + 4);
            const v2f w[4] = {{w0.x, w0.y}, {w0.z, w0.w}, {w1.x, w1.y}, {w1.z, w1.w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const v2f xx = {xv[2 * j + kx], xv[2 * j + kx]};
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = __builtin_elementwise_fma(xx, w[e], acc[j][e]);
            }
        }
    }
    const size_t oe = (((size_t)n * d.HS + oy0 + rl) * WS + 4 * pg) * 32 + q * 8;
    float* o = out + oe;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        *reinterpret_cast<float4*>(o + j * 32) = make_float4(acc[j][0].x, acc[j][0].y, acc[j][1].x, acc[j][1].y);
        *reinterpret_cast<float4*>(o + j * 32 + 4) = make_float4(acc[j][2].x, acc[j][2].y, acc[j][3].x, acc[j][3].y);
    }
}

// filter gradient: thread = 4 channels x one of 32 pixel lanes, 25 x 4 accumulators: one 16-byte gradient load and 25 LDS reads per
// 100 FMAs (packed pairs).  A block takes RPB consecutive output rows of ONE sample (RPB divides HS): their 2 RPB + 3 input rows are
// staged once, the gradient loads of the next row pair are in flight while the current pair is accumulated.  The pixel lanes are
// folded with shuffles inside the wave, then across the 4 waves through LDS, in a fixed order; one partial [25][32] per block, summed
// by reduce_partials.
template <int WS>
__global__ void __launch_bounds__(256) conv_first_wgrad32_kernel(UadConvDesc d, const float* __restrict__ x, const float* __restrict__ g,
                                                                 int RPB, float* __restrict__ partial) {
    constexpr int XW = 2 * WS + 4, NP = WS / 32, MAXR = 16;
    __shared__ __attribute__((aligned(16))) float xs[(2 * MAXR + 3) * XW];
    __shared__ __attribute__((aligned(16))) float red[4][25 * 32];
    const int tid = threadIdx.x, cq = tid & 7, pl = tid >> 3;
    const int row0 = blockIdx.x * RPB;                 // n * HS + oy0
    const int n = row0 / d.HS, oy0 = row0 % d.HS;
    for (int i = tid; i < (2 * RPB + 3) * XW; i += 256) {
        const int r = i / XW, xx = i % XW;
        const int iy = 2 * oy0 - 1 + r, ix = xx - 1;
        xs[i] = ((unsigned)iy < (unsigned)d.HB && (unsigned)ix < (unsigned)d.WB) ? x[((size_t)n * d.HB + iy) * d.WB + ix] : 0.f;
    }
    v2f acc[25][2];
#pragma unroll
    for (int t = 0; t < 25; ++t) { acc[t][0] = v2f{0.f, 0.f}; acc[t][1] = v2f{0.f, 0.f}; }
    const float* gb = g + ((size_t)row0 * WS + pl) * 32 + cq * 4;
    float4 cur[2][NP], nxt[2][NP];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < NP; ++k) cur[r][k] = *reinterpret_cast<const float4*>(gb + ((size_t)r * WS + k * 32) * 32);
    __syncthreads();
    for (int rp = 0; rp < RPB; rp += 2) {
        if (rp + 2 < RPB) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < NP; ++k) nxt[r][k] = *reinterpret_cast<const float4*>(gb + ((size_t)(rp + 2 + r) * WS + k * 32) * 32);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const float* xr = xs + 2 * (rp + r) * XW + 2 * (k * 32 + pl);
                const v2f g0 = {cur[r][k].x, cur[r][k].y}, g1 = {cur[r][k].z, cur[r][k].w};
#pragma unroll
                for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 5; ++kx) {
                        const float xv = xr[ky * XW + kx];
                        const v2f xx = {xv, xv};
                        acc[ky * 5 + kx][0] = __builtin_elementwise_fma(xx, g0, acc[ky * 5 + kx][0]);
                        acc[ky * 5 + kx][1] = __builtin_elementwise_fma(xx, g1, acc[ky * 5 + kx][1]);
                    }
            }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < NP; ++k) cur[r][k] = nxt[r][k];
    }
    // fold the 8 pixel lanes of this wave (lane = cq + 8 * (pl & 7)), then the 4 waves
#pragma unroll
    for (int t = 0; t < 25; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float a = acc[t][h].x, b = acc[t][h].y;
            a += __shfl_xor(a, 8); b += __shfl_xor(b, 8);
            a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);
            a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
            acc[t][h] = v2f{a, b};
        }
    const int wave = tid >> 6;
    if ((tid & 63) < 8) {
#pragma unroll
        for (int t = 0; t < 25; ++t)
            *reinterpret_cast<float4*>(&red[wave][t * 32 + cq * 4]) = make_float4(acc[t][0].x, acc[t][0].y, acc[t][1].x, acc[t][1].y);
    }
    __syncthreads();
    for (int i = tid; i < 25 * 32; i += 256) partial[(size_t)blockIdx.x * 800 + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// ------------------------------------------------------------------------------------------------
// Final 1x1 conv (C -> 1) + L1 loss, fused with its backward.  C/4 lanes per pixel (float4 of channels each).
// reference: models/customlayers.py:37 (dec_Conv2D_final), trainers/VAE.py:36-37,40
// ------------------------------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(256) final_kernel(const UadFinalArgs a, int pix_per_block) {
    __shared__ float red[4][200];  // per-wave partials: 3*C+2 values, C <= 64
    const int lpp = a.C / 4;               // lanes per pixel (8 for C=32)
    const int ppp = 256 / lpp;             // pixels per pass
    const int cl = threadIdx.x % lpp, slot = threadIdx.x / lpp;
    const int n = blockIdx.y;
    const int hw = a.H * a.W;
    const int p0 = blockIdx.x * pix_per_block;
    const int p1 = min(p0 + pix_per_block, hw);
    float4 sc = *reinterpret_cast<const float4*>(a.scale + cl * 4);
    sc.x *= a.mult; sc.y *= a.mult; sc.z *= a.mult; sc.w *= a.mult;
    const float4 sh = *reinterpret_cast<const float4*>(a.shift + cl * 4);
    const float4 wf = *reinterpret_cast<const float4*>(a.wf + cl * 4);
    const float bf = a.bf[0];
    float rec = 0.f, dbf = 0.f;
    float dw[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    // UNR pixels per thread and pass, all loads issued before any use: the kernel is a pure stream (read c, write d_c) and one
    // 16-byte load in flight per lane saturates at ~3.7 TB/s on this chip
    constexpr int UNR = 4;
    auto one_pixel = [&](const size_t pix, const float4 c, const float xv) {
        float bn[4] = {fmaf(c.x, sc.x, sh.x), fmaf(c.y, sc.y, sh.y), fmaf(c.z, sc.z, sh.z), fmaf(c.w, sc.w, sh.w)};
        float av[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = bn[e] > 0.f ? bn[e] : bn[e] * a.alpha;
        float dot = av[0] * wf.x;
        dot = fmaf(av[1], wf.y, dot);
        dot = fmaf(av[2], wf.z, dot);
        dot = fmaf(av[3], wf.w, dot);
        for (int o = 1; o < lpp; o <<= 1) dot += __shfl_xor(dot, o);
        const float xh = dot + bf;
        const float diff = xh - xv;
        if (cl == 0) {
            a.x_hat[pix] = xh;
            if (a.l1_map) a.l1_map[pix] = fabsf(diff);
            rec += fabsf(diff);
        }
        if (BWD) {
            const float s = a.dxhat_in ? a.dxhat_in[pix] : (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * a.inv_batch;
            const float wv[4] = {wf.x, wf.y, wf.z, wf.w};
            const float cv[4] = {c.x, c.y, c.z, c.w};
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w};
            float dc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float da = s * wv[e];
                const float dbn = bn[e] > 0.f ? da : da * a.alpha;
                dc[e] = dbn * scv[e];
                dw[e] = fmaf(s, av[e], dw[e]);
                s1[e] += dbn;
                s2[e] = fmaf(dbn, cv[e], s2[e]);
            }
            *reinterpret_cast<float4*>(a.d_c + pix * a.C + cl * 4) = make_float4(dc[0], dc[1], dc[2], dc[3]);
            if (cl == 0) dbf += s;
        }
    };
    for (int p = p0 + slot; p < p1; p += ppp * UNR) {
        float4 cv[UNR];
        float xv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int pp = min(p + u * ppp, p1 - 1);
            const size_t pix = (size_t)n * hw + pp;
            cv[u] = *reinterpret_cast<const float4*>(a.c_last + pix * a.C + cl * 4);
            xv[u] = a.x[pix];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (p + u * ppp < p1) one_pixel((size_t)n * hw + p + u * ppp, cv[u], xv[u]);
    }
    // reduce over the pixel slots: lanes with equal cl inside the wave, then across the 4 waves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = lpp; o < 64; o <<= 1) {
        rec += __shfl_xor(rec, o);
        if (BWD) {
            dbf += __shfl_xor(dbf, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dw[e] += __shfl_xor(dw[e], o);
                s1[e] += __shfl_xor(s1[e], o);
                s2[e] += __shfl_xor(s2[e], o);
            }
        }
    }
    if (lane < lpp) {
        if (BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red[wave][0 * a.C + lane * 4 + e] = dw[e];
                red[wave][1 * a.C + lane * 4 + e] = s1[e];
                red[wave][2 * a.C + lane * 4 + e] = s2[e];
            }
        }
        if (lane == 0) {
            red[wave][3 * a.C] = dbf;
            red[wave][3 * a.C + 1] = rec;
        }
    }
    __syncthreads();
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const int nred = 3 * a.C + 2;
    if ((int)threadIdx.x < nred) {
        const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if ((int)threadIdx.x == 3 * a.C + 1) a.rec_partial[blk] = v;
        else if (BWD) a.red_partial[(size_t)blk * (3 * a.C + 1) + threadIdx.x] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// VAE bottleneck elementwise: dropout masks, sigma = exp(log_sigma), z = mu + eps*sigma, KL per sample.
// reference: models/variational_autoencoder.py:31-34 ; trainers/VAE.py:38 (KL with log(sigma^2) = 2 log_sigma)
// one wavefront per sample
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) reparam_fwd_kernel(int zdim, int n_vae, const float* __restrict__ mu_raw,
                                                         const float* __restrict__ ls_raw,
                                                         const float* __restrict__ mask_mu,
                                                         const float* __restrict__ mask_ls,
                                                         const float* __restrict__ mask_mu_ce,
                                                         const float* __restrict__ eps, float* __restrict__ mu,
                                                         float* __restrict__ ls, float* __restrict__ sigma,
                                                         float* __restrict__ z, float* __restrict__ kl) {
    const int n = blockIdx.x;
    // samples >= n_vae are the ceVAE context branch: z = z_mu_ce, no sampling, no KL
    // (context_encoder_variational_autoencoder.py:37,43); their log-sigma head is never used.
    const bool ctx = n >= n_vae;
    float acc = 0.f;
    for (int k = threadIdx.x; k < zdim; k += 64) {
        const size_t i = (size_t)n * zdim + k;
        float m = mu_raw[i];
        if (ctx) {
            if (mask_mu_ce) m *= mask_mu_ce[(size_t)(n - n_vae) * zdim + k];
            mu[i] = m; ls[i] = 0.f; sigma[i] = 1.f; z[i] = m;
            continue;
        }
        float l = ls_raw[i];
        if (mask_mu) m *= mask_mu[i];
        if (mask_ls) l *= mask_ls[i];
        const float s = expf(l);
        const float e = eps ? eps[i] : 0.f;
        mu[i] = m; ls[i] = l; sigma[i] = s;
        z[i] = fmaf(e, s, m);
        acc += m * m + s * s - 2.f * l - 1.f;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) kl[n] = 0.5f * acc;
}

__global__ void reparam_bwd_kernel(size_t total, int zdim, int n_vae, const float* __restrict__ dz,
                                   const float* __restrict__ mu, const float* __restrict__ sigma,
                                   const float* __restrict__ eps, const float* __restrict__ mask_mu,
                                   const float* __restrict__ mask_ls, const float* __restrict__ mask_mu_ce,
                                   float inv_batch, float* __restrict__ dmu_raw, float* __restrict__ dls_raw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t n = i / zdim;
    const float g = dz[i];
    if (n >= (size_t)n_vae) {
        dmu_raw[i] = mask_mu_ce ? g * mask_mu_ce[i - (size_t)n_vae * zdim] : g;
        dls_raw[i] = 0.f;
        return;
    }
    const float s = sigma[i];
    const float e = eps ? eps[i] : 0.f;
    float dm = g + mu[i] * inv_batch;
    float dl = g * e * s + (s * s - 1.f) * inv_batch;
    if (mask_mu) dm *= mask_mu[i];
    if (mask_ls) dl *= mask_ls[i];
    dmu_raw[i] = dm;
    dls_raw[i] = dl;
}

__global__ void mul_kernel(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = mask ? x[i] * mask[i] : x[i];
}

// Tiled form for the real layer shape (k5 s2 SAME, 32 output channels): one workgroup per 16x16 input-pixel tile.  The 10x10
// patch of d c0 vectors that the tile touches is staged in LDS once; 8 lanes share a pixel (one float4 of channels each,
// weights of the pixel's parity class in registers, 3-step shuffle reduction).
struct FirstDgradEpi {
    const float* x; const float* x_hat; float inv_batch; float* anomaly; float* dx_out;
    const float* dxhat; float* x_upd; float restore_lr;
};
__device__ __forceinline__ void first_dgrad_store(const FirstDgradEpi& e, size_t pix, float acc) {
    if (e.dxhat) {
        const float gx = acc - e.dxhat[pix];
        if (e.dx_out) e.dx_out[pix] = gx;
        if (e.x_upd) e.x_upd[pix] -= e.restore_lr * gx;
        return;
    }
    if (!e.x) { e.dx_out[pix] = acc; return; }      // plain data gradient (f-AnoGAN critic)
    const float diff = e.x[pix] - e.x_hat[pix];
    const float gx = acc + (diff > 0.f ? e.inv_batch : (diff < 0.f ? -e.inv_batch : 0.f));
    if (e.dx_out) e.dx_out[pix] = gx;
    if (e.anomaly) e.anomaly[pix] = fabsf(diff) * fabsf(gx);
}
template <int PY, int PX>
__device__ __forceinline__ void first_dgrad_class(const float4* sg, const float* __restrict__ W, int cq, int slot, float* sout) {
    constexpr int NKY = PY ? 3 : 2, NKX = PX ? 3 : 2, KY0 = PY ? 0 : 1, KX0 = PX ? 0 : 1;
    float4 w[NKY][NKX];
#pragma unroll
    for (int a = 0; a < NKY; ++a)
#pragma unroll
        for (int b = 0; b < NKX; ++b)
            w[a][b] = *reinterpret_cast<const float4*>(W + ((KY0 + 2 * a) * 5 + (KX0 + 2 * b)) * 32 + cq * 4);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int p = slot + 32 * r, pyy = p >> 3, pxx = p & 7;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < NKY; ++a)
#pragma unroll
            for (int b = 0; b < NKX; ++b) {
                const float4 gv = sg[((pyy - a + 1 + PY) * 10 + (pxx - b + 1 + PX)) * 8 + cq];
                acc = fmaf(gv.x, w[a][b].x, acc); acc = fmaf(gv.y, w[a][b].y, acc);
                acc = fmaf(gv.z, w[a][b].z, acc); acc = fmaf(gv.w, w[a][b].w, acc);
            }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        // park the pixel's data gradient in the tile buffer; the epilogue (all 256 threads, one pixel each, coalesced rows)
        // runs after every parity class is done -- storing from the 8 lanes with cq == 0 used 1/8 of each memory instruction
        if (cq == 0) sout[(2 * pyy + PY) * 16 + 2 * pxx + PX] = acc;
    }
}
__global__ void __launch_bounds__(256) conv_first_dgrad_tiled_kernel(UadConvDesc d, const float* __restrict__ g,
                                                                     const float* __restrict__ W, FirstDgradEpi e) {
    __shared__ float4 sg[10 * 10 * 8];
    __shared__ float sout[16 * 16];
    const int n = blockIdx.z, ty0 = blockIdx.y * 16, tx0 = blockIdx.x * 16;
    const int i0 = ty0 / 2 - 1, j0 = tx0 / 2 - 1;
    for (int idx = threadIdx.x; idx < 800; idx += 256) {
        const int cq = idx & 7, jj = (idx >> 3) % 10, ii = idx / 80;
        const int i = i0 + ii, j = j0 + jj;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)i < (unsigned)d.HS && (unsigned)j < (unsigned)d.WS)
            v = *reinterpret_cast<const float4*>(g + (((size_t)n * d.HS + i) * d.WS + j) * 32 + cq * 4);
        sg[idx] = v;
    }
    __syncthreads();
    const int cq = threadIdx.x & 7, slot = threadIdx.x >> 3;
    first_dgrad_class<0, 0>(sg, W, cq, slot, sout);
    first_dgrad_class<0, 1>(sg, W, cq, slot, sout);
    first_dgrad_class<1, 0>(sg, W, cq, slot, sout);
    first_dgrad_class<1, 1>(sg, W, cq, slot, sout);
    __syncthreads();
    const int y = threadIdx.x >> 4, x = threadIdx.x & 15;
    first_dgrad_store(e, ((size_t)n * d.HB + ty0 + y) * d.WB + tx0 + x, sout[threadIdx.x]);
}

// rec_per_sample[i] = sum_b rec_partial[i][b].  Samples [0,n_vae) carry the VAE-branch losses, [n_vae,n) the ceVAE context
// branch (none for AE/VAE).  scalars = {reconstructionLoss, kl, loss, 0, Rec_vae, Rec_ce, loss_vae, 0}, all divided by the
// user batch (inv_batch); reconstructionLoss = rec_scale * (Rec_vae + Rec_ce)   (trainers/ceVAE.py:45-50)
__global__ void __launch_bounds__(256) loss_finalize_kernel(const float* __restrict__ rec_partial, int n, int n_vae,
                                                            int bps, const float* __restrict__ kl, float inv_batch,
                                                            float rec_scale, float* __restrict__ rec_per_sample,
                                                            float* __restrict__ scalars) {
    __shared__ float sr[256], sc[256], sk[256];
    float ar = 0.f, ac = 0.f, ak = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        float r = 0.f;
        for (int b = 0; b < bps; ++b) r += rec_partial[(size_t)i * bps + b];
        rec_per_sample[i] = r;
        if (i < n_vae) { ar += r; if (kl) ak += kl[i]; }
        else ac += r;
    }
    sr[threadIdx.x] = ar;
    sc[threadIdx.x] = ac;
    sk[threadIdx.x] = ak;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tr = 0.f, tc = 0.f, tk = 0.f;
        for (int i = 0; i < 256; ++i) { tr += sr[i]; tc += sc[i]; tk += sk[i]; }
        scalars[0] = rec_scale * (tr + tc) * inv_batch;
        scalars[1] = tk * inv_batch;
        scalars[2] = (tr + tk + tc) * inv_batch;
        scalars[3] = 0.f;
        scalars[4] = tr * inv_batch;
        scalars[5] = tc * inv_batch;
        scalars[6] = (tr + tk) * inv_batch;
        scalars[7] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// ceVAE anomaly map (trainers/ceVAE.py:51): anomaly = |x - x_hat| * |d loss_vae / d x| with
//   d loss_vae / d x = (data gradient of the first encoder conv) + sign(x - x_hat) / N      (x is also the L1 label)
// One thread per input pixel; it gathers the <= 3x3 output pixels whose 5x5 s2 window covers it (CB = 1).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv_first_dgrad_kernel(UadConvDesc d, const float* __restrict__ g,
                                                               const float* __restrict__ W,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ x_hat, float inv_batch,
                                                               float* __restrict__ anomaly, float* __restrict__ dx_out,
                                                               const float* __restrict__ dxhat, float* __restrict__ x_upd,
                                                               float restore_lr) {
    extern __shared__ __attribute__((aligned(16))) float sw[];     // [KS*KS][CS]
    const int CS = d.CS, KS = d.KS, S = d.S, P = d.P;
    for (int i = threadIdx.x; i < KS * KS * CS; i += 256) sw[i] = W[i];
    __syncthreads();
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)d.N * d.HB * d.WB;
    if (pix >= total) return;
    const int xx = (int)(pix % d.WB);
    const int yy = (int)((pix / d.WB) % d.HB);
    const int n = (int)(pix / ((size_t)d.WB * d.HB));
    float acc = 0.f;
    for (int ky = 0; ky < KS; ++ky) {
        const int ty = yy + P - ky;
        if (ty < 0 || ty % S) continue;
        const int i = ty / S;
        if (i >= d.HS) continue;
        for (int kx = 0; kx < KS; ++kx) {
            const int tx = xx + P - kx;
            if (tx < 0 || tx % S) continue;
            const int j = tx / S;
            if (j >= d.WS) continue;
            const float4* gp = reinterpret_cast<const float4*>(g + ((size_t)(n * d.HS + i) * d.WS + j) * CS);
            const float4* wp = reinterpret_cast<const float4*>(sw + (ky * KS + kx) * CS);
            float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
            for (int c = 0; c < CS / 4; c += 2) {
                const float4 g0 = gp[c], g1 = gp[c + 1];
                const float4 w0 = wp[c], w1 = wp[c + 1];
                a0 = fmaf(g0.x, w0.x, a0); a0 = fmaf(g0.y, w0.y, a0); a0 = fmaf(g0.z, w0.z, a0); a0 = fmaf(g0.w, w0.w, a0);
                a1 = fmaf(g1.x, w1.x, a1); a1 = fmaf(g1.y, w1.y, a1); a1 = fmaf(g1.z, w1.z, a1); a1 = fmaf(g1.w, w1.w, a1);
            }
            acc += a0 + a1;
        }
    }
    if (dxhat) {
        // GMVAE restore objective: x enters it directly only through r = x - x_hat, so its direct gradient is -dxhat
        const float gx = acc - dxhat[pix];
        if (dx_out) dx_out[pix] = gx;
        if (x_upd) x_upd[pix] -= restore_lr * gx;
        return;
    }
    if (!x) { dx_out[pix] = acc; return; }          // plain data gradient
    const float diff = x[pix] - x_hat[pix];
    const float gx = acc + (diff > 0.f ? inv_batch : (diff < 0.f ? -inv_batch : 0.f));
    if (dx_out) dx_out[pix] = gx;
    if (anomaly) anomaly[pix] = fabsf(diff) * fabsf(gx);
}

// TF-1.15 AdamOptimizer update (trainers/DLMODEL.py:112-131): lr_t is computed on the host.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, size_t n, float lr_t, float b1, float b2, float eps, float gscale, const unsigned* __restrict__ fault) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (fault && *fault) return;      // this step's gradients are invalid (timed-out bottleneck exchange): no update; the host reports it (uad_model.hip: check_fault)
    const float gi = g[i] * gscale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
}

// The other optimizers of DLMODEL.create_optimizer (trainers/DLMODEL.py:113-123), TF-1.15 update rules:
//   kind 1 GradientDescentOptimizer            p -= lr g
//   kind 2 MomentumOptimizer(momentum)         a = momentum a + g ; p -= lr a                        (slot a = s1, zero-initialised)
//   kind 3 RMSPropOptimizer(decay .9, momentum, eps 1e-10)   ms = decay ms + (1 - decay) g^2 ; mom = momentum mom + lr g / sqrt(ms + eps) ; p -= mom
//                                                            (slots ms = s2, ONE-initialised by TF, mom = s1)
__global__ void optim_kernel(int kind, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2, size_t n,
                             float lr, float momentum, float decay, float eps, float gscale, const unsigned* __restrict__ fault) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (fault && *fault) return;
    const float gi = g[i] * gscale;
    if (kind == 1) { p[i] -= lr * gi; return; }
    if (kind == 2) { const float a = momentum * s1[i] + gi; s1[i] = a; p[i] -= lr * a; return; }
    const float ms = decay * s2[i] + (1.f - decay) * gi * gi;
    const float mom = momentum * s1[i] + lr * gi / sqrtf(ms + eps);
    s2[i] = ms; s1[i] = mom;
    p[i] -= mom;
}

// residual anomaly map, one block row per sample (utils/Evaluation.py:282-289)
__global__ void __launch_bounds__(256) residual_kernel(const float* __restrict__ x, const float* __restrict__ xr,
                                                       const float* __restrict__ mask, int hw, int pos_only,
                                                       float prior, float* __restrict__ out,
                                                       float* __restrict__ l1part) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    float acc = 0.f;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
        const size_t i = (size_t)n * hw + p;
        const float xv = x[i], d = xv - xr[i];
        acc += fabsf(d);
        float r = pos_only ? fmaxf(d, 0.f) : fabsf(d);
        if (mask) r *= mask[i];
        if (xv < prior) r = 0.f;
        out[i] = r;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && l1part) l1part[(size_t)n * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Spatial autoencoder latent (models/autoencoder_spatial.py:13-17): z = mask * lrelu(gamma' c + beta) of the last encoder block,
// materialised because it is a graph output and the decoder input; backward: d c = d z * mask * lrelu' * gamma', with the
// per-block column sums the BN-gradient finalize expects (colpart[blk][0][ch] = sum d_bn, [1][ch] = sum d_bn * c).
__global__ void __launch_bounds__(256) spatial_z_fwd_kernel(const float* __restrict__ c, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float rs0, float alpha,
                                                            const float* __restrict__ mask, size_t total4, int C, float* __restrict__ z) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int ch = (int)((i * 4) % C);
    const float4 g = *reinterpret_cast<const float4*>(gamma + ch), b = *reinterpret_cast<const float4*>(beta + ch);
    const float4 v = reinterpret_cast<const float4*>(c)[i];
    float4 y = make_float4(fmaf(v.x, g.x * rs0, b.x), fmaf(v.y, g.y * rs0, b.y), fmaf(v.z, g.z * rs0, b.z), fmaf(v.w, g.w * rs0, b.w));
    y = make_float4(y.x > 0.f ? y.x : alpha * y.x, y.y > 0.f ? y.y : alpha * y.y, y.z > 0.f ? y.z : alpha * y.z, y.w > 0.f ? y.w : alpha * y.w);
    if (mask) { const float4 m = reinterpret_cast<const float4*>(mask)[i]; y = make_float4(y.x * m.x, y.y * m.y, y.z * m.z, y.w * m.w); }
    reinterpret_cast<float4*>(z)[i] = y;
}
__global__ void __launch_bounds__(256) spatial_z_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ c,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float rs0,
                                                            float alpha, const float* __restrict__ mask, int rows, int rows_per_block,
                                                            int C, float* __restrict__ dc, float* __restrict__ colpart) {
    __shared__ float r1[1024], r2[1024];
    const int Q = C / 4, RL = 256 / Q;
    const int cq = threadIdx.x % Q, rl = threadIdx.x / Q, ch = cq * 4;
    const float4 g0 = *reinterpret_cast<const float4*>(gamma + ch), b = *reinterpret_cast<const float4*>(beta + ch);
    const float4 g = make_float4(g0.x * rs0, g0.y * rs0, g0.z * rs0, g0.w * rs0);
    const int row0 = blockIdx.x * rows_per_block, row1 = min(rows, row0 + rows_per_block);
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    for (int row = row0 + rl; row < row1; row += RL) {
        const size_t o = (size_t)row * C + ch;
        const float4 cv = *reinterpret_cast<const float4*>(c + o);
        float4 d = *reinterpret_cast<const float4*>(dz + o);
        if (mask) { const float4 m = *reinterpret_cast<const float4*>(mask + o); d = make_float4(d.x * m.x, d.y * m.y, d.z * m.z, d.w * m.w); }
        const float4 dn = make_float4(fmaf(cv.x, g.x, b.x) > 0.f ? d.x : alpha * d.x, fmaf(cv.y, g.y, b.y) > 0.f ? d.y : alpha * d.y,
                                      fmaf(cv.z, g.z, b.z) > 0.f ? d.z : alpha * d.z, fmaf(cv.w, g.w, b.w) > 0.f ? d.w : alpha * d.w);
        *reinterpret_cast<float4*>(dc + o) = make_float4(dn.x * g.x, dn.y * g.y, dn.z * g.z, dn.w * g.w);
        s1 = make_float4(s1.x + dn.x, s1.y + dn.y, s1.z + dn.z, s1.w + dn.w);
        s2 = make_float4(fmaf(dn.x, cv.x, s2.x), fmaf(dn.y, cv.y, s2.y), fmaf(dn.z, cv.z, s2.z), fmaf(dn.w, cv.w, s2.w));
    }
    *reinterpret_cast<float4*>(r1 + rl * C + ch) = s1;
    *reinterpret_cast<float4*>(r2 + rl * C + ch) = s2;
    __syncthreads();
    for (int k = threadIdx.x; k < C; k += 256) {
        float a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < RL; ++j) { a1 += r1[j * C + k]; a2 += r2[j * C + k]; }
        colpart[((size_t)blockIdx.x * 2 + 0) * C + k] = a1;
        colpart[((size_t)blockIdx.x * 2 + 1) * C + k] = a2;
    }
}

// Batch assembly from an HBM-resident slice cache: out[b] = src[idx[b]] (fp32 slices, 16-byte copies) and
// mask[b][p] = lut[labels[idx[b]][p]] (u8 label maps -> 0/1 brain masks, dataloaders/BRAINWEB.py:466-476).
__global__ void __launch_bounds__(256) gather_slices_kernel(const float* __restrict__ src, const int* __restrict__ idx,
                                                            long long slice_f4, float* __restrict__ out) {
    const int b = blockIdx.y;
    const float4* s = reinterpret_cast<const float4*>(src) + (size_t)idx[b] * slice_f4;
    float4* o = reinterpret_cast<float4*>(out) + (size_t)b * slice_f4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slice_f4; i += (long long)gridDim.x * 256) o[i] = s[i];
}
__global__ void __launch_bounds__(256) gather_mask_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ idx,
                                                          long long slice_px, const unsigned char* __restrict__ lut,
                                                          float* __restrict__ out) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut ? (float)lut[threadIdx.x] : (float)threadIdx.x;
    __syncthreads();
    const int b = blockIdx.y;
    const unsigned char* l = labels + (size_t)idx[b] * slice_px;
    float* o = out + (size_t)b * slice_px;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slice_px; i += (long long)gridDim.x * 256) o[i] = s_lut[l[i]];
}

}  // namespace

// ================================================================================================
void uad_launch_spatial_z_fwd(const float* c, const float* gamma, const float* beta, float rs0, float alpha, const float* mask, int rows,
                              int C, float* z, hipStream_t st) {
    const size_t total4 = (size_t)rows * C / 4;
    hipLaunchKernelGGL(spatial_z_fwd_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, c, gamma, beta, rs0, alpha, mask, total4, C, z);
}
int uad_spatial_z_bwd_blocks(int rows) {      // blocks the backward launches (= colpart rows it writes)
    const int nb = rows < 512 ? rows : 512;
    const int rpb = (rows + nb - 1) / nb;
    return (rows + rpb - 1) / rpb;
}
void uad_launch_spatial_z_bwd(const float* dz, const float* c, const float* gamma, const float* beta, float rs0, float alpha,
                              const float* mask, int rows, int C, float* dc, float* colpart, hipStream_t st) {
    const int nb = uad_spatial_z_bwd_blocks(rows);
    const int rpb = (rows + nb - 1) / nb;
    hipLaunchKernelGGL(spatial_z_bwd_kernel, dim3(nb), dim3(256), 0, st, dz, c, gamma, beta, rs0, alpha, mask, rows, rpb, C, dc, colpart);
}
// ------------------------------------------------------------------------------------------------
// Counter-based noise of one step (the reference draws eps / dropout masks inside the TF graph: tf.random_normal,
// keras Dropout; models/variational_autoencoder.py:34, customlayers.py / autoencoder.py dropout layers).  Philox4x32-10 keyed by
// the run seed; the counter is (element quad within the sample, GLOBAL sample index, step, stream id): a sample's noise does not
// depend on which rank draws it or on how the global batch is split, so data-parallel runs reproduce the single-process run
// (SURVEY.md section 8e).  kind 0: N(0,1) by Box-Muller on two 24-bit uniforms; kind 1: inverted-dropout keep mask
// (u >= rate ? 1/(1-rate) : 0, nn.dropout's rule).  One launch fills every array of the step (grid.y = job).
// ------------------------------------------------------------------------------------------------
namespace {
// philox4x32_10, uad_rng_quad and uad_box_muller live in uad_kernels.h: uad_batch.hip adds the same numbers to a batch
struct RngJobs { UadRngJob j[8]; };
__global__ void __launch_bounds__(256) rng_fill_kernel(RngJobs jobs, int n, unsigned k0, unsigned k1, unsigned step_lo, unsigned step_hi,
                                                       long long sample0) {
    const UadRngJob jb = jobs.j[blockIdx.y];
    const int quads = (jb.per_sample + 3) / 4;
    const long long total = (long long)n * quads;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const int s = (int)(q / quads), e4 = (int)(q % quads);
        const unsigned long long gs = (unsigned long long)(sample0 + s);
        unsigned r[4];
        uad_rng_quad((unsigned)e4, gs, step_lo, step_hi, jb.stream, k0, k1, r);
        float v[4];
        if (jb.kind == 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h) uad_box_muller(r[2 * h], r[2 * h + 1], v[2 * h], v[2 * h + 1]);
        } else {
            const float keep = 1.0f / (1.0f - jb.rate);
#pragma unroll
            for (int h = 0; h < 4; ++h) v[h] = ((float)(r[h] >> 8) * 5.9604644775390625e-8f >= jb.rate) ? keep : 0.0f;
        }
        float* o = jb.out + (size_t)s * jb.per_sample + (size_t)e4 * 4;
#pragma unroll
        for (int h = 0; h < 4; ++h) if (e4 * 4 + h < jb.per_sample) o[h] = v[h];
    }
}
}  // namespace

void uad_launch_rng_fill(const UadRngJob* jobs, int njobs, int n, unsigned long long seed, unsigned long long step, long long sample0,
                         hipStream_t st) {
    RngJobs js;
    int maxq = 1;
    for (int i = 0; i < njobs; ++i) { js.j[i] = jobs[i]; const int q = (jobs[i].per_sample + 3) / 4; if (q > maxq) maxq = q; }
    long long blocks = ((long long)n * maxq + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rng_fill_kernel, dim3((unsigned)blocks, njobs), dim3(256), 0, st, js, n, (unsigned)seed, (unsigned)(seed >> 32),
                       (unsigned)step, (unsigned)(step >> 32), sample0);
}

namespace {
// One wave that watches both clocks for `ticks` 100 MHz ticks: out[0] = shader cycles (s_memtime), out[1] = 100 MHz ticks (s_memrealtime).
// Launched on a stream of its own beside a workload it measures the clock the chip actually sustains under that load (DVFS: the 2.4 GHz the
// MFMA peaks are priced at is the ceiling, not what a power-limited kernel mix runs at).  It sleeps between samples: one wave slot, no issue pressure.
__global__ void __launch_bounds__(64) clock_probe_kernel(unsigned long long* out, unsigned long long ticks) {
    const unsigned long long r0 = wall_clock64();
    const unsigned long long c0 = (unsigned long long)clock64();
    unsigned long long r = r0;
    while (r - r0 < ticks) { __builtin_amdgcn_s_sleep(64); r = wall_clock64(); }
    const unsigned long long c1 = (unsigned long long)clock64();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r - r0; }
}
}  // namespace
void uad_launch_clock_probe(unsigned long long* out, unsigned long long ticks, hipStream_t st) {
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, st, out, ticks);
}

void uad_launch_gather_slices(const float* src, const int* idx, int n, long long slice_elems, float* out, hipStream_t st) {
    const long long f4 = slice_elems / 4;
    int bx = (int)((f4 + 255) / 256); if (bx > 64) bx = 64; if (bx < 1) bx = 1;
    hipLaunchKernelGGL(gather_slices_kernel, dim3(bx, n), dim3(256), 0, st, src, idx, f4, out);
}
void uad_launch_gather_mask(const unsigned char* labels, const int* idx, int n, long long slice_px, const unsigned char* lut,
                            float* out, hipStream_t st) {
    int bx = (int)((slice_px + 255) / 256); if (bx > 64) bx = 64; if (bx < 1) bx = 1;
    hipLaunchKernelGGL(gather_mask_kernel, dim3(bx, n), dim3(256), 0, st, labels, idx, slice_px, lut, out);
}
// the form of a slab sum (its summation order): 16-byte lanes with 8 / 16 / 32 slab lanes, or the scalar form with 4 / 16
static int reduce_form(const float* partial, int S, int L, const float* out) {
    static const bool r4 = getenv("UAD_NO_REDUCE4") == nullptr;
    if (r4 && S > 8 && L % 4 == 0 && L >= 1024 && ((uintptr_t)partial & 15) == 0 && ((uintptr_t)out & 15) == 0) {
        const int L4 = L / 4;
        return (L4 + 63) / 64 >= 256 ? RF_VEC64 : (L4 + 31) / 32 >= 256 ? RF_VEC32 : RF_VEC16;
    }
    return ((L + 63) / 64 >= 256 || S <= 8) ? RF_SCALAR4 : RF_SCALAR16;
}
void uad_launch_reduce_partials(const float* partial, int S, int L, float scale, float* out, hipStream_t st) {
    const int blocks = (L + 63) / 64, L4 = L / 4;
    // streaming (non-temporal) loads: the slabs are read exactly once; plain loads pushed 52 MB per launch through the L2s the heavy kernels
    // on the main stream were working out of (same-box A/B, round 3: 0.945 -> 0.926 ms per step).
    constexpr int nt = 1;
    switch (reduce_form(partial, S, L, out)) {
    case RF_VEC64: hipLaunchKernelGGL((reduce_partials4_kernel<64, 8>), dim3((L4 + 63) / 64), dim3(512), 0, st, partial, S, L, scale, out); break;
    case RF_VEC32: hipLaunchKernelGGL((reduce_partials4_kernel<32, 16>), dim3((L4 + 31) / 32), dim3(512), 0, st, partial, S, L, scale, out); break;
    case RF_VEC16: hipLaunchKernelGGL((reduce_partials4_kernel<16, 32>), dim3((L4 + 15) / 16), dim3(512), 0, st, partial, S, L, scale, out); break;
    case RF_SCALAR4: hipLaunchKernelGGL((reduce_partials_kernel<4>), dim3(blocks), dim3(256), 0, st, partial, S, L, scale, out, nt); break;
    default: hipLaunchKernelGGL((reduce_partials_kernel<16>), dim3(blocks), dim3(1024), 0, st, partial, S, L, scale, out, nt); break;
    }
}

bool uad_grad_finish_takes(int C, int fin_C) { return C <= 512 && 3 * fin_C + 1 <= kFinishFinCols; }
size_t uad_grad_finish_scratch_floats() { return (size_t)kFinishBnFloats + 16 * kFinishFinCols; }
void uad_launch_grad_finish(const UadGradFinish& in, hipStream_t st) {
    UadGradFinish a = in;
    if (!a.fin_partial) a.fin_C = 0;
    if (!a.colpart) a.C = 0;
    if (!uad_grad_finish_takes(a.C, a.fin_C)) { fprintf(stderr, "uad: grad_finish does not take C = %d, fin_C = %d (uad_grad_finish_takes)\n", a.C, a.fin_C); abort(); }
    a.nfin = a.fin_partial ? (a.fin_T <= 8 ? 4 : 16) : 0;      // reduce_form of a [fin_T][<= 256] sum
    a.NB = a.T >= 2048 ? 32 : a.T >= 512 ? 16 : a.T >= 128 ? 8 : 1;      // uad_launch_bn_grad_finalize's tile ranges
    a.nbn = a.colpart ? ((a.C + 31) / 32) * a.NB : 0;
    const int form = (a.partial && a.S > 0) ? reduce_form(a.partial, a.S, a.L, a.dW) : RF_NONE;
    const int L4 = a.L / 4;
    const int nslab = form == RF_VEC64 ? (L4 + 63) / 64 : form == RF_VEC32 ? (L4 + 31) / 32 : form == RF_VEC16 ? (L4 + 15) / 16
                      : form == RF_SCALAR4 ? (a.L + 127) / 128 : form == RF_SCALAR16 ? (a.L + 31) / 32 : 0;
    const dim3 grid(a.nfin + a.nbn + nslab);
    if (!grid.x) return;
    switch (form) {
    case RF_VEC64: hipLaunchKernelGGL(grad_finish_kernel<RF_VEC64>, grid, dim3(512), 0, st, a); break;
    case RF_VEC32: hipLaunchKernelGGL(grad_finish_kernel<RF_VEC32>, grid, dim3(512), 0, st, a); break;
    case RF_VEC16: hipLaunchKernelGGL(grad_finish_kernel<RF_VEC16>, grid, dim3(512), 0, st, a); break;
    case RF_SCALAR4: hipLaunchKernelGGL(grad_finish_kernel<RF_SCALAR4>, grid, dim3(512), 0, st, a); break;
    case RF_SCALAR16: hipLaunchKernelGGL(grad_finish_kernel<RF_SCALAR16>, grid, dim3(512), 0, st, a); break;
    default: hipLaunchKernelGGL(grad_finish_kernel<RF_NONE>, grid, dim3(512), 0, st, a); break;
    }
}

void uad_launch_final_gradfin(const float* red, int C, const float* gamma, float rstd, float* dwf, float* dbf, float* dgamma, float* dbeta,
                              float* dbias, hipStream_t st) {
    hipLaunchKernelGGL(final_gradfin_kernel, dim3(1), dim3(256), 0, st, red, C, gamma, rstd, dwf, dbf, dgamma, dbeta, dbias);
}
// one workspace serves every launch of a stream: size it for the widest layer it will see (counters: first 64 words)
size_t uad_bn_grad_finalize_scratch_floats(int C) { return 64 + (size_t)((C + 31) / 32) * 32 * 64; }
void uad_launch_bn_grad_finalize(const float* colpart, int T, int C, const float* gamma, float rstd, float* dgamma,
                                 float* dbeta, float* dbias, hipStream_t st, float* scratch) {
    const int NB = T >= 2048 ? 32 : T >= 512 ? 16 : T >= 128 ? 8 : 1;
    if (scratch && NB > 1 && C <= 512) {          // callers size the scratch with uad_bn_grad_finalize_scratch_floats(512)
        hipLaunchKernelGGL(bn_grad_finalize2_kernel, dim3((C + 31) / 32, NB), dim3(1024), 0, st, colpart, T, C, gamma, rstd, dgamma, dbeta, dbias, scratch);
        return;
    }
    hipLaunchKernelGGL(bn_grad_finalize_kernel, dim3((C + 31) / 32), dim3(1024), 0, st, colpart, T, C, gamma, rstd,
                       dgamma, dbeta, dbias);
}

// Row chunks of a column sum.  Round 5: up to 1024 (was 64) as long as the partials fit the 64 x 1024-float scratch every handle allocates: the ResNet f-AnoGAN
// graph sums [393 k rows x 64 channels] tensors (100 MB) for its residual-stream bias gradients with 2 x 64 = 128 workgroups -- half the CUs, 1.8 TB/s, 3 % of an
// iteration (profiles/r04_z_fanogan_resnet64_kernel_stats.csv).  UAD_COLSUM_CHUNKS=n caps it (64: the old plan).
static inline int colsum_chunks(int rows, int C) {
    static const int cap_env = getenv("UAD_COLSUM_CHUNKS") ? atoi(getenv("UAD_COLSUM_CHUNKS")) : 0;
    int cap = cap_env > 0 ? cap_env : 1024;
    const int fit = (int)kUadColsumScratchFloats / (C < 1 ? 1 : C);
    if (cap > fit) cap = fit;
    if (cap < 1) cap = 1;
    int ch = (rows + 255) / 256;
    return ch < 1 ? 1 : (ch > cap ? cap : ch);
}
size_t uad_colsum_scratch_floats(int rows, int C) { return (size_t)colsum_chunks(rows, C) * C; }

void uad_launch_colsum(const float* g, int rows, int C, float* out, float* scratch, hipStream_t st) {
    const int ch = colsum_chunks(rows, C);
    const int rpc = (rows + ch - 1) / ch;
    dim3 grid((C + 31) / 32, ch);
    if (ch == 1) {
        hipLaunchKernelGGL(colsum_kernel, grid, dim3(256), 0, st, g, rows, C, rpc, out);
    } else {
        hipLaunchKernelGGL(colsum_kernel, grid, dim3(256), 0, st, g, rows, C, rpc, scratch);
        uad_launch_reduce_partials(scratch, ch, C, 1.0f, out, st);
    }
}

// the specialised first-layer kernels: 1 -> 32 channels, k5 s2 SAME on an even square-ish grid
static inline bool first32_ok(const UadConvDesc& d) {
    static const bool off = getenv("UAD_NO_FIRST32") != nullptr;
    return !off && d.CB == 1 && d.CS == 32 && d.KS == 5 && d.S == 2 && d.P == 1 && d.HB == 2 * d.HS && d.WB == 2 * d.WS &&
           (d.WS == 32 || d.WS == 64 || d.WS == 128) && d.HS % 8 == 0;
}
void uad_launch_conv_first_fwd(const UadConvDesc& d, const float* x, const float* W, const float* bias, float* out,
                               hipStream_t st) {
    const int tpp = d.CS / 8, ppb = 256 / tpp;
    const int xw = d.S * ppb + d.KS;
    const size_t lds = ((size_t)d.KS * d.KS * d.CB * d.CS + (size_t)d.KS * xw * d.CB) * sizeof(float);
    const int bpr = (d.WS + ppb - 1) / ppb;
    if (first32_ok(d)) {
        if (d.WS == 32) hipLaunchKernelGGL(conv_first_fwd32_kernel<32>, dim3(d.N * d.HS / 8), dim3(256), 0, st, d, x, W, bias, out);
        else if (d.WS == 64) hipLaunchKernelGGL(conv_first_fwd32_kernel<64>, dim3(d.N * d.HS / 4), dim3(256), 0, st, d, x, W, bias, out);
        else hipLaunchKernelGGL(conv_first_fwd32_kernel<128>, dim3(d.N * d.HS / 2), dim3(256), 0, st, d, x, W, bias, out);
        return;
    }
    hipLaunchKernelGGL(conv_first_fwd_kernel, dim3(d.N * d.HS * bpr), dim3(256), lds, st, d, x, W, bias, out);
}

static inline int first_wgrad_rows_per_block(const UadConvDesc& d) {
    const int total = d.N * d.HS;
    if (first32_ok(d)) {              // 4, 8 or 16 rows of one sample per block (the fold of the pixel lanes costs as much as ~3 rows)
        const int want = (total + 511) / 512;
        return (want > 8 && d.HS % 16 == 0) ? 16 : want > 4 ? 8 : 4;
    }
    int rpb = (total + 1023) / 1024;
    return rpb < 1 ? 1 : rpb;
}
size_t uad_conv_first_wgrad_partial_floats(const UadConvDesc& d) {
    const int rpb = first_wgrad_rows_per_block(d);
    const int blocks = (d.N * d.HS + rpb - 1) / rpb;
    return (size_t)blocks * d.KS * d.KS * d.CB * d.CS;
}
void uad_launch_conv_first_wgrad(const UadConvDesc& d, const float* x, const float* g, float* dW, float* partial,
                                 hipStream_t st) {
    const int rpb = first_wgrad_rows_per_block(d);
    const int blocks = (d.N * d.HS + rpb - 1) / rpb;
    const int ntap = d.KS * d.KS * d.CB;
    const int G = 256 / d.CS;
    const int xw = d.WB + d.KS + d.S;
    size_t lds_x = (size_t)4 * d.KS * xw * d.CB, lds_r = (size_t)G * ntap * d.CS;
    const size_t lds = (lds_x > lds_r ? lds_x : lds_r) * sizeof(float);
    if (first32_ok(d)) {
        if (d.WS == 32) hipLaunchKernelGGL(conv_first_wgrad32_kernel<32>, dim3(blocks), dim3(256), 0, st, d, x, g, rpb, partial);
        else if (d.WS == 64) hipLaunchKernelGGL(conv_first_wgrad32_kernel<64>, dim3(blocks), dim3(256), 0, st, d, x, g, rpb, partial);
        else hipLaunchKernelGGL(conv_first_wgrad32_kernel<128>, dim3(blocks), dim3(256), 0, st, d, x, g, rpb, partial);
    } else if (d.KS == 5 && d.CB == 1)
        hipLaunchKernelGGL((conv_first_wgrad_kernel<5, 1>), dim3(blocks), dim3(256), lds, st, d, x, g, rpb, partial);
    else if (d.KS == 5 && d.CB == 3)
        hipLaunchKernelGGL((conv_first_wgrad_kernel<5, 3>), dim3(blocks), dim3(256), lds, st, d, x, g, rpb, partial);
    else if (d.KS == 3 && d.CB == 1)
        hipLaunchKernelGGL((conv_first_wgrad_kernel<3, 1>), dim3(blocks), dim3(256), lds, st, d, x, g, rpb, partial);
    else if (d.KS == 4 && d.CB == 1)
        hipLaunchKernelGGL((conv_first_wgrad_kernel<4, 1>), dim3(blocks), dim3(256), lds, st, d, x, g, rpb, partial);
    else
        return;  // validated by the caller (uad_model.hip)
    uad_launch_reduce_partials(partial, blocks, ntap * d.CS, 1.0f, dW, st);
}

int uad_final_blocks_per_sample(int H, int W) {
    const int hw = H * W;
    int bps = hw / 512;
    return bps < 1 ? 1 : bps;
}
void uad_launch_final_fwd_bwd(const UadFinalArgs& a, hipStream_t st) {
    const int bps = uad_final_blocks_per_sample(a.H, a.W);
    const int ppb = (a.H * a.W + bps - 1) / bps;
    dim3 grid(bps, a.N);
    if (a.d_c)
        hipLaunchKernelGGL((final_kernel<true>), grid, dim3(256), 0, st, a, ppb);
    else
        hipLaunchKernelGGL((final_kernel<false>), grid, dim3(256), 0, st, a, ppb);
}

void uad_launch_reparam_fwd(int n, int n_vae, int zdim, const float* mu_raw, const float* ls_raw, const float* mask_mu,
                            const float* mask_ls, const float* mask_mu_ce, const float* eps, float* mu, float* ls,
                            float* sigma, float* z, float* kl_per_sample, hipStream_t st) {
    hipLaunchKernelGGL(reparam_fwd_kernel, dim3(n), dim3(64), 0, st, zdim, n_vae, mu_raw, ls_raw, mask_mu, mask_ls,
                       mask_mu_ce, eps, mu, ls, sigma, z, kl_per_sample);
}
void uad_launch_reparam_bwd(int n, int n_vae, int zdim, const float* dz, const float* mu, const float* sigma,
                            const float* eps, const float* mask_mu, const float* mask_ls, const float* mask_mu_ce,
                            float inv_batch, float* dmu_raw, float* dls_raw, hipStream_t st) {
    const size_t total = (size_t)n * zdim;
    hipLaunchKernelGGL(reparam_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, st, total, zdim, n_vae, dz, mu,
                       sigma, eps, mask_mu, mask_ls, mask_mu_ce, inv_batch, dmu_raw, dls_raw);
}
static bool first_dgrad_tiled_ok(const UadConvDesc& d) {
    return d.KS == 5 && d.S == 2 && d.P == 1 && d.CB == 1 && d.CS == 32 && d.HB % 16 == 0 && d.WB % 16 == 0 &&
           d.HB == 2 * d.HS && d.WB == 2 * d.WS && d.N <= 65535;
}
bool uad_conv_first_dgrad_tiled(const UadConvDesc& d) { return first_dgrad_tiled_ok(d); }
void uad_launch_conv_first_dgrad(const UadConvDesc& d, const float* g, const float* W, const float* x,
                                 const float* x_hat, float inv_batch, float* anomaly, float* dx, hipStream_t st, bool generic) {
    if (!generic && first_dgrad_tiled_ok(d)) {
        FirstDgradEpi e{x, x_hat, inv_batch, anomaly, dx, nullptr, nullptr, 0.f};
        hipLaunchKernelGGL(conv_first_dgrad_tiled_kernel, dim3(d.WB / 16, d.HB / 16, d.N), dim3(256), 0, st, d, g, W, e);
        return;
    }
    const size_t total = (size_t)d.N * d.HB * d.WB;
    hipLaunchKernelGGL(conv_first_dgrad_kernel, dim3((total + 255) / 256), dim3(256),
                       (size_t)d.KS * d.KS * d.CS * sizeof(float), st, d, g, W, x, x_hat, inv_batch, anomaly, dx,
                       (const float*)nullptr, (float*)nullptr, 0.f);
}
void uad_launch_conv_first_dgrad_restore(const UadConvDesc& d, const float* g, const float* W, const float* dxhat,
                                         float* dx, float* x_upd, float restore_lr, hipStream_t st, bool generic) {
    if (!generic && first_dgrad_tiled_ok(d)) {
        FirstDgradEpi e{nullptr, nullptr, 0.f, nullptr, dx, dxhat, x_upd, restore_lr};
        hipLaunchKernelGGL(conv_first_dgrad_tiled_kernel, dim3(d.WB / 16, d.HB / 16, d.N), dim3(256), 0, st, d, g, W, e);
        return;
    }
    const size_t total = (size_t)d.N * d.HB * d.WB;
    hipLaunchKernelGGL(conv_first_dgrad_kernel, dim3((total + 255) / 256), dim3(256),
                       (size_t)d.KS * d.KS * d.CS * sizeof(float), st, d, g, W, (const float*)nullptr,
                       (const float*)nullptr, 0.f, (float*)nullptr, dx, dxhat, x_upd, restore_lr);
}
void uad_launch_conv_first_dgrad_plain(const UadConvDesc& d, const float* g, const float* W, float* dx, hipStream_t st) {
    uad_launch_conv_first_dgrad(d, g, W, nullptr, nullptr, 0.f, nullptr, dx, st);
}
void uad_launch_mul(const float* x, const float* mask, float* y, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(mul_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, mask, y, n);
}
void uad_launch_loss_finalize(const float* rec_partial, int n, int n_vae, int bps, const float* kl_per_sample,
                              float inv_batch, float rec_scale, float* rec_per_sample, float* scalars, hipStream_t st) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, rec_partial, n, n_vae, bps, kl_per_sample,
                       inv_batch, rec_scale, rec_per_sample, scalars);
}
void uad_launch_optim(int kind, float* p, const float* g, float* s1, float* s2, size_t n, float lr, float momentum, float decay, float eps,
                      float gscale, hipStream_t st, const unsigned* fault) {
    hipLaunchKernelGGL(optim_kernel, dim3((n + 255) / 256), dim3(256), 0, st, kind, p, g, s1, s2, n, lr, momentum, decay, eps, gscale, fault);
}
void uad_launch_adam(float* p, const float* g, float* m, float* v, size_t n, float lr_t, float beta1, float beta2,
                     float eps, float gscale, hipStream_t st, const unsigned* fault) {
    hipLaunchKernelGGL(adam_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p, g, m, v, n, lr_t, beta1, beta2, eps,
                       gscale, fault);
}
void uad_launch_residual(const float* x, const float* xr, const float* mask, int n, int hw, int pos_only,
                         float prior_thresh, float* out, float* l1err, hipStream_t st) {
    // one block per sample keeps the per-sample |x - xr| sum a single deterministic partial
    hipLaunchKernelGGL(residual_kernel, dim3(1, n), dim3(256), 0, st, x, xr, mask, hw, pos_only, prior_thresh, out,
                       l1err);
}
