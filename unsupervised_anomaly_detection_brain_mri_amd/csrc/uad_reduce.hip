// Deterministic sums of the train step's partial results (no float atomics on data): the slab reductions behind the split filter gradients, the BN / bias
// gradient finalize, the one-launch gradient finish of the side stream (grad_finish_kernel: the same sums as workgroups of one grid) and the column sum.
// Owns the launch rules that keep the fused launch bit-identical to the launches it replaces: the form of a slab sum (reduce_form, kRf) and the tile ranges of
// the BN finalize (bn_tile_ranges).  Switches: UAD_NO_REDUCE4, UAD_COLSUM_CHUNKS.
#include "uad_kernels.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

namespace {

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

}  // namespace

// ================================================================================================
// The lane split of each form of a slab sum, stated once (indexed by RF_*): a thread takes `cols` adjacent columns (one 16-byte quad in the vector forms), a workgroup is
// jl column lanes x sl slab lanes, and sl alone fixes a column's summation order.  The stand-alone kernels (reduce_partials4_kernel<jl, sl>, reduce_partials_kernel<sl>)
// and the slab workgroups of grad_finish_kernel run the same block bodies.  The vector forms have one shape in both hosts.  The two scalar forms keep sl and differ in jl:
// reduce_partials_kernel is 64 columns wide whatever sl (256 / 1024 threads), grad_finish_kernel is 512 threads whatever the form (jl_fused: the shapes its chain names).
struct RfSplit { int cols, sl, jl, jl_fused; };
constexpr RfSplit kRf[] = {{1, 0, 0, 0}, {4, 8, 64, 64}, {4, 16, 32, 32}, {4, 32, 16, 16}, {1, 4, 64, 128}, {1, 16, 64, 32}};
static_assert(kRf[RF_VEC64].jl_fused * kRf[RF_VEC64].sl == 512 && kRf[RF_VEC32].jl_fused * kRf[RF_VEC32].sl == 512 && kRf[RF_VEC16].jl_fused * kRf[RF_VEC16].sl == 512 &&
              kRf[RF_SCALAR4].jl_fused * kRf[RF_SCALAR4].sl == 512 && kRf[RF_SCALAR16].jl_fused * kRf[RF_SCALAR16].sl == 512, "grad_finish_kernel is 512 threads");
// workgroups a form spends on L columns, alone or as the slab part of grad_finish_kernel
static int rf_blocks(int form, int L, bool fused) {
    const int c = kRf[form].cols * (fused ? kRf[form].jl_fused : kRf[form].jl);
    return c ? (L + c - 1) / c : 0;
}
// the form of a slab sum (its summation order): 16-byte lanes with 8 / 16 / 32 slab lanes, or the scalar form with 4 / 16
static int reduce_form_scalar(int S, int L) { return (rf_blocks(RF_SCALAR4, L, false) >= 256 || S <= 8) ? RF_SCALAR4 : RF_SCALAR16; }
static int reduce_form(const float* partial, int S, int L, const float* out) {
    static const bool r4 = getenv("UAD_NO_REDUCE4") == nullptr;
    if (r4 && S > 8 && L % 4 == 0 && L >= 1024 && ((uintptr_t)partial & 15) == 0 && ((uintptr_t)out & 15) == 0)
        return rf_blocks(RF_VEC64, L, false) >= 256 ? RF_VEC64 : rf_blocks(RF_VEC32, L, false) >= 256 ? RF_VEC32 : RF_VEC16;
    return reduce_form_scalar(S, L);
}
void uad_launch_reduce_partials(const float* partial, int S, int L, float scale, float* out, hipStream_t st) {
    const int form = reduce_form(partial, S, L, out);
    const dim3 grid(rf_blocks(form, L, false)), block(kRf[form].jl * kRf[form].sl);
    // streaming (non-temporal) loads: the slabs are read exactly once; plain loads pushed 52 MB per launch through the L2s the heavy kernels
    // on the main stream were working out of (same-box A/B, round 3: 0.945 -> 0.926 ms per step).
    constexpr int nt = 1;
    static_assert(kRf[RF_SCALAR4].jl == 64 && kRf[RF_SCALAR16].jl == 64, "reduce_partials_kernel is 64 columns wide");
    switch (form) {
    case RF_VEC64: hipLaunchKernelGGL((reduce_partials4_kernel<kRf[RF_VEC64].jl, kRf[RF_VEC64].sl>), grid, block, 0, st, partial, S, L, scale, out); break;
    case RF_VEC32: hipLaunchKernelGGL((reduce_partials4_kernel<kRf[RF_VEC32].jl, kRf[RF_VEC32].sl>), grid, block, 0, st, partial, S, L, scale, out); break;
    case RF_VEC16: hipLaunchKernelGGL((reduce_partials4_kernel<kRf[RF_VEC16].jl, kRf[RF_VEC16].sl>), grid, block, 0, st, partial, S, L, scale, out); break;
    case RF_SCALAR4: hipLaunchKernelGGL((reduce_partials_kernel<kRf[RF_SCALAR4].sl>), grid, block, 0, st, partial, S, L, scale, out, nt); break;
    default: hipLaunchKernelGGL((reduce_partials_kernel<kRf[RF_SCALAR16].sl>), grid, block, 0, st, partial, S, L, scale, out, nt); break;
    }
}

// tile ranges of the BN / bias finalize (bn_grad_finalize2_kernel's grid.y, UadGradFinish::NB): one statement for the stand-alone launch and the fused one
static int bn_tile_ranges(int T) { return T >= 2048 ? 32 : T >= 512 ? 16 : T >= 128 ? 8 : 1; }

bool uad_grad_finish_takes(int C, int fin_C) { return C <= 512 && 3 * fin_C + 1 <= kFinishFinCols; }
size_t uad_grad_finish_scratch_floats() { return (size_t)kFinishBnFloats + 16 * kFinishFinCols; }
void uad_launch_grad_finish(const UadGradFinish& in, hipStream_t st) {
    UadGradFinish a = in;
    if (!a.fin_partial) a.fin_C = 0;
    if (!a.colpart) a.C = 0;
    if (!uad_grad_finish_takes(a.C, a.fin_C)) { fprintf(stderr, "uad: grad_finish does not take C = %d, fin_C = %d (uad_grad_finish_takes)\n", a.C, a.fin_C); abort(); }
    a.nfin = a.fin_partial ? kRf[reduce_form_scalar(a.fin_T, 3 * a.fin_C + 1)].sl : 0;      // one workgroup per slab lane of the [fin_T][3 fin_C + 1] sum's form
    a.NB = bn_tile_ranges(a.T);
    a.nbn = a.colpart ? ((a.C + 31) / 32) * a.NB : 0;
    const int form = (a.partial && a.S > 0) ? reduce_form(a.partial, a.S, a.L, a.dW) : RF_NONE;
    const dim3 grid(a.nfin + a.nbn + rf_blocks(form, a.L, true));
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
    const int NB = bn_tile_ranges(T);
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
