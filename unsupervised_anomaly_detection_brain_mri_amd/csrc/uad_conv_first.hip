// The first encoder layer (raw image in, tiny input-channel count): direct conv forward, filter gradient and data gradient, each in a generic form and in the
// form of the shape every graph has (1 -> 32 channels, k5 s2 SAME), with the policy that picks between them (first32_ok, first_wgrad_rows_per_block,
// first_dgrad_tiled_ok).  The filter gradient's slabs are summed by uad_launch_reduce_partials (uad_reduce.hip).  Switch: UAD_NO_FIRST32.
#include "uad_kernels.h"
#include <stdlib.h>
#include <type_traits>

namespace {

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

}  // namespace

// the specialised first-layer kernels: 1 -> 32 channels, k5 s2 SAME on an even square-ish grid
static inline bool first32_ok(const UadConvDesc& d) {
    static const bool off = getenv("UAD_NO_FIRST32") != nullptr;
    return !off && d.CB == 1 && d.CS == 32 && d.KS == 5 && d.S == 2 && d.P == 1 && d.HB == 2 * d.HS && d.WB == 2 * d.WS &&
           (d.WS == 32 || d.WS == 64 || d.WS == 128) && d.HS % 8 == 0;
}
// the WS instance of the fwd32 / wgrad32 pair for a first32_ok shape: f receives WS as an integral constant
template <class F>
static void dispatch_ws32(int WS, F f) {
    if (WS == 32) f(std::integral_constant<int, 32>{});
    else if (WS == 64) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 128>{});
}
void uad_launch_conv_first_fwd(const UadConvDesc& d, const float* x, const float* W, const float* bias, float* out,
                               hipStream_t st) {
    const int tpp = d.CS / 8, ppb = 256 / tpp;
    const int xw = d.S * ppb + d.KS;
    const size_t lds = ((size_t)d.KS * d.KS * d.CB * d.CS + (size_t)d.KS * xw * d.CB) * sizeof(float);
    const int bpr = (d.WS + ppb - 1) / ppb;
    if (first32_ok(d)) {      // a block takes 256 / WS output rows
        dispatch_ws32(d.WS, [&](auto ws) {
            constexpr int WS = decltype(ws)::value;
            hipLaunchKernelGGL(conv_first_fwd32_kernel<WS>, dim3(d.N * d.HS / (256 / WS)), dim3(256), 0, st, d, x, W, bias, out);
        });
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
    if (first32_ok(d))
        dispatch_ws32(d.WS, [&](auto ws) {
            hipLaunchKernelGGL(conv_first_wgrad32_kernel<decltype(ws)::value>, dim3(blocks), dim3(256), 0, st, d, x, g, rpb, partial);
        });
    else if (d.KS == 5 && d.CB == 1)
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

static bool first_dgrad_tiled_ok(const UadConvDesc& d) {
    return d.KS == 5 && d.S == 2 && d.P == 1 && d.CB == 1 && d.CS == 32 && d.HB % 16 == 0 && d.WB % 16 == 0 &&
           d.HB == 2 * d.HS && d.WB == 2 * d.WS && d.N <= 65535;
}
bool uad_conv_first_dgrad_tiled(const UadConvDesc& d) { return first_dgrad_tiled_ok(d); }
// one launcher for the three epilogue forms (first_dgrad_store): the tiled kernel takes the struct, the generic kernel its fields
static void launch_first_dgrad(const UadConvDesc& d, const float* g, const float* W, const FirstDgradEpi& e, bool generic, hipStream_t st) {
    if (!generic && first_dgrad_tiled_ok(d)) {
        hipLaunchKernelGGL(conv_first_dgrad_tiled_kernel, dim3(d.WB / 16, d.HB / 16, d.N), dim3(256), 0, st, d, g, W, e);
        return;
    }
    const size_t total = (size_t)d.N * d.HB * d.WB;
    hipLaunchKernelGGL(conv_first_dgrad_kernel, dim3((total + 255) / 256), dim3(256), (size_t)d.KS * d.KS * d.CS * sizeof(float), st, d, g, W,
                       e.x, e.x_hat, e.inv_batch, e.anomaly, e.dx_out, e.dxhat, e.x_upd, e.restore_lr);
}
void uad_launch_conv_first_dgrad(const UadConvDesc& d, const float* g, const float* W, const float* x,
                                 const float* x_hat, float inv_batch, float* anomaly, float* dx, hipStream_t st, bool generic) {
    launch_first_dgrad(d, g, W, FirstDgradEpi{x, x_hat, inv_batch, anomaly, dx, nullptr, nullptr, 0.f}, generic, st);
}
void uad_launch_conv_first_dgrad_restore(const UadConvDesc& d, const float* g, const float* W, const float* dxhat,
                                         float* dx, float* x_upd, float restore_lr, hipStream_t st, bool generic) {
    launch_first_dgrad(d, g, W, FirstDgradEpi{nullptr, nullptr, 0.f, nullptr, dx, dxhat, x_upd, restore_lr}, generic, st);
}
void uad_launch_conv_first_dgrad_plain(const UadConvDesc& d, const float* g, const float* W, float* dx, hipStream_t st) {
    launch_first_dgrad(d, g, W, FirstDgradEpi{nullptr, nullptr, 0.f, nullptr, dx, nullptr, nullptr, 0.f}, false, st);
}
