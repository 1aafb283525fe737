// Implicit-GEMM convolution kernels for gfx950 (CDNA4), fp32 in / fp32 accumulate on the
// matrix cores (v_mfma_f32_32x32x2_f32: exact f32, 157 TFLOP/s chip peak).
//
// Three kernel families cover every contraction on the AE/VAE hot path
// (reference: models/customlayers.py:16-38 Conv2D / Conv2DTranspose k5 s2 SAME, the 1x1 convs and
//  Dense layers of models/variational_autoencoder.py:20-36, and their tf.gradients):
//   F ("gather")  : small[n,i,j,cs]            = sum_tap,cb big[n,S*i-P+ky,S*j-P+kx,cb] * W[tap][cb][cs]
//   D ("scatter") : big[n,S*i-P+ky,S*j-P+kx,cb] += small[n,i,j,cs] * W[tap][cb][cs]   (per output-parity class)
//   W ("filter")  : dW[tap][cb][cs]             = sum_n,i,j big[..tap..,cb] * small[n,i,j,cs]
// Layout: NHWC activations, W[tap][cb][cs] weights (HWIO for Conv2D, [kh,kw,Cout,Cin] for Conv2DTranspose),
// so the channel (contraction) axis is always contiguous: 16-byte coalesced global loads, one 128-B line per
// pixel per 32 channels.  Tiles are staged global -> VGPR -> LDS (double buffered, one barrier per K-step) because
// the producer layer's frozen-BN affine + LeakyReLU is applied on load (activation tensors are stored once, pre-BN).
// The 64-lane wavefront owns (32*FM)x(32*FN) of the block tile; K is walked 8 at a time with the lane-half
// permutation k = 8*kk + 4*(lane>>5) + s so that one ds_read_b128 feeds four MFMAs.
//
// This unit owns the generic family: conv_gemm_kernel / conv_gemm16_kernel (any KS / S / P), the split-K epilogue, the generic filter gradient and the weight
// packs.  The k5 s2 and k3 specialisations are units of their own (uad_conv5_f / _d / _w.hip, uad_gemm_d16s*.hip, uad_conv_k3.hip); which kernel a launch
// runs is decided in uad_conv_plan.hip, which calls the uad_gemm_launch* functions below.
#include <stdint.h>
#include "uad_gemm_common.h"

namespace {

template <int BM, int BN, int BK, int WGM, int WGN, int KIND>
__global__ void __launch_bounds__(64 * WGM * WGN) conv_gemm_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int FM = WTM / 32, FN = WTN / 32;
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of the 32x32 MFMA");
    static_assert(BK % 8 == 0, "BK multiple of 8");
    constexpr int NKK = BK / 8;
    constexpr int LDA = BK + 4;  // (LDA/4) odd -> conflict-free ds_read_b128 across 16-lane groups
    constexpr int LDB = (KIND == KIND_F) ? (BN + 4) : (BK + 4);
    constexpr int A_EL = BM * LDA;
    constexpr int B_EL = (KIND == KIND_F) ? (BK * LDB) : (BN * LDB);
    constexpr int STAGE = A_EL + B_EL;
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    __shared__ __attribute__((aligned(16))) float s_xf[2 * XF_LDS_CH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const UadConvDesc& d = a.d;
    const int S = d.S, P = d.P, KS = d.KS;

    // ---- tap set: all KS*KS taps (F) or the taps of this output-parity class (D) ----
    int py = 0, px = 0, ky0 = 0, kx0 = 0, nty = KS, ntx = KS, dy0 = 0, dx0 = 0;
    const int nsplit = a.nsplit;
    const int split = (KIND == KIND_D) ? (int)(blockIdx.z % nsplit) : (int)blockIdx.z;
    if (KIND == KIND_D) {
        const int cz = blockIdx.z / nsplit;
        py = (S - 1) - cz / S;
        px = (S - 1) - cz % S;
        ky0 = (py + P) % S;
        kx0 = (px + P) % S;
        dy0 = (py + P) / S;
        dx0 = (px + P) / S;
        nty = ky0 < KS ? (KS - ky0 + S - 1) / S : 0;
        ntx = kx0 < KS ? (KS - kx0 + S - 1) / S : 0;
    }
    const int ntaps = nty * ntx;
    const int ncc = a.CA / BK;
    const int nk = ntaps * ncc;
    // split-K: this workgroup contracts K-steps [ks0, ks1)
    const int kper = (nk + nsplit - 1) / nsplit;
    const int ks0 = split * kper;
    const int ks1 = min(nk, ks0 + kper);

    // ---- activation-on-load tables -> LDS (once) ----
    const bool xf = a.xf.scale != nullptr;
    if (xf) {
        for (int c = tid; c < a.CA; c += NT) {
            s_xf[c] = a.xf.scale[c] * a.xf.mult;
            s_xf[XF_LDS_CH + c] = a.xf.shift[c];
        }
    }

    // ---- per-thread A rows (positions) ----
    constexpr int TPR = BK / 4, RPP = NT / TPR, PA = (BM + RPP - 1) / RPP;
    const int acol = (tid % TPR) * 4;
    const int arow0 = tid / TPR;
    int rbase[PA], ry[PA], rx[PA];
    bool rok[PA];
#pragma unroll
    for (int q = 0; q < PA; ++q) {
        const int r = arow0 + q * RPP;
        const int m = m0 + r;
        rok[q] = (r < BM) && (m < a.M);
        int n, i, j;
        decode_pos(rok[q] ? m : 0, d.HS, d.WS, a.lhs, a.lws, n, i, j);
        if (KIND == KIND_F) {
            rbase[q] = n * d.HB * d.WB;
            ry[q] = S * i - P;
            rx[q] = S * j - P;
        } else {
            rbase[q] = n * d.HS * d.WS;
            ry[q] = i;
            rx[q] = j;
        }
    }
    const int AH = (KIND == KIND_F) ? d.HB : d.HS;
    const int AW = (KIND == KIND_F) ? d.WB : d.WS;

    // ---- per-thread B slots (predicates are loop invariant; out-of-range slots read element 0 and are zeroed) ----
    constexpr int TPRB = (KIND == KIND_F) ? (BN / 4) : (BK / 4);
    constexpr int RPB = NT / TPRB;
    constexpr int BROWS = (KIND == KIND_F) ? BK : BN;
    constexpr int PB = (BROWS + RPB - 1) / RPB;
    const int bcol = (tid % TPRB) * 4;
    const int brow0 = tid / TPRB;
    bool bok[PB];
    int boff[PB];   // loop-invariant part of the weight offset
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const int r = brow0 + q * RPB;
        if (KIND == KIND_F) {
            bok[q] = (r < BK) && (n0 + bcol) < a.Nn;
            boff[q] = bok[q] ? (r * d.CS + n0 + bcol) : 0;
        } else {
            bok[q] = (r < BN) && (n0 + r) < a.Nn;
            boff[q] = bok[q] ? ((n0 + r) * d.CS + bcol) : 0;
        }
    }

    float4 va[PA], vb[PB];
    unsigned okbits = 0;
    int xc0 = 0;

    // branch-free tile fetch: every load is issued unconditionally from a clamped (always valid) address
    auto load_tiles = [&](int tap, int c0) {
        int ky, kx, oy, ox;
        {
            const int ty = tap / ntx, tx = tap - ty * ntx;
            if (KIND == KIND_F) { ky = ty; kx = tx; oy = ky; ox = kx; }
            else { ky = ky0 + S * ty; kx = kx0 + S * tx; oy = dy0 - ty; ox = dx0 - tx; }
        }
        xc0 = c0;
        okbits = 0;
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int y = ry[q] + oy, x = rx[q] + ox;
            const bool ok = rok[q] && (unsigned)y < (unsigned)AH && (unsigned)x < (unsigned)AW;
            const int pix = ok ? (rbase[q] + y * AW + x) : 0;
            va[q] = *reinterpret_cast<const float4*>(a.A + (size_t)pix * a.CA + c0 + acol);
            okbits |= (ok ? 1u : 0u) << q;
        }
        const int tapw = ky * KS + kx;
        const size_t wbase = (KIND == KIND_F) ? ((size_t)tapw * d.CB + c0) * d.CS : ((size_t)tapw * d.CB) * d.CS + c0;
#pragma unroll
        for (int q = 0; q < PB; ++q) vb[q] = *reinterpret_cast<const float4*>(a.W + wbase + boff[q]);
    };
    auto store_tiles = [&](int buf) {
        float* sA = smem + buf * STAGE;
        float* sB = sA + A_EL;
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (xf) {
            sc = *reinterpret_cast<const float4*>(s_xf + xc0 + acol);
            sh = *reinterpret_cast<const float4*>(s_xf + XF_LDS_CH + xc0 + acol);
        }
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int r = arow0 + q * RPP;
            float4 v = va[q];
            if (xf) v = xform4(v, sc, sh, a.xf.alpha);
            // padding pixels stay exactly 0 (the pad is applied to the ACTIVATED tensor)
            v = keep4((okbits >> q) & 1u, v);
            if (r < BM) *reinterpret_cast<float4*>(sA + r * LDA + acol) = v;
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
            const int r = brow0 + q * RPB;
            const float4 v = keep4(bok[q], vb[q]);
            if (r < BROWS) *reinterpret_cast<float4*>(sB + r * LDB + bcol) = v;
        }
    };

    v16f acc[FM][FN];
#pragma unroll
    for (int im = 0; im < FM; ++im)
#pragma unroll
        for (int jn = 0; jn < FN; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[im][jn][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;

    __syncthreads();   // s_xf visible
    int tap = ks0 / ncc, cc = ks0 - tap * ncc;
    if (ks0 < ks1) {
        load_tiles(tap, cc * BK);
        store_tiles(0);
    }
    __syncthreads();

    // fragment double buffer: the ds_reads of k-slice kk+1 are in flight while the MFMAs of kk issue
    float4 af[2][FM];
    float bf[2][FN][4];
    auto load_frags = [&](int slot, const float* sA, const float* sB, int kk) {
#pragma unroll
        for (int im = 0; im < FM; ++im)
            af[slot][im] = *reinterpret_cast<const float4*>(sA + (wm * WTM + im * 32 + l31) * LDA + kk * 8 + 4 * lh);
#pragma unroll
        for (int jn = 0; jn < FN; ++jn) {
            if (KIND == KIND_F) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    bf[slot][jn][s] = sB[(kk * 8 + 4 * lh + s) * LDB + wn * WTN + jn * 32 + l31];
            } else {
                const float4 t = *reinterpret_cast<const float4*>(sB + (wn * WTN + jn * 32 + l31) * LDB + kk * 8 + 4 * lh);
                bf[slot][jn][0] = t.x; bf[slot][jn][1] = t.y; bf[slot][jn][2] = t.z; bf[slot][jn][3] = t.w;
            }
        }
    };

    for (int ks = ks0; ks < ks1; ++ks) {
        const int buf = (ks - ks0) & 1;
        int ntap = tap, ncc_ = cc + 1;
        if (ncc_ == ncc) { ncc_ = 0; ntap = tap + 1; }
        const bool more = (ks + 1 < ks1);
        const float* sA = smem + buf * STAGE;
        const float* sB = sA + A_EL;
        load_frags(0, sA, sB, 0);
        if (more) load_tiles(ntap, ncc_ * BK);
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const int cur = kk & 1;
            if (kk + 1 < NKK) load_frags(cur ^ 1, sA, sB, kk + 1);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int im = 0; im < FM; ++im) {
                    const float av = (s == 0) ? af[cur][im].x : (s == 1) ? af[cur][im].y : (s == 2) ? af[cur][im].z : af[cur][im].w;
#pragma unroll
                    for (int jn = 0; jn < FN; ++jn)
                        acc[im][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[cur][jn][s], acc[im][jn], 0, 0, 0);
                }
            }
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
        tap = ntap;
        cc = ncc_;
    }

    // ---------------------------------------------------------------- epilogue
    if (nsplit > 1) {
        // raw partial tile into this split's slab (output layout); bias / activation-backward / column sums are
        // applied by splitk_epilogue_kernel after the slabs are summed in a fixed order
        float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
        for (int im = 0; im < FM; ++im)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = m0 + row;
                if (m >= a.M) continue;
                size_t ob;
                if (KIND == KIND_F) ob = (size_t)m * a.Nn;
                else {
                    int n, i, j;
                    decode_pos(m, d.HS, d.WS, a.lhs, a.lws, n, i, j);
                    ob = ((size_t)(n * d.HB + S * i + py) * d.WB + (S * j + px)) * a.Nn;
                }
#pragma unroll
                for (int jn = 0; jn < FN; ++jn) {
                    const int col = n0 + wn * WTN + jn * 32 + l31;
                    if (col < a.Nn) slab[ob + col] = acc[im][jn][r];
                }
            }
        return;
    }
    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    // per-lane column constants
    bool colok[FN];
    int colc[FN];
    float c_a[FN], c_b[FN];   // !bwd: bias, -- ; bwd: escale*emult, eshift
#pragma unroll
    for (int jn = 0; jn < FN; ++jn) {
        const int col = n0 + wn * WTN + jn * 32 + l31;
        colok[jn] = col < a.Nn;
        colc[jn] = colok[jn] ? col : 0;
        if (!bwd) {
            c_a[jn] = a.ep.bias ? a.ep.bias[colc[jn]] : 0.f;
            c_b[jn] = 0.f;
        } else {
            c_a[jn] = a.ep.escale[colc[jn]] * a.ep.emult;
            c_b[jn] = a.ep.eshift[colc[jn]];
        }
    }
    float s1[FN], s2[FN];
#pragma unroll
    for (int jn = 0; jn < FN; ++jn) { s1[jn] = 0.f; s2[jn] = 0.f; }

#pragma unroll
    for (int im = 0; im < FM; ++im) {
        // row bases of this fragment's 16 rows
        size_t obase[16];
        bool rowok[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int m = m0 + row;
            rowok[r] = m < a.M;
            const int mc = rowok[r] ? m : 0;
            if (KIND == KIND_F) {
                obase[r] = (size_t)mc * a.Nn;
            } else {
                int n, i, j;
                decode_pos(mc, d.HS, d.WS, a.lhs, a.lws, n, i, j);
                obase[r] = ((size_t)(n * d.HB + S * i + py) * d.WB + (S * j + px)) * a.Nn;
            }
        }
        if (!bwd) {
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!(rowok[r] && colok[jn])) continue;
                    const size_t off = obase[r] + colc[jn];
                    float v = acc[im][jn][r] + c_a[jn];
                    if (a.ep.mul) v *= a.ep.mul[off];
                    if (a.ep.add) v += a.ep.add[off];
                    a.Out[off] = v;
                }
            }
        } else {
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
                // all 16 c_prev loads of this fragment are issued before the first one is consumed
                float cp[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = rowok[r] && colok[jn];
                    cp[r] = a.ep.cprev[ok ? (obase[r] + colc[jn]) : 0];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = rowok[r] && colok[jn];
                    const float c = cp[r];
                    const float bn = fmaf(c_a[jn], c, c_b[jn]);
                    const float v = acc[im][jn][r];
                    float dbn = bn > 0.f ? v : v * a.ep.ealpha;
                    dbn = ok ? dbn : 0.f;
                    if (ok) a.Out[obase[r] + colc[jn]] = dbn * c_a[jn];
                    s1[jn] += dbn;
                    s2[jn] = fmaf(dbn, c, s2[jn]);
                }
            }
        }
    }
    if (bwd) {
        // column sums: lane halves -> waves along M -> one partial row per block tile
        float* red = smem;  // [WGM][2][BN]
        __syncthreads();
#pragma unroll
        for (int jn = 0; jn < FN; ++jn) {
            float t1 = s1[jn] + __shfl_xor(s1[jn], 32);
            float t2 = s2[jn] + __shfl_xor(s2[jn], 32);
            if (lh == 0) {
                red[(wm * 2 + 0) * BN + wn * WTN + jn * 32 + l31] = t1;
                red[(wm * 2 + 1) * BN + wn * WTN + jn * 32 + l31] = t2;
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += red[(w * 2 + which) * BN + c];
            const int col = n0 + c;
            const size_t tile = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
            if (col < a.Nn) a.ep.colpart[(tile * 2 + which) * a.Nn + col] = t;
        }
    }
}

// ---- generic (any KS / S / P) contraction in bf16x3 math: the fp32 tiles are split into bf16 hi | lo planes while they are stored
// to LDS (same bytes as fp32), both operands K-contiguous, so a fragment is one ds_read_b128 per plane and a K = 16 slice costs
// three v_mfma_f32_32x32x16_bf16 instead of eight fp32 MFMAs.  Identity activation-on-load only.
template <int BM, int BN, int BK, int WGM, int WGN, int KIND>
__global__ void __launch_bounds__(64 * WGM * WGN) conv_gemm16_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int FM = WTM / 32, FN = WTN / 32;
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of the 32x32 MFMA");
    static_assert(BK % 16 == 0, "BK multiple of 16");
    constexpr int NKK = BK / 16;
    constexpr int LDK = BK + 8;                        // bf16 row stride (80 B at BK = 32): 16-byte aligned rows
    constexpr int A_EL = BM * LDK, B_EL = BN * LDK;    // per plane; both operands are stored K-contiguous
    constexpr int STAGE = 2 * A_EL + 2 * B_EL;         // A hi | A lo | B hi | B lo
    __shared__ __attribute__((aligned(16))) unsigned short smem16[2 * STAGE];
    float* const smem = reinterpret_cast<float*>(smem16);   // epilogue scratch

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const UadConvDesc& d = a.d;
    const int S = d.S, P = d.P, KS = d.KS;

    // ---- tap set: all KS*KS taps (F) or the taps of this output-parity class (D) ----
    int py = 0, px = 0, ky0 = 0, kx0 = 0, nty = KS, ntx = KS, dy0 = 0, dx0 = 0;
    const int nsplit = a.nsplit;
    const int split = (KIND == KIND_D) ? (int)(blockIdx.z % nsplit) : (int)blockIdx.z;
    if (KIND == KIND_D) {
        const int cz = blockIdx.z / nsplit;
        py = (S - 1) - cz / S;
        px = (S - 1) - cz % S;
        ky0 = (py + P) % S;
        kx0 = (px + P) % S;
        dy0 = (py + P) / S;
        dx0 = (px + P) / S;
        nty = ky0 < KS ? (KS - ky0 + S - 1) / S : 0;
        ntx = kx0 < KS ? (KS - kx0 + S - 1) / S : 0;
    }
    const int ntaps = nty * ntx;
    const int ncc = a.CA / BK;
    const int nk = ntaps * ncc;
    // split-K: this workgroup contracts K-steps [ks0, ks1)
    const int kper = (nk + nsplit - 1) / nsplit;
    const int ks0 = split * kper;
    const int ks1 = min(nk, ks0 + kper);

    // (no activation-on-load in this variant: the launcher only selects it for identity transforms)

    // ---- per-thread A rows (positions) ----
    constexpr int TPR = BK / 4, RPP = NT / TPR, PA = (BM + RPP - 1) / RPP;
    const int acol = (tid % TPR) * 4;
    const int arow0 = tid / TPR;
    int rbase[PA], ry[PA], rx[PA];
    bool rok[PA];
#pragma unroll
    for (int q = 0; q < PA; ++q) {
        const int r = arow0 + q * RPP;
        const int m = m0 + r;
        rok[q] = (r < BM) && (m < a.M);
        int n, i, j;
        decode_pos(rok[q] ? m : 0, d.HS, d.WS, a.lhs, a.lws, n, i, j);
        if (KIND == KIND_F) {
            rbase[q] = n * d.HB * d.WB;
            ry[q] = S * i - P;
            rx[q] = S * j - P;
        } else {
            rbase[q] = n * d.HS * d.WS;
            ry[q] = i;
            rx[q] = j;
        }
    }
    const int AH = (KIND == KIND_F) ? d.HB : d.HS;
    const int AW = (KIND == KIND_F) ? d.WB : d.WS;

    // ---- per-thread B slots (predicates are loop invariant; out-of-range slots read element 0 and are zeroed) ----
    constexpr int TPRB = (KIND == KIND_F) ? (BN / 4) : (BK / 4);
    constexpr int RPB = NT / TPRB;
    constexpr int BROWS = (KIND == KIND_F) ? BK : BN;
    constexpr int PB = (BROWS + RPB - 1) / RPB;
    static_assert(KIND != KIND_F || PB == 2, "F-type: each thread owns two adjacent K rows of the weight tile");
    const int bcol = (tid % TPRB) * 4;
    const int brow0 = tid / TPRB;
    // F-type: rows (2*brow0, 2*brow0+1) so that the transposed LDS store writes one 32-bit pair per output column
    auto brow = [&](int q) { return (KIND == KIND_F) ? (brow0 * PB + q) : (brow0 + q * RPB); };
    bool bok[PB];
    int boff[PB];   // loop-invariant part of the weight offset
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const int r = brow(q);
        if (KIND == KIND_F) {
            bok[q] = (r < BK) && (n0 + bcol) < a.Nn;
            boff[q] = bok[q] ? (r * d.CS + n0 + bcol) : 0;
        } else {
            bok[q] = (r < BN) && (n0 + r) < a.Nn;
            boff[q] = bok[q] ? ((n0 + r) * d.CS + bcol) : 0;
        }
    }

    float4 va[PA], vb[PB];
    unsigned okbits = 0;
    int xc0 = 0;

    // branch-free tile fetch: every load is issued unconditionally from a clamped (always valid) address
    auto load_tiles = [&](int tap, int c0) {
        int ky, kx, oy, ox;
        {
            const int ty = tap / ntx, tx = tap - ty * ntx;
            if (KIND == KIND_F) { ky = ty; kx = tx; oy = ky; ox = kx; }
            else { ky = ky0 + S * ty; kx = kx0 + S * tx; oy = dy0 - ty; ox = dx0 - tx; }
        }
        xc0 = c0;
        okbits = 0;
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int y = ry[q] + oy, x = rx[q] + ox;
            const bool ok = rok[q] && (unsigned)y < (unsigned)AH && (unsigned)x < (unsigned)AW;
            const int pix = ok ? (rbase[q] + y * AW + x) : 0;
            va[q] = *reinterpret_cast<const float4*>(a.A + (size_t)pix * a.CA + c0 + acol);
            okbits |= (ok ? 1u : 0u) << q;
        }
        const int tapw = ky * KS + kx;
        const size_t wbase = (KIND == KIND_F) ? ((size_t)tapw * d.CB + c0) * d.CS : ((size_t)tapw * d.CB) * d.CS + c0;
#pragma unroll
        for (int q = 0; q < PB; ++q) vb[q] = *reinterpret_cast<const float4*>(a.W + wbase + boff[q]);
    };
    auto store_tiles = [&](int buf) {
        unsigned short* sAh = smem16 + buf * STAGE;
        unsigned short* sAl = sAh + A_EL;
        unsigned short* sBh = sAl + A_EL;
        unsigned short* sBl = sBh + B_EL;
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int r = arow0 + q * RPP;
            // padding pixels stay exactly 0
            const float4 v = keep4((okbits >> q) & 1u, va[q]);
            uint2 hi, lo;
            split_bf16(v, hi, lo);
            if (r < BM) {
                *reinterpret_cast<uint2*>(sAh + r * LDK + acol) = hi;
                *reinterpret_cast<uint2*>(sAl + r * LDK + acol) = lo;
            }
        }
        if (KIND == KIND_F) {
            // W tile arrives [k][n]; the matrix cores want n-major rows with K contiguous: transposed store, one (k, k+1) pair per n
            uint2 h0, l0, h1, l1;
            split_bf16(keep4(bok[0], vb[0]), h0, l0);
            split_bf16(keep4(bok[PB - 1], vb[PB - 1]), h1, l1);
            const unsigned hh0[4] = {h0.x & 0xFFFFu, h0.x >> 16, h0.y & 0xFFFFu, h0.y >> 16};
            const unsigned hh1[4] = {h1.x & 0xFFFFu, h1.x >> 16, h1.y & 0xFFFFu, h1.y >> 16};
            const unsigned ll0[4] = {l0.x & 0xFFFFu, l0.x >> 16, l0.y & 0xFFFFu, l0.y >> 16};
            const unsigned ll1[4] = {l1.x & 0xFFFFu, l1.x >> 16, l1.y & 0xFFFFu, l1.y >> 16};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<unsigned*>(sBh + (bcol + i) * LDK + 2 * brow0) = hh0[i] | (hh1[i] << 16);
                *reinterpret_cast<unsigned*>(sBl + (bcol + i) * LDK + 2 * brow0) = ll0[i] | (ll1[i] << 16);
            }
        } else {
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int r = brow0 + q * RPB;
                uint2 hi, lo;
                split_bf16(keep4(bok[q], vb[q]), hi, lo);
                if (r < BROWS) {
                    *reinterpret_cast<uint2*>(sBh + r * LDK + bcol) = hi;
                    *reinterpret_cast<uint2*>(sBl + r * LDK + bcol) = lo;
                }
            }
        }
    };

    v16f acc[FM][FN];
#pragma unroll
    for (int im = 0; im < FM; ++im)
#pragma unroll
        for (int jn = 0; jn < FN; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[im][jn][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;

    int tap = ks0 / ncc, cc = ks0 - tap * ncc;
    if (ks0 < ks1) {
        load_tiles(tap, cc * BK);
        store_tiles(0);
    }
    __syncthreads();

    // fragment double buffer: the ds_reads of k-slice kk+1 are in flight while the MFMAs of kk issue
    uint4 ah[2][FM], al[2][FM], bh[2][FN], bl[2][FN];
    auto load_frags = [&](int slot, const unsigned short* sAh, int kk) {
        const unsigned short* sAl = sAh + A_EL;
        const unsigned short* sBh = sAl + A_EL;
        const unsigned short* sBl = sBh + B_EL;
#pragma unroll
        for (int im = 0; im < FM; ++im) {
            const int o = (wm * WTM + im * 32 + l31) * LDK + kk * 16 + 8 * lh;
            ah[slot][im] = *reinterpret_cast<const uint4*>(sAh + o);
            al[slot][im] = *reinterpret_cast<const uint4*>(sAl + o);
        }
#pragma unroll
        for (int jn = 0; jn < FN; ++jn) {
            const int o = (wn * WTN + jn * 32 + l31) * LDK + kk * 16 + 8 * lh;
            bh[slot][jn] = *reinterpret_cast<const uint4*>(sBh + o);
            bl[slot][jn] = *reinterpret_cast<const uint4*>(sBl + o);
        }
    };

    for (int ks = ks0; ks < ks1; ++ks) {
        const int buf = (ks - ks0) & 1;
        int ntap = tap, ncc_ = cc + 1;
        if (ncc_ == ncc) { ncc_ = 0; ntap = tap + 1; }
        const bool more = (ks + 1 < ks1);
        const unsigned short* sA = smem16 + buf * STAGE;
        load_frags(0, sA, 0);
        if (more) load_tiles(ntap, ncc_ * BK);
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const int cur = kk & 1;
            if (kk + 1 < NKK) load_frags(cur ^ 1, sA, kk + 1);
#pragma unroll
            for (int im = 0; im < FM; ++im)
#pragma unroll
                for (int jn = 0; jn < FN; ++jn) {
                    acc[im][jn] = mfma_bf16(ah[cur][im], bh[cur][jn], acc[im][jn]);
                    acc[im][jn] = mfma_bf16(ah[cur][im], bl[cur][jn], acc[im][jn]);
                    acc[im][jn] = mfma_bf16(al[cur][im], bh[cur][jn], acc[im][jn]);
                }
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
        tap = ntap;
        cc = ncc_;
    }

    // ---------------------------------------------------------------- epilogue
    if (nsplit > 1) {
        // raw partial tile into this split's slab (output layout); bias / activation-backward / column sums are
        // applied by splitk_epilogue_kernel after the slabs are summed in a fixed order
        float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
        for (int im = 0; im < FM; ++im)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = m0 + row;
                if (m >= a.M) continue;
                size_t ob;
                if (KIND == KIND_F) ob = (size_t)m * a.Nn;
                else {
                    int n, i, j;
                    decode_pos(m, d.HS, d.WS, a.lhs, a.lws, n, i, j);
                    ob = ((size_t)(n * d.HB + S * i + py) * d.WB + (S * j + px)) * a.Nn;
                }
#pragma unroll
                for (int jn = 0; jn < FN; ++jn) {
                    const int col = n0 + wn * WTN + jn * 32 + l31;
                    if (col < a.Nn) slab[ob + col] = acc[im][jn][r];
                }
            }
        return;
    }
    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    // per-lane column constants
    bool colok[FN];
    int colc[FN];
    float c_a[FN], c_b[FN];   // !bwd: bias, -- ; bwd: escale*emult, eshift
#pragma unroll
    for (int jn = 0; jn < FN; ++jn) {
        const int col = n0 + wn * WTN + jn * 32 + l31;
        colok[jn] = col < a.Nn;
        colc[jn] = colok[jn] ? col : 0;
        if (!bwd) {
            c_a[jn] = a.ep.bias ? a.ep.bias[colc[jn]] : 0.f;
            c_b[jn] = 0.f;
        } else {
            c_a[jn] = a.ep.escale[colc[jn]] * a.ep.emult;
            c_b[jn] = a.ep.eshift[colc[jn]];
        }
    }
    float s1[FN], s2[FN];
#pragma unroll
    for (int jn = 0; jn < FN; ++jn) { s1[jn] = 0.f; s2[jn] = 0.f; }

#pragma unroll
    for (int im = 0; im < FM; ++im) {
        // row bases of this fragment's 16 rows
        size_t obase[16];
        bool rowok[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int m = m0 + row;
            rowok[r] = m < a.M;
            const int mc = rowok[r] ? m : 0;
            if (KIND == KIND_F) {
                obase[r] = (size_t)mc * a.Nn;
            } else {
                int n, i, j;
                decode_pos(mc, d.HS, d.WS, a.lhs, a.lws, n, i, j);
                obase[r] = ((size_t)(n * d.HB + S * i + py) * d.WB + (S * j + px)) * a.Nn;
            }
        }
        if (!bwd) {
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!(rowok[r] && colok[jn])) continue;
                    const size_t off = obase[r] + colc[jn];
                    float v = acc[im][jn][r] + c_a[jn];
                    if (a.ep.mul) v *= a.ep.mul[off];
                    if (a.ep.add) v += a.ep.add[off];
                    a.Out[off] = v;
                }
            }
        } else {
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
                // all 16 c_prev loads of this fragment are issued before the first one is consumed
                float cp[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = rowok[r] && colok[jn];
                    cp[r] = a.ep.cprev[ok ? (obase[r] + colc[jn]) : 0];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = rowok[r] && colok[jn];
                    const float c = cp[r];
                    const float bn = fmaf(c_a[jn], c, c_b[jn]);
                    const float v = acc[im][jn][r];
                    float dbn = bn > 0.f ? v : v * a.ep.ealpha;
                    dbn = ok ? dbn : 0.f;
                    if (ok) a.Out[obase[r] + colc[jn]] = dbn * c_a[jn];
                    s1[jn] += dbn;
                    s2[jn] = fmaf(dbn, c, s2[jn]);
                }
            }
        }
    }
    if (bwd) {
        // column sums: lane halves -> waves along M -> one partial row per block tile
        float* red = smem;  // [WGM][2][BN]
        __syncthreads();
#pragma unroll
        for (int jn = 0; jn < FN; ++jn) {
            float t1 = s1[jn] + __shfl_xor(s1[jn], 32);
            float t2 = s2[jn] + __shfl_xor(s2[jn], 32);
            if (lh == 0) {
                red[(wm * 2 + 0) * BN + wn * WTN + jn * 32 + l31] = t1;
                red[(wm * 2 + 1) * BN + wn * WTN + jn * 32 + l31] = t2;
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += red[(w * 2 + which) * BN + c];
            const int col = n0 + c;
            const size_t tile = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
            if (col < a.Nn) a.ep.colpart[(tile * 2 + which) * a.Nn + col] = t;
        }
    }
}

// bf16 hi|lo planes for the bf16x3 kernels: Wf16[plane][tap][cb/8][cs][8], Wd16[plane][tap][cs/8][cb][8] (ushort),
// each tensor at 2*off with its lo plane `count` elements behind the hi plane
__device__ __forceinline__ unsigned bf16_rne_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// Sums S split-K slabs (fixed order -> deterministic) and applies the epilogue.  Block = 64 rows x 64 columns:
// 16 column-quad lanes x 16 row lanes, 4 rows per thread.
__global__ void __launch_bounds__(256) splitk_epilogue_kernel(const float* __restrict__ slabs, int S, long long out_elems,
                                                              int rows, int Nn, UadEpilogue ep, float* __restrict__ out) {
    __shared__ float red[2][16][64];
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int col = blockIdx.y * 64 + cq * 4;
    const bool colok = col < Nn;
    const bool bwd = ep.kind == UAD_EPI_BWD_ACT;
    float4 ca = make_float4(0, 0, 0, 0), cb = ca;
    if (colok) {
        if (!bwd) { if (ep.bias) ca = *reinterpret_cast<const float4*>(ep.bias + col); }
        else {
            ca = *reinterpret_cast<const float4*>(ep.escale + col);
            ca.x *= ep.emult; ca.y *= ep.emult; ca.z *= ep.emult; ca.w *= ep.emult;
            cb = *reinterpret_cast<const float4*>(ep.eshift + col);
        }
    }
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int row = blockIdx.x * 64 + u * 16 + rl;
        if (row >= rows || !colok) continue;
        const size_t off = (size_t)row * Nn + col;
        float4 v = *reinterpret_cast<const float4*>(slabs + off);
        for (int s = 1; s < S; ++s) {
            const float4 t = *reinterpret_cast<const float4*>(slabs + (size_t)s * out_elems + off);
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if (!bwd) {
            v.x += ca.x; v.y += ca.y; v.z += ca.z; v.w += ca.w;
            if (ep.mul) { const float4 t = *reinterpret_cast<const float4*>(ep.mul + off); v.x *= t.x; v.y *= t.y; v.z *= t.z; v.w *= t.w; }
            if (ep.add) { const float4 t = *reinterpret_cast<const float4*>(ep.add + off); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
            *reinterpret_cast<float4*>(out + off) = v;
        } else {
            const float4 c = *reinterpret_cast<const float4*>(ep.cprev + off);
            const float vv[4] = {v.x, v.y, v.z, v.w}, cc[4] = {c.x, c.y, c.z, c.w};
            const float aa[4] = {ca.x, ca.y, ca.z, ca.w}, bb[4] = {cb.x, cb.y, cb.z, cb.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float bn = fmaf(aa[e], cc[e], bb[e]);
                const float dbn = bn > 0.f ? vv[e] : vv[e] * ep.ealpha;
                o[e] = dbn * aa[e];
                s1[e] += dbn;
                s2[e] = fmaf(dbn, cc[e], s2[e]);
            }
            *reinterpret_cast<float4*>(out + off) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (bwd) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[0][rl][cq * 4 + e] = s1[e]; red[1][rl][cq * 4 + e] = s2[e]; }
        __syncthreads();
        if (threadIdx.x < 128) {
            const int which = threadIdx.x >> 6, c = threadIdx.x & 63;
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) t += red[which][k][c];
            const int gc = blockIdx.y * 64 + c;
            if (gc < Nn) ep.colpart[((size_t)blockIdx.x * 2 + which) * Nn + gc] = t;
        }
    }
}

// Weight re-layout for the spatial kernels.  One thread per source element W[tap][cb][cs] of any of up to 8 tensors:
//   F-pack: Wp[tap][cb/4][cs][cb%4]     D-pack: Wq[tap][cs/4][cb][cs%4]      (both at the tensor's own flat offset)
struct PackDesc { long long off[16]; int cb[16], cs[16], count[16]; int n; };
__global__ void pack_weights_kernel(const float* __restrict__ W, float* __restrict__ Wf, float* __restrict__ Wd, PackDesc pd) {
    long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int t = 0;
    while (t < pd.n && gid >= pd.count[t]) { gid -= pd.count[t]; ++t; }
    if (t >= pd.n) return;
    const int CB = pd.cb[t], CS = pd.cs[t];
    const int cs = (int)(gid % CS);
    const int r = (int)(gid / CS);
    const int cb = r % CB, tap = r / CB;
    const float v = W[pd.off[t] + gid];
    Wf[pd.off[t] + ((size_t)(tap * (CB / 4) + cb / 4) * CS + cs) * 4 + (cb & 3)] = v;
    Wd[pd.off[t] + ((size_t)(tap * (CS / 4) + cs / 4) * CB + cb) * 4 + (cs & 3)] = v;
}

__global__ void pack_weights_bf16_kernel(const float* __restrict__ W, unsigned short* __restrict__ Wf, unsigned short* __restrict__ Wd, PackDesc pd) {
    long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int t = 0;
    while (t < pd.n && gid >= pd.count[t]) { gid -= pd.count[t]; ++t; }
    if (t >= pd.n) return;
    const int CB = pd.cb[t], CS = pd.cs[t];
    const int cs = (int)(gid % CS);
    const int r = (int)(gid / CS);
    const int cb = r % CB, tap = r / CB;
    const float v = W[pd.off[t] + gid];
    const unsigned hi = bf16_rne_bits(v);
    const unsigned lo = bf16_rne_bits(v - __uint_as_float(hi << 16));
    const size_t base = 2 * (size_t)pd.off[t], cnt = (size_t)pd.count[t];
    const size_t fi = ((size_t)(tap * (CB / 8) + cb / 8) * CS + cs) * 8 + (cb & 7);
    const size_t di = ((size_t)(tap * (CS / 8) + cs / 8) * CB + cb) * 8 + (cs & 7);
    Wf[base + fi] = (unsigned short)hi; Wf[base + cnt + fi] = (unsigned short)lo;
    Wd[base + di] = (unsigned short)hi; Wd[base + cnt + di] = (unsigned short)lo;
}

// Three planes (bf16x6, uad_convk16.inc): x = h + m + l; planes of a tensor at ushort index 4 * off + p * count in buffers of 4 * nparams ushorts
// (4, not 3: a tensor's first plane then starts 8 * off bytes in -- dword-aligned for the fragment loads whatever the offset's parity).
__global__ void pack_weights_bf16_3p_kernel(const float* __restrict__ W, unsigned short* __restrict__ Wf, unsigned short* __restrict__ Wd, PackDesc pd) {
    long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int t = 0;
    while (t < pd.n && gid >= pd.count[t]) { gid -= pd.count[t]; ++t; }
    if (t >= pd.n) return;
    const int CB = pd.cb[t], CS = pd.cs[t];
    const int cs = (int)(gid % CS);
    const int r = (int)(gid / CS);
    const int cb = r % CB, tap = r / CB;
    const float v = W[pd.off[t] + gid];
    const unsigned h = bf16_rne_bits(v);
    const float r1 = v - __uint_as_float(h << 16);
    const unsigned m = bf16_rne_bits(r1);
    const unsigned l = bf16_rne_bits(r1 - __uint_as_float(m << 16));
    const size_t base = 4 * (size_t)pd.off[t], cnt = (size_t)pd.count[t];
    const size_t fi = ((size_t)(tap * (CB / 8) + cb / 8) * CS + cs) * 8 + (cb & 7);
    const size_t di = ((size_t)(tap * (CS / 8) + cs / 8) * CB + cb) * 8 + (cs & 7);
    Wf[base + fi] = (unsigned short)h; Wf[base + cnt + fi] = (unsigned short)m; Wf[base + 2 * cnt + fi] = (unsigned short)l;
    Wd[base + di] = (unsigned short)h; Wd[base + cnt + di] = (unsigned short)m; Wd[base + 2 * cnt + di] = (unsigned short)l;
}

// The same packing, one 16-byte group of a packed layout per thread (blockIdx.y: 0 = the F layout, 8 consecutive cb of one (tap, cs); 1 = the D
// layout, 8 consecutive cs of one (tap, cb)): coalesced 16-byte stores instead of four scattered 2-byte stores per element (the repack runs on the
// side stream behind the optimizer step; at 20 us it outlasted the main-stream work before the first packed-weight consumer).  Same bits.
// A tensor's offset in the flat parameter vector need not be a multiple of four floats (the ResNet graph's critic starts one float after the generator's
// one-channel 1x1 convolution: every critic tensor sat at offset 1 mod 4 and took the per-element kernels -- 133 + 81 us per phase in the round-6 trace):
// the 16-byte accesses are typed dword-aligned, which the hardware serves at any dword address.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u4u __attribute__((ext_vector_type(4), aligned(4)));
template <int NPL>      // 2: hi | lo planes at ushort index 2 * off (bf16x3); 3: h | m | l at 4 * off (bf16x6; round 6 -- the per-element 3p kernel was 4.5 % of a configs[3] iteration)
__global__ void __launch_bounds__(256) pack_weights_bf16_v8_kernel(const float* __restrict__ W, unsigned short* __restrict__ Wf, unsigned short* __restrict__ Wd, PackDesc pd) {
    long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // group index inside the tensor list
    int t = 0;
    while (t < pd.n && g >= pd.count[t] / 8) { g -= pd.count[t] / 8; ++t; }
    if (t >= pd.n) return;
    const int CB = pd.cb[t], CS = pd.cs[t];
    const float* w = W + pd.off[t];
    float v[8];
    size_t dst;      // first element of the group inside the tensor's packed plane
    if (blockIdx.y == 0) {
        const int cs = (int)(g % CS);
        const int r = (int)(g / CS);
        const int cb8 = r % (CB / 8), tap = r / (CB / 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = w[((size_t)tap * CB + cb8 * 8 + e) * CS + cs];
        dst = ((size_t)(tap * (CB / 8) + cb8) * CS + cs) * 8;
    } else {
        const int cb = (int)(g % CB);
        const int r = (int)(g / CB);
        const int cs8 = r % (CS / 8), tap = r / (CS / 8);
        const f4u a = *reinterpret_cast<const f4u*>(w + ((size_t)tap * CB + cb) * CS + cs8 * 8);
        const f4u b = *reinterpret_cast<const f4u*>(w + ((size_t)tap * CB + cb) * CS + cs8 * 8 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        dst = ((size_t)(tap * (CS / 8) + cs8) * CB + cb) * 8;
    }
    unsigned pl[NPL][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float r = v[e];
#pragma unroll
        for (int q = 0; q < NPL; ++q) {      // same arithmetic as the per-element kernels: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)
            pl[q][e] = bf16_rne_bits(r);
            r -= __uint_as_float(pl[q][e] << 16);
        }
    }
    unsigned short* out = blockIdx.y == 0 ? Wf : Wd;
    const size_t base = (NPL == 3 ? 4 : 2) * (size_t)pd.off[t], cnt = (size_t)pd.count[t];
#pragma unroll
    for (int q = 0; q < NPL; ++q)
        *reinterpret_cast<u4u*>(out + base + q * cnt + dst) = u4u{pl[q][0] | (pl[q][1] << 16), pl[q][2] | (pl[q][3] << 16), pl[q][4] | (pl[q][5] << 16), pl[q][6] | (pl[q][7] << 16)};
}

// ------------------------------------------------------------------------------------------------
// W-type: filter gradient.  GEMM M = (tap, cb) flattened, N = cs, K = positions (split over blockIdx.z).
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int BK, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) conv_w_kernel(const ConvWArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int FM = WTM / 32, FN = WTN / 32;
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int A_EL = BK * LDA, B_EL = BK * LDB, STAGE = A_EL + B_EL;
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const UadConvDesc& d = a.d;
    const int kbeg = blockIdx.z * a.kper;
    const int kend = min(kbeg + a.kper, a.Kt);
    const int nk = (kend - kbeg + BK - 1) / BK;

    constexpr int TPRA = BM / 4, RPA = NT / TPRA, PA = (BK + RPA - 1) / RPA;
    const int acol = (tid % TPRA) * 4, arow0 = tid / TPRA;
    const int mcol = m0 + acol;
    const bool acolok = mcol < a.Mtot;
    const int tapA = acolok ? mcol / d.CB : 0;
    const int cbA = acolok ? mcol - tapA * d.CB : 0;
    const int kyA = tapA / d.KS, kxA = tapA - kyA * d.KS;
    float4 scA = make_float4(1, 1, 1, 1), shA = make_float4(0, 0, 0, 0);
    const bool xfa = a.xfb.scale != nullptr;
    if (xfa && acolok) {
        scA = *reinterpret_cast<const float4*>(a.xfb.scale + cbA);
        shA = *reinterpret_cast<const float4*>(a.xfb.shift + cbA);
        scA.x *= a.xfb.mult; scA.y *= a.xfb.mult; scA.z *= a.xfb.mult; scA.w *= a.xfb.mult;
    }
    constexpr int TPRB = BN / 4, RPB = NT / TPRB, PB = (BK + RPB - 1) / RPB;
    const int bcol = (tid % TPRB) * 4, brow0 = tid / TPRB;
    const int ncol = n0 + bcol;
    const bool bcolok = ncol < d.CS;
    float4 scB = make_float4(1, 1, 1, 1), shB = make_float4(0, 0, 0, 0);
    const bool xfs = a.xfs.scale != nullptr;
    if (xfs && bcolok) {
        scB = *reinterpret_cast<const float4*>(a.xfs.scale + ncol);
        shB = *reinterpret_cast<const float4*>(a.xfs.shift + ncol);
        scB.x *= a.xfs.mult; scB.y *= a.xfs.mult; scB.z *= a.xfs.mult; scB.w *= a.xfs.mult;
    }

    float4 va[PA], vb[PB];
    unsigned okA = 0, okB = 0;
    auto load_tiles = [&](int kpos) {
        okA = 0; okB = 0;
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int r = arow0 + q * RPA;
            const int pos = kpos + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < BK && pos < kend && acolok) {
                int n, i, j;
                decode_pos(pos, d.HS, d.WS, a.lhs, a.lws, n, i, j);
                const int y = d.S * i - d.P + kyA, x = d.S * j - d.P + kxA;
                if ((unsigned)y < (unsigned)d.HB && (unsigned)x < (unsigned)d.WB) {
                    v = *reinterpret_cast<const float4*>(a.big + ((size_t)(n * d.HB + y) * d.WB + x) * d.CB + cbA);
                    okA |= 1u << q;
                }
            }
            va[q] = v;
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
            const int r = brow0 + q * RPB;
            const int pos = kpos + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < BK && pos < kend && bcolok) {
                v = *reinterpret_cast<const float4*>(a.small_ + (size_t)pos * d.CS + ncol);
                okB |= 1u << q;
            }
            vb[q] = v;
        }
    };
    auto store_tiles = [&](int buf) {
        float* sA = smem + buf * STAGE;
        float* sB = sA + A_EL;
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int r = arow0 + q * RPA;
            float4 v = va[q];
            if (xfa && ((okA >> q) & 1u)) v = xform4(v, scA, shA, a.xfb.alpha);
            if (r < BK) *reinterpret_cast<float4*>(sA + r * LDA + acol) = v;
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
            const int r = brow0 + q * RPB;
            float4 v = vb[q];
            if (xfs && ((okB >> q) & 1u)) v = xform4(v, scB, shB, a.xfs.alpha);
            if (r < BK) *reinterpret_cast<float4*>(sB + r * LDB + bcol) = v;
        }
    };

    v16f acc[FM][FN];
#pragma unroll
    for (int im = 0; im < FM; ++im)
#pragma unroll
        for (int jn = 0; jn < FN; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[im][jn][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;
    if (nk > 0) {
        load_tiles(kbeg);
        store_tiles(0);
    }
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < nk;
        if (more) load_tiles(kbeg + (ks + 1) * BK);
        const float* sA = smem + buf * STAGE;
        const float* sB = sA + A_EL;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = kk * 8 + 4 * lh + s;
                float av[FM], bv[FN];
#pragma unroll
                for (int im = 0; im < FM; ++im) av[im] = sA[k * LDA + wm * WTM + im * 32 + l31];
#pragma unroll
                for (int jn = 0; jn < FN; ++jn) bv[jn] = sB[k * LDB + wn * WTN + jn * 32 + l31];
#pragma unroll
                for (int im = 0; im < FM; ++im)
#pragma unroll
                    for (int jn = 0; jn < FN; ++jn)
                        acc[im][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[im], bv[jn], acc[im][jn], 0, 0, 0);
            }
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
    }

    float* out = a.partial + (size_t)blockIdx.z * a.Mtot * d.CS;
#pragma unroll
    for (int im = 0; im < FM; ++im)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m >= a.Mtot) continue;
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
                const int col = n0 + wn * WTN + jn * 32 + l31;
                if (col < d.CS) out[(size_t)m * d.CS + col] = acc[im][jn][r];
            }
        }
}


// ---- generic filter gradient in bf16x3 math (UAD_MATH_BF16X3_ALL): both operands arrive position-major ([k = position][channels]) and the
// matrix cores want channel-major rows with K contiguous, so each thread owns PAIRS of adjacent positions and stores (k, k+1) as one
// 32-bit word per channel into the hi | lo bf16 planes; a K = 16 slice is three v_mfma_f32_32x32x16_bf16.  Identity activation-on-load only.
template <int BM, int BN, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) conv_w16_kernel(const ConvWArgs a) {
    constexpr int BK = 32, NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int FM = WTM / 32, FN = WTN / 32;
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
    constexpr int LDK = BK + 8;
    constexpr int A_EL = BM * LDK, B_EL = BN * LDK, STAGE = 2 * A_EL + 2 * B_EL;     // A hi | A lo | B hi | B lo
    __shared__ __attribute__((aligned(16))) unsigned short smem16[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const UadConvDesc& d = a.d;
    const int kbeg = blockIdx.z * a.kper;
    const int kend = min(kbeg + a.kper, a.Kt);
    const int nk = (kend - kbeg + BK - 1) / BK;

    constexpr int TPRA = BM / 4, RPA = NT / TPRA, PA = BK / RPA;
    constexpr int TPRB = BN / 4, RPB = NT / TPRB, PB = BK / RPB;
    static_assert(PA % 2 == 0 && PB % 2 == 0 && PA * RPA == BK && PB * RPB == BK, "each thread owns pairs of adjacent positions");
    const int acol = (tid % TPRA) * 4, arow0 = tid / TPRA;
    const int bcol = (tid % TPRB) * 4, brow0 = tid / TPRB;
    auto arow = [&](int q) { return 2 * arow0 + (q & 1) + 2 * RPA * (q >> 1); };
    auto brow = [&](int q) { return 2 * brow0 + (q & 1) + 2 * RPB * (q >> 1); };
    const int mcol = m0 + acol;
    const bool acolok = mcol < a.Mtot;
    const int tapA = acolok ? mcol / d.CB : 0;
    const int cbA = acolok ? mcol - tapA * d.CB : 0;
    const int kyA = tapA / d.KS, kxA = tapA - kyA * d.KS;
    const int ncol = n0 + bcol;
    const bool bcolok = ncol < d.CS;

    float4 va[PA], vb[PB];
    auto load_tiles = [&](int kpos) {
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            const int pos = kpos + arow(q);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos < kend && acolok) {
                int n, i, j;
                decode_pos(pos, d.HS, d.WS, a.lhs, a.lws, n, i, j);
                const int y = d.S * i - d.P + kyA, x = d.S * j - d.P + kxA;
                if ((unsigned)y < (unsigned)d.HB && (unsigned)x < (unsigned)d.WB)
                    v = *reinterpret_cast<const float4*>(a.big + ((size_t)(n * d.HB + y) * d.WB + x) * d.CB + cbA);
            }
            va[q] = v;
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
            const int pos = kpos + brow(q);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos < kend && bcolok) v = *reinterpret_cast<const float4*>(a.small_ + (size_t)pos * d.CS + ncol);
            vb[q] = v;
        }
    };
    // (k, k+1) of four channels -> four 32-bit words per plane
    auto store_pair = [&](unsigned short* ph, unsigned short* pl, int col, int k, const float4 v0, const float4 v1) {
        uint2 h0, l0, h1, l1;
        split_bf16(v0, h0, l0);
        split_bf16(v1, h1, l1);
        const unsigned hh0[4] = {h0.x & 0xFFFFu, h0.x >> 16, h0.y & 0xFFFFu, h0.y >> 16};
        const unsigned hh1[4] = {h1.x & 0xFFFFu, h1.x >> 16, h1.y & 0xFFFFu, h1.y >> 16};
        const unsigned ll0[4] = {l0.x & 0xFFFFu, l0.x >> 16, l0.y & 0xFFFFu, l0.y >> 16};
        const unsigned ll1[4] = {l1.x & 0xFFFFu, l1.x >> 16, l1.y & 0xFFFFu, l1.y >> 16};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<unsigned*>(ph + (col + i) * LDK + k) = hh0[i] | (hh1[i] << 16);
            *reinterpret_cast<unsigned*>(pl + (col + i) * LDK + k) = ll0[i] | (ll1[i] << 16);
        }
    };
    auto store_tiles = [&](int buf) {
        unsigned short* sAh = smem16 + buf * STAGE;
        unsigned short* sAl = sAh + A_EL;
        unsigned short* sBh = sAl + A_EL;
        unsigned short* sBl = sBh + B_EL;
#pragma unroll
        for (int q = 0; q < PA; q += 2) store_pair(sAh, sAl, acol, arow(q), va[q], va[q + 1]);
#pragma unroll
        for (int q = 0; q < PB; q += 2) store_pair(sBh, sBl, bcol, brow(q), vb[q], vb[q + 1]);
    };

    v16f acc[FM][FN];
#pragma unroll
    for (int im = 0; im < FM; ++im)
#pragma unroll
        for (int jn = 0; jn < FN; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[im][jn][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;
    if (nk > 0) {
        load_tiles(kbeg);
        store_tiles(0);
    }
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        const bool more = ks + 1 < nk;
        if (more) load_tiles(kbeg + (ks + 1) * BK);
        const unsigned short* sAh = smem16 + buf * STAGE;
        const unsigned short* sAl = sAh + A_EL;
        const unsigned short* sBh = sAl + A_EL;
        const unsigned short* sBl = sBh + B_EL;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            uint4 ah[FM], al[FM], bh[FN], bl[FN];
#pragma unroll
            for (int im = 0; im < FM; ++im) {
                const int o = (wm * WTM + im * 32 + l31) * LDK + kk * 16 + 8 * lh;
                ah[im] = *reinterpret_cast<const uint4*>(sAh + o);
                al[im] = *reinterpret_cast<const uint4*>(sAl + o);
            }
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
                const int o = (wn * WTN + jn * 32 + l31) * LDK + kk * 16 + 8 * lh;
                bh[jn] = *reinterpret_cast<const uint4*>(sBh + o);
                bl[jn] = *reinterpret_cast<const uint4*>(sBl + o);
            }
#pragma unroll
            for (int im = 0; im < FM; ++im)
#pragma unroll
                for (int jn = 0; jn < FN; ++jn) {
                    acc[im][jn] = mfma_bf16(ah[im], bh[jn], acc[im][jn]);
                    acc[im][jn] = mfma_bf16(ah[im], bl[jn], acc[im][jn]);
                    acc[im][jn] = mfma_bf16(al[im], bh[jn], acc[im][jn]);
                }
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
    }

    float* out = a.partial + (size_t)blockIdx.z * a.Mtot * d.CS;
#pragma unroll
    for (int im = 0; im < FM; ++im)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m >= a.Mtot) continue;
#pragma unroll
            for (int jn = 0; jn < FN; ++jn) {
                const int col = n0 + wn * WTN + jn * 32 + l31;
                if (col < d.CS) out[(size_t)m * d.CS + col] = acc[im][jn][r];
            }
        }
}

template <int KIND>
void launch_gemm(const ConvGemmArgs& a, int classes, hipStream_t st) {
    const TileChoice t = choose_tile(a.M, a.Nn, a.CA, classes);
    dim3 grid((a.M + t.BM - 1) / t.BM, (a.Nn + t.BN - 1) / t.BN, classes * a.nsplit);
    if (a.math16 && !a.xf.scale && t.BK == 32 && t.BN == 64 && !getenv("UAD_NO_G16")) {
        if (t.BM == 128) { hipLaunchKernelGGL((conv_gemm16_kernel<128, 64, 32, 2, 2, KIND>), grid, dim3(256), 0, st, a); return; }
        if (t.BM == 64) { hipLaunchKernelGGL((conv_gemm16_kernel<64, 64, 32, 2, 2, KIND>), grid, dim3(256), 0, st, a); return; }
    }
#define UAD_GEMM_CASE(bm, bn, bk, wgm, wgn)                                                              \
    if (t.BM == bm && t.BN == bn && t.BK == bk) {                                                        \
        hipLaunchKernelGGL((conv_gemm_kernel<bm, bn, bk, wgm, wgn, KIND>), grid, dim3(64 * wgm * wgn), 0, st, a); \
        return;                                                                                          \
    }
    UAD_GEMM_CASE(128, 64, 32, 2, 2)
    UAD_GEMM_CASE(128, 32, 32, 4, 1)
    UAD_GEMM_CASE(64, 64, 32, 2, 2)
    UAD_GEMM_CASE(64, 32, 32, 2, 1)
    UAD_GEMM_CASE(64, 64, 16, 2, 2)
    UAD_GEMM_CASE(64, 32, 16, 2, 1)
    UAD_GEMM_CASE(64, 64, 8, 2, 2)
    UAD_GEMM_CASE(64, 32, 8, 2, 1)
#undef UAD_GEMM_CASE
}

}  // namespace
void uad_gemm_launch(const ConvGemmArgs& a, bool f_type, int classes, hipStream_t st) {
    if (f_type) launch_gemm<KIND_F>(a, classes, st); else launch_gemm<KIND_D>(a, classes, st);
}

void uad_gemm_launch_splitk_epilogue(const float* slabs, int nsplit, long long out_elems, int rows, int Nn, const UadEpilogue& ep, float* out, hipStream_t st) {
    dim3 grid((rows + 63) / 64, (Nn + 63) / 64);
    hipLaunchKernelGGL(splitk_epilogue_kernel, grid, dim3(256), 0, st, slabs, nsplit, out_elems, rows, Nn, ep, out);
}

void uad_gemm_launch_w(const ConvWArgs& a, dim3 grid, int BM, int BN, bool w16, hipStream_t st) {
    if (w16 && BM == 128)
        hipLaunchKernelGGL((conv_w16_kernel<128, 64, 2, 2>), grid, dim3(256), 0, st, a);
    else if (w16 && BM == 64)
        hipLaunchKernelGGL((conv_w16_kernel<64, 64, 2, 2>), grid, dim3(256), 0, st, a);
    else if (BM == 128 && BN == 64)
        hipLaunchKernelGGL((conv_w_kernel<128, 64, 32, 2, 2>), grid, dim3(256), 0, st, a);
    else if (BM == 128 && BN == 32)
        hipLaunchKernelGGL((conv_w_kernel<128, 32, 32, 4, 1>), grid, dim3(256), 0, st, a);
    else if (BM == 64 && BN == 64)
        hipLaunchKernelGGL((conv_w_kernel<64, 64, 32, 2, 2>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((conv_w_kernel<64, 32, 32, 2, 1>), grid, dim3(128), 0, st, a);
}

void uad_launch_pack_weights(const float* params, float* wpack_f, float* wpack_d, const long long* offs, const int* cbs,
                             const int* css, const int* taps, int n, hipStream_t st) {
    PackDesc pd;
    long long total = 0;
    pd.n = n;
    for (int i = 0; i < n; ++i) {
        pd.off[i] = offs[i]; pd.cb[i] = cbs[i]; pd.cs[i] = css[i]; pd.count[i] = taps[i] * cbs[i] * css[i];
        total += pd.count[i];
    }
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, params, wpack_f, wpack_d, pd);
}

void uad_launch_pack_weights_bf16_3p(const float* params, unsigned short* w3_f, unsigned short* w3_d, const long long* offs,
                                     const int* cbs, const int* css, const int* taps, int n, hipStream_t st) {
    PackDesc pd;
    pd.n = n;
    long long total = 0;
    for (int i = 0; i < n; ++i) { pd.off[i] = offs[i]; pd.cb[i] = cbs[i]; pd.cs[i] = css[i]; pd.count[i] = taps[i] * cbs[i] * css[i]; total += pd.count[i]; }
    bool v8 = ((((uintptr_t)params | (uintptr_t)w3_f | (uintptr_t)w3_d) & 15) == 0);
    for (int i = 0; i < n; ++i) v8 = v8 && pd.count[i] % 8 == 0 && pd.cb[i] % 8 == 0 && pd.cs[i] % 8 == 0;      // whole 8-element groups (any dword-aligned offset: f4u / u4u)
    if (v8) hipLaunchKernelGGL(pack_weights_bf16_v8_kernel<3>, dim3((unsigned)((total / 8 + 255) / 256), 2), dim3(256), 0, st, params, w3_f, w3_d, pd);
    else hipLaunchKernelGGL(pack_weights_bf16_3p_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, params, w3_f, w3_d, pd);
}

void uad_launch_pack_weights_bf16(const float* params, unsigned short* w16_f, unsigned short* w16_d, const long long* offs,
                                  const int* cbs, const int* css, const int* taps, int n, hipStream_t st) {
    PackDesc pd;
    long long total = 0;
    pd.n = n;
    for (int i = 0; i < n; ++i) {
        pd.off[i] = offs[i]; pd.cb[i] = cbs[i]; pd.cs[i] = css[i]; pd.count[i] = taps[i] * cbs[i] * css[i];
        total += pd.count[i];
    }
    bool v8 = ((((uintptr_t)params | (uintptr_t)w16_f | (uintptr_t)w16_d) & 15) == 0);
    for (int i = 0; i < n; ++i) v8 = v8 && pd.cb[i] % 8 == 0 && pd.cs[i] % 8 == 0;      // (any dword-aligned offset: f4u / u4u)
    if (v8) hipLaunchKernelGGL(pack_weights_bf16_v8_kernel<2>, dim3((unsigned)((total / 8 + 255) / 256), 2), dim3(256), 0, st, params, w16_f, w16_d, pd);
    else hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, params, w16_f, w16_d, pd);
}
