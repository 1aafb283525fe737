// k5 s2 D kind ("scatter" by output-parity class) outside the lane = pixel family: conv5_d16_kernel (class-sequential, bf16x3: the lane = pixel kernels' fallback),
// conv5_bf16_kernel (channel chunks streamed through LDS, bf16x3) and conv5_d_kernel (exact fp32, incl. the fused final epilogue).  uad_conv_plan.hip decides
// the instance and calls the uad_conv5_d*_launch functions below.
#include "uad_gemm_common.h"

namespace {

// halo (TH+2)x(TW+2), four output-parity classes (the F form of this kernel was superseded by conv5_f16_kernel)
template <int TH, int TW, int CK, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) conv5_bf16_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = TH + 2, IW = TW + 2;
    constexpr int LDH = CK + 8;                 // ushorts per pixel row (+16 B pad: odd number of 16-B slots)
    constexpr int NKS = CK / 16, CQ = CK / 4;
    constexpr int BN = 32 * WGN;
    constexpr int NACC = 8;
    static_assert(TH * TW == 32 * WGM, "one 32-row fragment per wave along M");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* sHi = reinterpret_cast<unsigned short*>(dsm);
    unsigned short* sLo = sHi + IH * IW * LDH;
    float* s_xf = reinterpret_cast<float*>(sLo + IH * IW * LDH);
    float* s_red = s_xf + 2 * XF_LDS_CH;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int tilesx = d.WS / TW;
    const int ty0 = (blockIdx.x / tilesx) * TH, tx0 = (blockIdx.x % tilesx) * TW;
    const int n = blockIdx.y;
    const int nsplit = a.nsplit;
    const int n0 = (blockIdx.z / nsplit) * BN;
    const int split = blockIdx.z % nsplit;
    const int CA = a.CA, Nn = a.Nn;   // contraction / output channels
    const int AH = d.HS, AW = d.WS;

    const bool xf = a.xf.scale != nullptr;
    if (xf)
        for (int c = tid; c < CA; c += NT) {
            s_xf[c] = a.xf.scale[c] * a.xf.mult;
            s_xf[XF_LDS_CH + c] = a.xf.shift[c];
        }

    const int m = wm * 32 + l31;
    const int pty = m / TW, ptx = m % TW;
    const int aoff = ((pty + 1) * IW + ptx + 1) * LDH + 8 * lh;
    const int col = n0 + wn * 32 + l31;
    const bool colok = col < Nn;
    const int colc = colok ? col : 0;
    // packed planes [tap][k/8][n][8] bf16: one uint4 per (k-octet, n)
    const uint4* wq = reinterpret_cast<const uint4*>(a.Wp16) + (size_t)lh * Nn + colc;
    const size_t plane_q = (size_t)a.w16_plane / 8;

    BFrag16<NKS> b0, b1;
    auto loadB = [&](BFrag16<NKS>& b, int tap, int c0) {
        const uint4* w = wq + ((size_t)tap * (CA / 8) + c0 / 8) * Nn;
#pragma unroll
        for (int j = 0; j < NKS; ++j) {
            b.hi[j] = w[(size_t)(2 * j) * Nn];
            b.lo[j] = w[(size_t)(2 * j) * Nn + plane_q];
        }
    };

    v16f acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    const int cper = (CA / CK + nsplit - 1) / nsplit;
    const int ch0 = split * cper;
    const int nchunks = min(CA / CK, ch0 + cper);
    const int gy0 = ty0 - 1, gx0 = tx0 - 1;
    const float* inb = a.A + (size_t)n * AH * AW * CA;
    loadB(b0, 0, ch0 * CK);
    __syncthreads();

    for (int ch = ch0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        if (ch > ch0) __syncthreads();
        constexpr int TOT = IH * IW * CQ;
        constexpr int BATCH = 4;
        for (int f0 = tid; f0 < TOT; f0 += NT * BATCH) {
            float4 v[BATCH];
            bool ok[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                const int pix = f / CQ, cq = f % CQ;
                const int iy = pix / IW, ix = pix % IW;
                const int gy = gy0 + iy, gx = gx0 + ix;
                ok[u] = (f < TOT) && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
                const int gp = ok[u] ? (gy * AW + gx) : 0;
                v[u] = *reinterpret_cast<const float4*>(inb + (size_t)gp * CA + c0 + (ok[u] ? cq * 4 : 0));
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                if (f >= TOT) continue;
                const int pix = f / CQ, cq = f % CQ;
                float4 t = v[u];
                if (xf) {
                    const float4 sc = *reinterpret_cast<const float4*>(s_xf + c0 + cq * 4);
                    const float4 sh = *reinterpret_cast<const float4*>(s_xf + XF_LDS_CH + c0 + cq * 4);
                    t = xform4(t, sc, sh, a.xf.alpha);
                }
                t = keep4(ok[u], t);
                uint2 hi, lo;
                split_bf16(t, hi, lo);
                *reinterpret_cast<uint2*>(sHi + pix * LDH + cq * 4) = hi;
                *reinterpret_cast<uint2*>(sLo + pix * LDH + cq * 4) = lo;
            }
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 25; ++tap) {
            const int ky = tap / 5, kx = tap % 5;
            const int py = (ky + 1) & 1, px = (kx + 1) & 1;
            const int dy = (py + 1 - ky) / 2, dx = (px + 1 - kx) / 2;
            const int toff = (dy * IW + dx) * LDH;
            const int cls = py * 2 + px;
            BFrag16<NKS>& cur = (tap & 1) ? b1 : b0;
            BFrag16<NKS>& nxt = (tap & 1) ? b0 : b1;
            if (tap < 24) loadB(nxt, tap + 1, c0);
            else if (ch + 1 < nchunks) loadB(nxt, 0, c0 + CK);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NKS; ++j) {
                const uint4 ah = *reinterpret_cast<const uint4*>(sHi + aoff + toff + 16 * j);
                const uint4 al = *reinterpret_cast<const uint4*>(sLo + aoff + toff + 16 * j);
                acc[2 * cls] = mfma_bf16(ah, cur.hi[j], acc[2 * cls]);
                acc[2 * cls + 1] = mfma_bf16(ah, cur.lo[j], acc[2 * cls + 1]);
                acc[2 * cls + 1] = mfma_bf16(al, cur.hi[j], acc[2 * cls + 1]);
            }
        }
        b0 = b1;
    }

    // ---- epilogue (identical to the fp32 spatial kernels: the C layout of the MFMA is dtype independent) ----
    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    float c_a, c_b = 0.f;
    if (!bwd) c_a = a.ep.bias ? a.ep.bias[colc] : 0.f;
    else { c_a = a.ep.escale[colc] * a.ep.emult; c_b = a.ep.eshift[colc]; }
    float s1 = 0.f, s2 = 0.f;
    constexpr int NCLS = 4;
#pragma unroll
    for (int cls = 0; cls < NCLS; ++cls) {
        v16f o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = acc[2 * cls][r] + acc[2 * cls + 1][r];
        size_t obase[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int Y = 2 * (ty0 + mm / TW) + (cls >> 1), X = 2 * (tx0 + mm % TW) + (cls & 1);
            obase[r] = ((size_t)(n * d.HB + Y) * d.WB + X) * Nn;
        }
        if (nsplit > 1) {
            float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (colok) slab[obase[r] + colc] = o[r];
        } else {
            epilogue_frag<0>(a, o, obase, colok, colc, c_a, c_b, s1, s2);
        }
    }
    if (nsplit > 1) return;
    if (bwd) {
        const float t1 = s1 + __shfl_xor(s1, 32), t2 = s2 + __shfl_xor(s2, 32);
        if (lh == 0) {
            s_red[(wm * 2 + 0) * BN + wn * 32 + l31] = t1;
            s_red[(wm * 2 + 1) * BN + wn * 32 + l31] = t2;
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += s_red[(w * 2 + which) * BN + c];
            const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            if (n0 + c < Nn) a.ep.colpart[(tile * 2 + which) * Nn + n0 + c] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// D-kind, class-sequential form (bf16x3).  Every tap of a k5 s2 transposed contraction feeds exactly ONE of the four
// output-parity classes, so the classes share no operand: the workgroup stages its WHOLE channel range (CST channels of the
// (TH+2)x(TW+2) halo) once, then walks the classes one after the other -- 3 accumulator fragments live instead of 8
// (340 -> ~150 registers: two-three waves per SIMD instead of one), and each class's epilogue stores overlap the next
// class's MFMAs.  Requires CA == CST * nsplit.
// ------------------------------------------------------------------------------------------------

template <int TH, int TW, int CST, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) __attribute__((amdgpu_waves_per_eu(2))) conv5_d16_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = TH + 2, IW = TW + 2;
    constexpr int LDH = CST + 8;                // ushorts per pixel row (+16 B pad)
    constexpr int NCH = CST / 32, CQ = CST / 4;
    constexpr int BN = 32 * WGN;
    static_assert(TH * TW == 32 * WGM, "one 32-row fragment per wave along M");
    static_assert(CST % 32 == 0, "32-channel weight-fragment units");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* sHi = reinterpret_cast<unsigned short*>(dsm);
    unsigned short* sLo = sHi + IH * IW * LDH;
    float* s_xf = reinterpret_cast<float*>(sLo + IH * IW * LDH);
    float* s_red = s_xf + 2 * XF_LDS_CH;
    float* s_epi = s_red + WGM * 2 * BN;        // per-wave 32 x EPI_LD transpose tile of the epilogue
    float* s_fx = s_epi + WGM * WGN * 32 * 36;  // EPI_FINAL: target / reconstruction / L1 tiles of the 2TH x 2TW output block
    float* s_fo = s_fx + 4 * TH * TW;
    float* s_fl = s_fo + 4 * TH * TW;
    unsigned* s_fb = reinterpret_cast<unsigned*>(s_fl + 4 * TH * TW);   // EPI_FINAL + fin_bits: pattern word / d objective / d x_hat per pixel
    float* s_fg = reinterpret_cast<float*>(s_fb + 4 * TH * TW);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int tilesx = d.WS / TW;
    const int ty0 = (blockIdx.x / tilesx) * TH, tx0 = (blockIdx.x % tilesx) * TW;
    const int n = blockIdx.y;
    const int nsplit = a.nsplit;
    const int n0 = (blockIdx.z / nsplit) * BN;
    const int split = blockIdx.z % nsplit;
    const int CA = a.CA, Nn = a.Nn;
    const int cbase = split * CST;
    const int AH = d.HS, AW = d.WS;

    const bool xf = a.xf.scale != nullptr;
    if (xf)
        for (int c = tid; c < CST; c += NT) {
            s_xf[c] = a.xf.scale[cbase + c] * a.xf.mult;
            s_xf[XF_LDS_CH + c] = a.xf.shift[cbase + c];
        }

    if (a.ep.kind == UAD_EPI_FINAL)
        for (int idx = tid; idx < 4 * TH * TW; idx += NT) {
            const int yl = idx / (2 * TW), xl = idx % (2 * TW);
            s_fx[idx] = a.ep.fin_x[((size_t)n * d.HB + 2 * ty0 + yl) * d.WB + 2 * tx0 + xl];
        }

    const int m = wm * 32 + l31;
    const int pty = m / TW, ptx = m % TW;
    const int aoff = ((pty + 1) * IW + ptx + 1) * LDH + 8 * lh;
    const int col = n0 + wn * 32 + l31;
    const bool colok = col < Nn;
    const int colc = colok ? col : 0;
    const size_t plane_q = (size_t)a.w16_plane / 8;

    // Weight fragments: global -> VGPR ring of four, three units (one unit = one tap x 32 channels) ahead of their use: the
    // loads are L2 hits (a layer's planes exceed the 32 KB L1), ~500+ cycles against 192 cycles of MFMA work per unit.
    // (Sharing them through LDS was measured slower: it doubles the LDS read traffic, which then bounds the loop.)
    // Activation fragments: LDS -> VGPR, double-buffered one unit ahead, so the MFMAs of a unit never wait for LDS.
    constexpr int NUNIT = 25 * NCH;
    const uint4* wq = reinterpret_cast<const uint4*>(a.Wp16) + (size_t)lh * Nn + colc;
    BFrag16<2> b0, b1, b2, b3;
    // wave-uniform base (SGPR pair, scalar arithmetic) + one 32-bit per-lane offset: no 64-bit VALU add per load
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.Wp16), 0, 0xffffffff, 0x00020000);
    const unsigned lb = (unsigned)(lh * Nn + colc) * 16u;      // byte offsets, 32 bits: the packed weights of a layer are < 4 GB
    const unsigned plane_b = (unsigned)plane_q * 16u;
    auto loadB = [&](BFrag16<2>& b, int unit) __attribute__((always_inline)) {
        const int tap = kTapOrderD.tap[unit / NCH], c0 = cbase + (unit % NCH) * 32;
        const unsigned u = (unsigned)((tap * (CA / 8) + c0 / 8) * Nn) * 16u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            b.hi[j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u);
            b.lo[j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u + plane_b);
        }
    };
    auto loadA = [&](BFrag16<2>& f, int unit) __attribute__((always_inline)) {
        const int tap = kTapOrderD.tap[unit / NCH], kc = unit % NCH;
        const int ky = tap / 5, kx = tap % 5;
        const int py = (ky + 1) & 1, px = (kx + 1) & 1;
        const int dy = (py + 1 - ky) / 2, dx = (px + 1 - kx) / 2;
        const int toff = (dy * IW + dx) * LDH;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f.hi[j] = *reinterpret_cast<const uint4*>(sHi + aoff + toff + kc * 32 + 16 * j);
            f.lo[j] = *reinterpret_cast<const uint4*>(sLo + aoff + toff + kc * 32 + 16 * j);
        }
    };
    loadB(b0, 0);
    if (1 < NUNIT) loadB(b1, 1);
    if (2 < NUNIT) loadB(b2, 2);
    if (xf) __syncthreads();

    // ---- stage the whole halo tile of this workgroup's channel range: global fp32 -> activation -> bf16 hi|lo planes ----
    const int gy0 = ty0 - 1, gx0 = tx0 - 1;
    const float* inb = a.A + (size_t)n * AH * AW * CA + cbase;
    {
        constexpr int TOT = IH * IW * CQ;
        constexpr int BATCH = 4;
        for (int f0 = tid; f0 < TOT; f0 += NT * BATCH) {
            float4 v[BATCH];
            bool ok[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                const int pix = f / CQ, cq = f % CQ;
                const int iy = pix / IW, ix = pix % IW;
                const int gy = gy0 + iy, gx = gx0 + ix;
                ok[u] = (f < TOT) && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
                const int gp = ok[u] ? (gy * AW + gx) : 0;
                v[u] = *reinterpret_cast<const float4*>(inb + (size_t)gp * CA + (ok[u] ? cq * 4 : 0));
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                if (f >= TOT) continue;
                const int pix = f / CQ, cq = f % CQ;
                float4 t = v[u];
                if (xf) {
                    const float4 sc = *reinterpret_cast<const float4*>(s_xf + cq * 4);
                    const float4 sh = *reinterpret_cast<const float4*>(s_xf + XF_LDS_CH + cq * 4);
                    t = xform4(t, sc, sh, a.xf.alpha);
                }
                t = keep4(ok[u], t);
                uint2 hi, lo;
                split_bf16(t, hi, lo);
                *reinterpret_cast<uint2*>(sHi + pix * LDH + cq * 4) = hi;
                *reinterpret_cast<uint2*>(sLo + pix * LDH + cq * 4) = lo;
            }
        }
    }
    __syncthreads();

    // Epilogue: the 32x32 C fragment (lane = column) is transposed through a wave-private LDS tile so that every lane owns
    // 4 consecutive channels of 4 rows: 4 x 16-byte stores (and cprev loads) per class instead of 16 x 4-byte ones -- the
    // scattered dword form spent ~190 cycles per store instruction in the address path (3000 of 10000 cycles per class).
    constexpr int EPI_LD = 36;
    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    float* etile = s_epi + wave * 32 * EPI_LD;
    const int ec4 = (lane & 7) * 4, erow = lane >> 3;
    const int ecol = n0 + wn * 32 + ec4;                 // Nn % 32 == 0 on this path: always in range
    float4 e_a = make_float4(0.f, 0.f, 0.f, 0.f), e_b = e_a;
    if (!bwd) { if (a.ep.bias) e_a = *reinterpret_cast<const float4*>(a.ep.bias + ecol); }
    else {
        e_a = *reinterpret_cast<const float4*>(a.ep.escale + ecol);
        e_a.x *= a.ep.emult; e_a.y *= a.ep.emult; e_a.z *= a.ep.emult; e_a.w *= a.ep.emult;
        e_b = *reinterpret_cast<const float4*>(a.ep.eshift + ecol);
    }
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    // EPI_FINAL: e_a := conv bias, f_sc/f_sh := this layer's BN, f_w := final 1x1 kernel; per-lane running sums of the
    // final conv's kernel gradient (dwf), the loss (rec) and the final bias gradient (dbf)
    const bool fin = (a.ep.kind == UAD_EPI_FINAL);
    float4 f_sc = make_float4(0.f, 0.f, 0.f, 0.f), f_sh = f_sc, f_w = f_sc;
    float f_bf = 0.f, rec = 0.f, dbf = 0.f;
    float dwf[4] = {0.f, 0.f, 0.f, 0.f};
    if (fin) {
        f_sc = *reinterpret_cast<const float4*>(a.ep.escale + ecol);
        f_sc.x *= a.ep.emult; f_sc.y *= a.ep.emult; f_sc.z *= a.ep.emult; f_sc.w *= a.ep.emult;
        f_sh = *reinterpret_cast<const float4*>(a.ep.eshift + ecol);
        f_w = *reinterpret_cast<const float4*>(a.ep.fin_wf + ecol);
        f_bf = a.ep.fin_bf[0];
    }
    // reduce = false: the accumulators of one parity class; reduce = true (split-K, last workgroup of the tile): the class's sum over the slabs
    auto class_epilogue = [&](const v16f& o, int py, int px, const bool reduce) __attribute__((always_inline)) {
        if (!reduce) {
#pragma unroll
            for (int r = 0; r < 16; ++r) etile[((r & 3) + 8 * (r >> 2) + 4 * lh) * EPI_LD + l31] = o[r];
        }
        __builtin_amdgcn_wave_barrier();
        float4 v[4];
        size_t off[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = erow + 8 * k;
            v[k] = reduce ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(etile + row * EPI_LD + ec4);
            const int mm = wm * 32 + row;
            const int Y = 2 * (ty0 + mm / TW) + py, X = 2 * (tx0 + mm % TW) + px;
            off[k] = ((size_t)(n * d.HB + Y) * d.WB + X) * Nn + ecol;
        }
        __builtin_amdgcn_wave_barrier();
        float* outp = a.Out;
        if (nsplit > 1 && reduce) {
            const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.Out, 0, 0xffffffff, 0x00020000);
            for (int sp = 0; sp < nsplit; sp += 2) {          // split order, two slabs (8 loads) in flight
                float4 t[4][2];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int h = 0; h < 2; ++h) t[k][h] = sk_load16(srs, (unsigned)(((size_t)(sp + h) * a.out_elems + off[k]) * 4));
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int h = 0; h < 2; ++h) { v[k].x += t[k][h].x; v[k].y += t[k][h].y; v[k].z += t[k][h].z; v[k].w += t[k][h].w; }
            }
            outp = a.out_final;
        }
        if (nsplit > 1 && !reduce) {
            if (a.sk_counter) {
                const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.Out, 0, 0xffffffff, 0x00020000);
#pragma unroll
                for (int k = 0; k < 4; ++k) sk_store16(srs, (unsigned)(((size_t)split * a.out_elems + off[k]) * 4), v[k]);
            } else {
                float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
                for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(slab + off[k]) = v[k];
            }
        } else if (fin) {
            // last decoder block: BN + LeakyReLU, final 1x1 conv (C -> 1, reduced over the 8 lanes that share a pixel), L1 loss
            // and, if wanted, its gradient back to this layer's pre-BN output (models/customlayers.py:35-37, trainers/VAE.py:36-40)
            int lidx[4];
            float xin[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int mm = wm * 32 + erow + 8 * k;
                lidx[k] = (2 * (mm / TW) + py) * (2 * TW) + 2 * (mm % TW) + px;
                xin[k] = s_fx[lidx[k]];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float cc[4] = {v[k].x + e_a.x, v[k].y + e_a.y, v[k].z + e_a.z, v[k].w + e_a.w};
                const float scv[4] = {f_sc.x, f_sc.y, f_sc.z, f_sc.w}, shv[4] = {f_sh.x, f_sh.y, f_sh.z, f_sh.w};
                const float wv[4] = {f_w.x, f_w.y, f_w.z, f_w.w};
                float bn[4], av[4];
                float dot = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bn[e] = fmaf(cc[e], scv[e], shv[e]);
                    av[e] = bn[e] > 0.f ? bn[e] : bn[e] * a.ep.ealpha;
                    dot = fmaf(av[e], wv[e], dot);
                }
                dot = sum8_dpp(dot);
                const float xh = dot + f_bf;
                const float diff = xh - xin[k];
                // all 8 lanes of the pixel hold the same xh / diff: lanes 0..3 of the group each store one of the four per-pixel values
                // (x_hat, |diff|, pattern word, sign), the running sums are kept in every lane and read from lane 0 of the group
                rec += fabsf(diff);
                if (a.Out) *reinterpret_cast<float4*>(a.Out + off[k]) = make_float4(cc[0], cc[1], cc[2], cc[3]);
                unsigned pw = 0u;
                float sg = 0.f;
                if (a.ep.fin_dc || a.ep.fin_bits) {
                    const float sgn = (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * a.ep.fin_inv_batch;
                    float dc[4];
                    unsigned nib = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float da = sgn * wv[e];
                        const bool pos = bn[e] > 0.f;
                        const float dbn = pos ? da : da * a.ep.ealpha;
                        dc[e] = dbn * scv[e];
                        dwf[e] = fmaf(sgn, av[e], dwf[e]);
                        s1[e] += dbn;
                        s2[e] = fmaf(dbn, cc[e], s2[e]);
                        nib |= (pos ? 1u : 0u) << e;
                    }
                    if (a.ep.fin_dc) *reinterpret_cast<float4*>(a.ep.fin_dc + off[k]) = make_float4(dc[0], dc[1], dc[2], dc[3]);
                    // d loss / d c of this pixel = sgn * w_f[ch] * (bit ? 1 : alpha) * scale[ch]: one word + one float instead of 32 floats
                    pw = or8_dpp(nib << ecol);
                    sg = sgn;
                    dbf += sgn;
                }
                {
                    const int role = lane & 3;
                    const float val = role == 0 ? xh : role == 1 ? fabsf(diff) : role == 2 ? __uint_as_float(pw) : sg;
                    if ((lane & 4) == 0) s_fo[role * (4 * TH * TW) + lidx[k]] = val;      // s_fo | s_fl | s_fb | s_fg are adjacent
                }
            }
        } else if (!bwd) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float4 t = v[k];
                t.x += e_a.x; t.y += e_a.y; t.z += e_a.z; t.w += e_a.w;
                if (a.ep.mul) { const float4 q = *reinterpret_cast<const float4*>(a.ep.mul + off[k]); t.x *= q.x; t.y *= q.y; t.z *= q.z; t.w *= q.w; }
                if (a.ep.add) { const float4 q = *reinterpret_cast<const float4*>(a.ep.add + off[k]); t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w; }
                *reinterpret_cast<float4*>(outp + off[k]) = t;
            }
        } else {
            float4 cp[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) cp[k] = *reinterpret_cast<const float4*>(a.ep.cprev + off[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float vv[4] = {v[k].x, v[k].y, v[k].z, v[k].w}, cc[4] = {cp[k].x, cp[k].y, cp[k].z, cp[k].w};
                const float aa[4] = {e_a.x, e_a.y, e_a.z, e_a.w}, bb[4] = {e_b.x, e_b.y, e_b.z, e_b.w};
                float oo[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float bn = fmaf(aa[e], cc[e], bb[e]);
                    const float dbn = bn > 0.f ? vv[e] : vv[e] * a.ep.ealpha;
                    oo[e] = dbn * aa[e];
                    s1[e] += dbn;
                    s2[e] = fmaf(dbn, cc[e], s2[e]);
                }
                *reinterpret_cast<float4*>(outp + off[k]) = make_float4(oo[0], oo[1], oo[2], oo[3]);
            }
        }
    };

    // The unit sequence is expanded at compile time (static_for, not `#pragma unroll`: the optimizer declined to unroll the loop form
    // and then selected tap / class / accumulator-reset at run time -- 48 v_cndmask per unit of 6 MFMAs).
    v16f acc0, acc1, acc2;
    BFrag16<2> a0, a1;
    loadA(a0, 0);
    auto unit = [&](const BFrag16<2>& bc, BFrag16<2>& bpf, const BFrag16<2>& ac, BFrag16<2>& an, auto S) __attribute__((always_inline)) {
        constexpr int sidx = decltype(S)::value;
        constexpr int t = sidx / NCH, kc = sidx % NCH;
        constexpr int tap = kTapOrderD.tap[t];
        constexpr int ky = tap / 5, kx = tap % 5;
        constexpr int py = (ky + 1) & 1, px = (kx + 1) & 1;
        constexpr int cls = py * 2 + px;
        constexpr bool first = (kc == 0 && t == kTapOrderD.start[cls]);
        constexpr bool last = (kc == NCH - 1 && t + 1 == kTapOrderD.start[cls + 1]);
        if constexpr (sidx + 3 < NUNIT) loadB(bpf, sidx + 3);
        if constexpr (sidx + 1 < NUNIT) loadA(an, sidx + 1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (first) {
            const v16f z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc0 = mfma_bf16(ac.hi[0], bc.hi[0], z);
            acc1 = mfma_bf16(ac.hi[0], bc.lo[0], z);
            acc2 = mfma_bf16(ac.lo[0], bc.hi[0], z);
        } else {
            acc0 = mfma_bf16(ac.hi[0], bc.hi[0], acc0);
            acc1 = mfma_bf16(ac.hi[0], bc.lo[0], acc1);
            acc2 = mfma_bf16(ac.lo[0], bc.hi[0], acc2);
        }
        acc0 = mfma_bf16(ac.hi[1], bc.hi[1], acc0);
        acc1 = mfma_bf16(ac.hi[1], bc.lo[1], acc1);
        acc2 = mfma_bf16(ac.lo[1], bc.hi[1], acc2);
        if constexpr (last) {
            // ---- epilogue of this parity class ----
            v16f o;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = acc0[r] + (acc1[r] + acc2[r]);
            class_epilogue(o, py, px, false);
        }
    };
    static_for<0, (NUNIT + 3) / 4>([&](auto G) __attribute__((always_inline)) {
        constexpr int g4 = decltype(G)::value;
        if constexpr (4 * g4 + 0 < NUNIT) unit(b0, b3, a0, a1, std::integral_constant<int, 4 * g4 + 0>{});
        if constexpr (4 * g4 + 1 < NUNIT) unit(b1, b0, a1, a0, std::integral_constant<int, 4 * g4 + 1>{});
        if constexpr (4 * g4 + 2 < NUNIT) unit(b2, b1, a0, a1, std::integral_constant<int, 4 * g4 + 2>{});
        if constexpr (4 * g4 + 3 < NUNIT) unit(b3, b2, a1, a0, std::integral_constant<int, 4 * g4 + 3>{});
    });
    if (fin) {
        // workgroup partials in the final kernel's layout: red_partial[tile][3C+1] = {dwf[C], S1[C], S2[C], dbf}, rec_partial[tile]
        __syncthreads();                        // every wave is done with its transpose tile (s_epi is reused below)
        for (int idx = tid; idx < 4 * TH * TW; idx += NT) {
            const int yl = idx / (2 * TW), xl = idx % (2 * TW);
            const size_t pix = ((size_t)n * d.HB + 2 * ty0 + yl) * d.WB + 2 * tx0 + xl;
            a.ep.fin_xhat[pix] = s_fo[idx];
            if (a.ep.fin_l1) a.ep.fin_l1[pix] = s_fl[idx];
            if (a.ep.fin_bits) { a.ep.fin_bits[pix] = s_fb[idx]; a.ep.fin_dxhat[pix] = s_fg[idx]; }
        }
        float* fr = s_epi;                      // [waves][3*BN + 2]
        constexpr int FL = 3 * BN + 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t0 = dwf[e], t1 = s1[e], t2 = s2[e];
            t0 += __shfl_xor(t0, 8); t0 += __shfl_xor(t0, 16); t0 += __shfl_xor(t0, 32);
            t1 += __shfl_xor(t1, 8); t1 += __shfl_xor(t1, 16); t1 += __shfl_xor(t1, 32);
            t2 += __shfl_xor(t2, 8); t2 += __shfl_xor(t2, 16); t2 += __shfl_xor(t2, 32);
            if (lane < 8) {
                fr[wave * FL + 0 * BN + wn * 32 + ec4 + e] = t0;
                fr[wave * FL + 1 * BN + wn * 32 + ec4 + e] = t1;
                fr[wave * FL + 2 * BN + wn * 32 + ec4 + e] = t2;
            }
        }
        float r0 = rec, r1 = dbf;
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) { r0 += __shfl_xor(r0, o); r1 += __shfl_xor(r1, o); }
        if (lane == 0) { fr[wave * FL + 3 * BN] = r1; fr[wave * FL + 3 * BN + 1] = r0; }
        __syncthreads();
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        if (tid < FL) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM * WGN; ++w) t += fr[w * FL + tid];
            if (tid == 3 * BN + 1) a.ep.fin_rec_partial[tile] = t;
            else if (a.ep.fin_dc || a.ep.fin_bits) a.ep.fin_red_partial[tile * (3 * BN + 1) + tid] = t;
        }
        return;
    }
    if (nsplit > 1) {
        if (!a.sk_counter) return;            // splitk_epilogue_kernel finishes the job
        const unsigned slot = (blockIdx.y * gridDim.x + blockIdx.x) * (gridDim.z / nsplit) + blockIdx.z / nsplit;
        if (!sk_last_arriver(a.sk_counter + slot, nsplit, reinterpret_cast<int*>(s_red), tid)) return;
        const v16f none = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        class_epilogue(none, 0, 0, true); class_epilogue(none, 0, 1, true); class_epilogue(none, 1, 0, true); class_epilogue(none, 1, 1, true);
    }
    if (bwd) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t1 = s1[e], t2 = s2[e];
            t1 += __shfl_xor(t1, 8); t1 += __shfl_xor(t1, 16); t1 += __shfl_xor(t1, 32);
            t2 += __shfl_xor(t2, 8); t2 += __shfl_xor(t2, 16); t2 += __shfl_xor(t2, 32);
            if (lane < 8) {
                s_red[(wm * 2 + 0) * BN + wn * 32 + ec4 + e] = t1;
                s_red[(wm * 2 + 1) * BN + wn * 32 + ec4 + e] = t2;
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += s_red[(w * 2 + which) * BN + c];
            const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            if (n0 + c < Nn) a.ep.colpart[(tile * 2 + which) * Nn + n0 + c] = t;
        }
    }
}

// FIN (round 4): the last decoder block of the exact-fp32 mode -- its BN + LeakyReLU, the final 1 x 1 convolution, the L1 loss and the loss
// gradient run in this kernel's epilogue exactly as in conv5_d16_kernel (UAD_EPI_FINAL), instead of a final_kernel pass that re-reads the
// block's 128 B / pixel output; the epilogue's tiles alias the halo tile, so the instance needs no more LDS than the plain one.
template <int TH, int TW, int CK, int WGM, int WGN, bool FIN = false>
__global__ void __launch_bounds__(64 * WGM * WGN) conv5_d_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = TH + 2, IW = TW + 2;
    constexpr int LDC = CK + 4, NKK = CK / 8, CQ = CK / 4;
    constexpr int BN = 32 * WGN;
    static_assert(TH * TW == 32 * WGM, "one 32-row fragment per wave along M");
    __shared__ __attribute__((aligned(16))) float sIn[IH * IW * LDC];
    __shared__ __attribute__((aligned(16))) float s_xf[2 * XF_LDS_CH];
    __shared__ float s_red[WGM * 2 * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int tilesx = d.WS / TW;
    const int ty0 = (blockIdx.x / tilesx) * TH, tx0 = (blockIdx.x % tilesx) * TW;
    const int n = blockIdx.y;
    const int nsplit = a.nsplit;
    const int n0 = (blockIdx.z / nsplit) * BN;
    const int split = blockIdx.z % nsplit;
    const int CB = d.CB, CS = d.CS;   // output channels = CB, contraction = CS

    const bool xf = a.xf.scale != nullptr;
    if (xf)
        for (int c = tid; c < CS; c += NT) {
            s_xf[c] = a.xf.scale[c] * a.xf.mult;
            s_xf[XF_LDS_CH + c] = a.xf.shift[c];
        }

    const int m = wm * 32 + l31;
    const int pty = m / TW, ptx = m % TW;
    const int aoff = ((pty + 1) * IW + ptx + 1) * LDC + 4 * lh;
    const int col = n0 + wn * 32 + l31;
    const bool colok = col < CB;
    const int colc = colok ? col : 0;
    // packed weights Wq[tap][cs/4][cb][4] (contraction quad innermost, output channel next): coalesced 16-byte loads
    const float* wptr = a.Wp + ((size_t)lh * CB + colc) * 4;

    BFragD<NKK> b0, b1;
    auto loadB = [&](BFragD<NKK>& b, int tap, int c0) {
        const float* w = wptr + ((size_t)tap * CS + c0) * CB;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) b.v[kk] = *reinterpret_cast<const float4*>(w + (size_t)(kk * 2) * CB * 4);
    };

    v16f acc[4];   // output-parity classes (py, px)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    const int cper = (CS / CK + nsplit - 1) / nsplit;
    const int ch0 = split * cper;
    const int nchunks = min(CS / CK, ch0 + cper);
    const float* inb = a.A + (size_t)n * d.HS * d.WS * CS;
    loadB(b0, 0, ch0 * CK);
    __syncthreads();

    for (int ch = ch0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        if (ch > ch0) __syncthreads();
        constexpr int TOT = IH * IW * CQ;
        constexpr int BATCH = 4;
        for (int f0 = tid; f0 < TOT; f0 += NT * BATCH) {
            float4 v[BATCH];
            bool ok[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                const int pix = f / CQ, cq = f % CQ;
                const int iy = pix / IW, ix = pix % IW;
                const int gy = ty0 - 1 + iy, gx = tx0 - 1 + ix;
                ok[u] = (f < TOT) && (unsigned)gy < (unsigned)d.HS && (unsigned)gx < (unsigned)d.WS;
                const int gp = ok[u] ? (gy * d.WS + gx) : 0;
                v[u] = *reinterpret_cast<const float4*>(inb + (size_t)gp * CS + c0 + (ok[u] ? cq * 4 : 0));
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                if (f >= TOT) continue;
                const int pix = f / CQ, cq = f % CQ;
                float4 t = v[u];
                if (xf) {
                    const float4 sc = *reinterpret_cast<const float4*>(s_xf + c0 + cq * 4);
                    const float4 sh = *reinterpret_cast<const float4*>(s_xf + XF_LDS_CH + c0 + cq * 4);
                    t = xform4(t, sc, sh, a.xf.alpha);
                }
                *reinterpret_cast<float4*>(sIn + pix * LDC + cq * 4) = keep4(ok[u], t);
            }
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 25; ++tap) {
            const int ky = tap / 5, kx = tap % 5;
            // y[2i-1+ky] += x[i]: output parity py = (ky+1)&1, source row i + dy with dy = (py + 1 - ky) / 2
            const int py = (ky + 1) & 1, px = (kx + 1) & 1;
            const int dy = (py + 1 - ky) / 2, dx = (px + 1 - kx) / 2;
            const int cls = py * 2 + px;
            BFragD<NKK>& cur = (tap & 1) ? b1 : b0;
            BFragD<NKK>& nxt = (tap & 1) ? b0 : b1;
            if (tap < 24) loadB(nxt, tap + 1, c0);
            else if (ch + 1 < nchunks) loadB(nxt, 0, c0 + CK);
            // keep the prefetch a full tap ahead: without this fence the scheduler sinks the loads to their first
            // use (vmcnt(0) right behind the issue) and every tap eats an L2 round trip
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const float4 av = *reinterpret_cast<const float4*>(sIn + aoff + (dy * IW + dx) * LDC + kk * 8);
                acc[cls] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, cur.v[kk].x, acc[cls], 0, 0, 0);
                acc[cls] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, cur.v[kk].y, acc[cls], 0, 0, 0);
                acc[cls] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, cur.v[kk].z, acc[cls], 0, 0, 0);
                acc[cls] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, cur.v[kk].w, acc[cls], 0, 0, 0);
            }
        }
        b0 = b1;
    }

    if constexpr (FIN) {
        // (models/customlayers.py:35-37 + trainers/VAE.py:36-40 behind the last Conv2DTranspose; partials in final_kernel's layout)
        static_assert(WGN == 1, "one 32-channel column block holds every channel of the last block");
        constexpr int EPI_LD = 36;
        float* s_epi = sIn;                                   // per-wave 32 x EPI_LD transpose tile (the halo tile is dead by now)
        float* s_fx = s_epi + WGM * 32 * EPI_LD;              // target | reconstruction | L1 tiles of the 2TH x 2TW output block
        float* s_fo = s_fx + 4 * TH * TW;                     // (s_fo | s_fl adjacent)
        static_assert(WGM * 32 * EPI_LD + 3 * 4 * TH * TW <= IH * IW * LDC, "epilogue tiles fit in the halo tile");
        __syncthreads();
        for (int idx = tid; idx < 4 * TH * TW; idx += NT) {
            const int yl = idx / (2 * TW), xl = idx % (2 * TW);
            s_fx[idx] = a.ep.fin_x[((size_t)n * d.HB + 2 * ty0 + yl) * d.WB + 2 * tx0 + xl];
        }
        __syncthreads();
        float* etile = s_epi + wave * 32 * EPI_LD;
        const int ec4 = (lane & 7) * 4, erow = lane >> 3;
        const int ecol = n0 + ec4;                            // CB == 32: always in range
        float4 e_a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.ep.bias) e_a = *reinterpret_cast<const float4*>(a.ep.bias + ecol);
        float4 f_sc = *reinterpret_cast<const float4*>(a.ep.escale + ecol);
        f_sc.x *= a.ep.emult; f_sc.y *= a.ep.emult; f_sc.z *= a.ep.emult; f_sc.w *= a.ep.emult;
        const float4 f_sh = *reinterpret_cast<const float4*>(a.ep.eshift + ecol);
        const float4 f_w = *reinterpret_cast<const float4*>(a.ep.fin_wf + ecol);
        const float f_bf = a.ep.fin_bf[0];
        const float scv[4] = {f_sc.x, f_sc.y, f_sc.z, f_sc.w}, shv[4] = {f_sh.x, f_sh.y, f_sh.z, f_sh.w};
        const float wv[4] = {f_w.x, f_w.y, f_w.z, f_w.w};
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, dwf[4] = {0.f, 0.f, 0.f, 0.f};
        float rec = 0.f, dbf = 0.f;
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int py = cls >> 1, px = cls & 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) etile[((r & 3) + 8 * (r >> 2) + 4 * lh) * EPI_LD + l31] = acc[cls][r];
            __builtin_amdgcn_wave_barrier();
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(etile + (erow + 8 * k) * EPI_LD + ec4);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int mm = wm * 32 + erow + 8 * k;
                const int Y = 2 * (ty0 + mm / TW) + py, X = 2 * (tx0 + mm % TW) + px;
                const size_t off = ((size_t)(n * d.HB + Y) * d.WB + X) * CB + ecol;
                const int lidx = (2 * (mm / TW) + py) * (2 * TW) + 2 * (mm % TW) + px;
                const float cc[4] = {v[k].x + e_a.x, v[k].y + e_a.y, v[k].z + e_a.z, v[k].w + e_a.w};
                float bn[4], av[4];
                float dot = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bn[e] = fmaf(cc[e], scv[e], shv[e]);
                    av[e] = bn[e] > 0.f ? bn[e] : bn[e] * a.ep.ealpha;
                    dot = fmaf(av[e], wv[e], dot);
                }
                dot = sum8_dpp(dot);                          // the 8 lanes that share the pixel
                const float xh = dot + f_bf;
                const float diff = xh - s_fx[lidx];
                rec += fabsf(diff);
                if (a.Out) *reinterpret_cast<float4*>(a.Out + off) = make_float4(cc[0], cc[1], cc[2], cc[3]);
                if (a.ep.fin_dc) {
                    const float sgn = (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * a.ep.fin_inv_batch;
                    float dc[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float da = sgn * wv[e];
                        const float dbn = bn[e] > 0.f ? da : da * a.ep.ealpha;
                        dc[e] = dbn * scv[e];
                        dwf[e] = fmaf(sgn, av[e], dwf[e]);
                        s1[e] += dbn;
                        s2[e] = fmaf(dbn, cc[e], s2[e]);
                    }
                    *reinterpret_cast<float4*>(a.ep.fin_dc + off) = make_float4(dc[0], dc[1], dc[2], dc[3]);
                    dbf += sgn;
                }
                if ((lane & 6) == 0) s_fo[(lane & 1) * (4 * TH * TW) + lidx] = (lane & 1) ? fabsf(diff) : xh;
            }
        }
        __syncthreads();                                      // every wave is done with its transpose tile (reused below)
        for (int idx = tid; idx < 4 * TH * TW; idx += NT) {
            const int yl = idx / (2 * TW), xl = idx % (2 * TW);
            const size_t pix = ((size_t)n * d.HB + 2 * ty0 + yl) * d.WB + 2 * tx0 + xl;
            a.ep.fin_xhat[pix] = s_fo[idx];
            if (a.ep.fin_l1) a.ep.fin_l1[pix] = s_fo[4 * TH * TW + idx];
        }
        // workgroup partials: red_partial[tile][3C + 1] = {dwf[C], S1[C], S2[C], dbf}, rec_partial[tile]
        float* fr = s_epi;
        constexpr int FL = 3 * BN + 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t0 = dwf[e], t1 = s1[e], t2 = s2[e];
            t0 += __shfl_xor(t0, 8); t0 += __shfl_xor(t0, 16); t0 += __shfl_xor(t0, 32);
            t1 += __shfl_xor(t1, 8); t1 += __shfl_xor(t1, 16); t1 += __shfl_xor(t1, 32);
            t2 += __shfl_xor(t2, 8); t2 += __shfl_xor(t2, 16); t2 += __shfl_xor(t2, 32);
            if (lane < 8) {
                fr[wave * FL + 0 * BN + ec4 + e] = t0;
                fr[wave * FL + 1 * BN + ec4 + e] = t1;
                fr[wave * FL + 2 * BN + ec4 + e] = t2;
            }
        }
        float r0 = rec, r1 = dbf;
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) { r0 += __shfl_xor(r0, o); r1 += __shfl_xor(r1, o); }
        if (lane == 0) { fr[wave * FL + 3 * BN] = r1; fr[wave * FL + 3 * BN + 1] = r0; }
        __syncthreads();
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        if (tid < FL) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += fr[w * FL + tid];
            if (tid == 3 * BN + 1) a.ep.fin_rec_partial[tile] = t;
            else if (a.ep.fin_dc) a.ep.fin_red_partial[tile * (3 * BN + 1) + tid] = t;
        }
        return;
    }

    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    float c_a, c_b = 0.f;
    if (!bwd) c_a = a.ep.bias ? a.ep.bias[colc] : 0.f;
    else { c_a = a.ep.escale[colc] * a.ep.emult; c_b = a.ep.eshift[colc]; }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
        const int py = cls >> 1, px = cls & 1;
        size_t obase[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int Y = 2 * (ty0 + mm / TW) + py, X = 2 * (tx0 + mm % TW) + px;
            obase[r] = ((size_t)(n * d.HB + Y) * d.WB + X) * CB;
        }
        if (nsplit > 1) {
            float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (colok) slab[obase[r] + colc] = acc[cls][r];
        } else {
            epilogue_frag<0>(a, acc[cls], obase, colok, colc, c_a, c_b, s1, s2);
        }
    }
    if (nsplit > 1) return;
    if (bwd) {
        const float t1 = s1 + __shfl_xor(s1, 32), t2 = s2 + __shfl_xor(s2, 32);
        if (lh == 0) {
            s_red[(wm * 2 + 0) * BN + wn * 32 + l31] = t1;
            s_red[(wm * 2 + 1) * BN + wn * 32 + l31] = t2;
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += s_red[(w * 2 + which) * BN + c];
            const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            if (n0 + c < CB) a.ep.colpart[(tile * 2 + which) * CB + n0 + c] = t;
        }
    }
}



template <int TH, int TW, int CST, int WGM, int WGN>
constexpr size_t conv5_d16_lds_bytes() {
    return (size_t)2 * (TH + 2) * (TW + 2) * (CST + 8) * 2 + (size_t)2 * XF_LDS_CH * 4 + (size_t)WGM * 2 * 32 * WGN * 4 +
           (size_t)WGM * WGN * 32 * 36 * 4 + (size_t)5 * 4 * TH * TW * 4;
}
template <int TH, int TW, int CST, int WGM, int WGN>
void launch_conv5_d16(const ConvGemmArgs& a, dim3 grid, hipStream_t st) {
    constexpr size_t lds = conv5_d16_lds_bytes<TH, TW, CST, WGM, WGN>();
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_d16_kernel<TH, TW, CST, WGM, WGN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((conv5_d16_kernel<TH, TW, CST, WGM, WGN>), grid, dim3(64 * WGM * WGN), lds, st, a);
}

template <int TH, int TW, int CK, int WGM, int WGN>
constexpr size_t conv5_bf16_lds_bytes() {
    return (size_t)2 * (TH + 2) * (TW + 2) * (CK + 8) * 2 + (size_t)2 * XF_LDS_CH * 4 + (size_t)WGM * 2 * 32 * WGN * 4;
}

template <int TH, int TW, int CK, int WGM, int WGN>
void launch_conv5_bf16(const ConvGemmArgs& a, dim3 grid, hipStream_t st) {
    constexpr size_t lds = conv5_bf16_lds_bytes<TH, TW, CK, WGM, WGN>();
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_bf16_kernel<TH, TW, CK, WGM, WGN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((conv5_bf16_kernel<TH, TW, CK, WGM, WGN>), grid, dim3(64 * WGM * WGN), lds, st, a);
}

}  // namespace

// (bn, cst): one of the planner's d16_instance() list
void uad_conv5_d16_launch(const ConvGemmArgs& a, dim3 grid, int bn, int cst, hipStream_t st) {
    if (bn == 64) {
        if (cst == 128) launch_conv5_d16<8, 8, 128, 2, 2>(a, grid, st);
        else if (cst == 64) launch_conv5_d16<8, 8, 64, 2, 2>(a, grid, st);
        else launch_conv5_d16<8, 8, 32, 2, 2>(a, grid, st);
    } else if (cst == 64) launch_conv5_d16<8, 16, 64, 4, 1>(a, grid, st);
    else launch_conv5_d16<8, 16, 32, 4, 1>(a, grid, st);
}

void uad_conv5_dbf16_launch(const ConvGemmArgs& a, dim3 grid, int bn, int ck, hipStream_t st) {
    if (bn == 64) launch_conv5_bf16<8, 8, 32, 2, 2>(a, grid, st);
    else if (ck == 32) launch_conv5_bf16<8, 16, 32, 4, 1>(a, grid, st);
    else launch_conv5_bf16<8, 16, 16, 4, 1>(a, grid, st);
}

void uad_conv5_d32_launch(const ConvGemmArgs& a, dim3 grid, int bn, int ck, bool fin, bool any_order, hipStream_t st) {
    if (fin) UAD_SPATIAL_LAUNCH(any_order, (conv5_d_kernel<8, 16, 32, 4, 1, true>), grid, dim3(256), 0, st, a);
    else if (bn == 64) UAD_SPATIAL_LAUNCH(any_order, (conv5_d_kernel<8, 8, 32, 2, 2>), grid, dim3(256), 0, st, a);
    else if (ck == 32) UAD_SPATIAL_LAUNCH(any_order, (conv5_d_kernel<8, 16, 32, 4, 1>), grid, dim3(256), 0, st, a);
    else UAD_SPATIAL_LAUNCH(any_order, (conv5_d_kernel<8, 16, 16, 4, 1>), grid, dim3(256), 0, st, a);
}
