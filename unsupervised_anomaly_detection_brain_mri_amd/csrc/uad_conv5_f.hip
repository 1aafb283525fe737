// k5 s2 F kind ("gather"): conv5_f16_kernel on bf16 planes (bf16x3 / bf16x6) and conv5_f_kernel in exact fp32.  uad_conv_plan.hip decides the instance and
// calls uad_conv5_f16_launch / uad_conv5_f32_launch below.
// ================================================================================================
// k5 s2 SAME specialisations ("spatial" kernels): the input halo tile of one channel chunk is staged in LDS ONCE
// (activation applied on the way in) and all 25 taps are contracted from it; the weight fragments go global -> VGPR,
// prefetched one tap ahead, so the tap loop has no barrier and no per-tap address arithmetic (tap offsets are
// immediates).  One workgroup = TH x TW output positions (F) / input-resolution positions (D) x 32*WGN channels.
// ================================================================================================
#include "uad_gemm_common.h"

namespace {

template <int TH, int TW, int CK, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) conv5_f_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = 2 * TH + 3, IW = 2 * TW + 3;
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
    const int CB = d.CB, CS = d.CS;

    const bool xf = a.xf.scale != nullptr;
    if (xf)
        for (int c = tid; c < CB; c += NT) {
            s_xf[c] = a.xf.scale[c] * a.xf.mult;
            s_xf[XF_LDS_CH + c] = a.xf.shift[c];
        }

    const int m = wm * 32 + l31;
    const int pty = m / TW, ptx = m % TW;
    const int aoff = ((2 * pty) * IW + 2 * ptx) * LDC + 4 * lh;
    const int col = n0 + wn * 32 + l31;
    const bool colok = col < CS;
    const int colc = colok ? col : 0;
    // packed weights Wp[tap][cb/4][cs][4]: the lane's four k-slots of one k-slice are ONE 16-byte load and the
    // 32 lanes of a half-wave read 512 contiguous bytes
    const float* wptr = a.Wp + ((size_t)lh * CS + colc) * 4;

    BFragD<NKK> b0, b1;
    auto loadB = [&](BFragD<NKK>& b, int tap, int c0) {
        const float* w = wptr + ((size_t)tap * CB + c0) * CS;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) b.v[kk] = *reinterpret_cast<const float4*>(w + (size_t)(kk * 2) * CS * 4);
    };

    // four independent accumulator chains (one per k-slot of the float4 fragment): an MFMA never waits on its
    // predecessor, so the ds_reads / weight loads interleaved between them cost no matrix-pipe time
    v16f acc4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc4[q][r] = 0.f;

    // split-K: this workgroup contracts channel chunks [ch0, nchunks)
    const int cper = (CB / CK + nsplit - 1) / nsplit;
    const int ch0 = split * cper;
    const int nchunks = min(CB / CK, ch0 + cper);
    const int gy0 = 2 * ty0 - 1, gx0 = 2 * tx0 - 1;
    const float* inb = a.A + (size_t)n * d.HB * d.WB * CB;
    loadB(b0, 0, ch0 * CK);
    __syncthreads();  // s_xf visible

    for (int ch = ch0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        if (ch > ch0) __syncthreads();  // everyone is done reading the previous chunk's tile
        // ---- stage the halo tile of this channel chunk (activation on the way in, padding = exact 0) ----
        constexpr int TOT = IH * IW * CQ;
        constexpr int BATCH = 6;
        for (int f0 = tid; f0 < TOT; f0 += NT * BATCH) {
            float4 v[BATCH];
            bool ok[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int f = f0 + u * NT;
                const int pix = f / CQ, cq = f % CQ;
                const int iy = pix / IW, ix = pix % IW;
                const int gy = gy0 + iy, gx = gx0 + ix;
                ok[u] = (f < TOT) && (unsigned)gy < (unsigned)d.HB && (unsigned)gx < (unsigned)d.WB;
                const int gp = ok[u] ? (gy * d.WB + gx) : 0;
                v[u] = *reinterpret_cast<const float4*>(inb + (size_t)gp * CB + c0 + (ok[u] ? cq * 4 : 0));
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
        // ---- 25 taps from LDS; weights one tap ahead in registers ----
#pragma unroll
        for (int tap = 0; tap < 25; ++tap) {
            const int ky = tap / 5, kx = tap % 5;
            BFragD<NKK>& cur = (tap & 1) ? b1 : b0;
            BFragD<NKK>& nxt = (tap & 1) ? b0 : b1;
            if (tap < 24) loadB(nxt, tap + 1, c0);
            else if (ch + 1 < nchunks) loadB(nxt, 0, c0 + CK);
            // keep the prefetch a full tap ahead: without this fence the scheduler sinks the loads to their first
            // use (vmcnt(0) right behind the issue) and every tap eats an L2 round trip
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const float4 av = *reinterpret_cast<const float4*>(sIn + aoff + (ky * IW + kx) * LDC + kk * 8);
                acc4[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, cur.v[kk].x, acc4[0], 0, 0, 0);
                acc4[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, cur.v[kk].y, acc4[1], 0, 0, 0);
                acc4[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, cur.v[kk].z, acc4[2], 0, 0, 0);
                acc4[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, cur.v[kk].w, acc4[3], 0, 0, 0);
            }
        }
        b0 = b1;  // 25 taps is odd: the prefetched tap 0 of the next chunk sits in b1
    }

    // ---- epilogue ----
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = (acc4[0][r] + acc4[1][r]) + (acc4[2][r] + acc4[3][r]);
    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    float c_a, c_b = 0.f;
    if (!bwd) c_a = a.ep.bias ? a.ep.bias[colc] : 0.f;
    else { c_a = a.ep.escale[colc] * a.ep.emult; c_b = a.ep.eshift[colc]; }
    size_t obase[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mm = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int oy = ty0 + mm / TW, ox = tx0 + mm % TW;
        obase[r] = ((size_t)(n * d.HS + oy) * d.WS + ox) * CS;
    }
    float s1 = 0.f, s2 = 0.f;
    if (nsplit > 1) {   // raw partial tile into this split's slab; splitk_epilogue_kernel finishes the job
        float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (colok) slab[obase[r] + colc] = acc[r];
        return;
    }
    epilogue_frag<0>(a, acc, obase, colok, colc, c_a, c_b, s1, s2);
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
            if (n0 + c < CS) a.ep.colpart[(tile * 2 + which) * CS + n0 + c] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// F-kind (gather) bf16x3 kernel with the same pipeline as conv5_d16_kernel: weight fragments three taps ahead in a VGPR ring,
// activation fragments double-buffered out of LDS one tap ahead, transposed 16-byte epilogue.  The (2TH+3)x(2TW+3) halo is
// too large to hold every channel at once, so channels are walked in CK-wide chunks (restaged per chunk, accumulators live
// across chunks); the weight ring runs through the chunk boundary.
// ------------------------------------------------------------------------------------------------
// Round 6: the staging phases on the same diet as conv5_w_bf16_tr_kernel -- the tile is fixed for a workgroup, so the byte offset of each of a
// thread's elements (out-of-image elements: 2^31 = the descriptor's size, the range check returns zeros), the padding mask and the LDS store
// addresses are computed ONCE; a chunk adds a wave-uniform channel offset.  Activation-on-load or not is a template parameter (XF).
template <int TH, int TW, int CK, int WGM, int WGN, int FB, bool XF, int NPL = 2>      // FB: 0 plain | 1 final-backward on load from c | 2 ... from the pattern bits; NPL: bf16 planes per operand (3 = bf16x6)
__global__ void __launch_bounds__(64 * WGM * WGN) __attribute__((amdgpu_waves_per_eu(2))) conv5_f16_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = 2 * TH + 3, IW = 2 * TW + 3;
    constexpr int LDH = CK + 8;
    constexpr int NKS = CK / 16, CQ = CK / 4;
    constexpr int BN = 32 * WGN;
    static_assert(TH * TW == 32 * WGM, "one 32-row fragment per wave along M");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    constexpr int PLANE = IH * IW * LDH;
    unsigned short* sPl = reinterpret_cast<unsigned short*>(dsm);      // NPL planes of IH x IW x LDH
    float* s_xf = reinterpret_cast<float*>(sPl + NPL * PLANE);
    float* s_red = s_xf + 3 * XF_LDS_CH;      // s_xf: scale | shift | final-conv kernel (fb mode)
    float* s_epi = reinterpret_cast<float*>(dsm);      // aliases the activation tile (dead after the last chunk)

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
    const int AH = d.HB, AW = d.WB;

    constexpr bool xf = XF;
    constexpr bool fb = FB == 1 || FB == 2;  // final-backward on load (UadXform::fb_*): its own instantiation, the extra
                                             // prefetch registers would otherwise spill the 64-column variant
    constexpr bool fbb = FB == 2;            // ... from one pattern word per pixel instead of the 32 pre-BN values (UadXform::fb_bits)
    static_assert(!(fb && !XF), "the final-backward forms are instantiated with XF = true (they read the scale table)");
    if (xf)
        for (int c = tid; c < CA; c += NT) {
            s_xf[c] = a.xf.scale[c] * a.xf.mult;
            s_xf[XF_LDS_CH + c] = a.xf.shift[c];
            if (fb) s_xf[2 * XF_LDS_CH + c] = a.xf.fb_wf[c];
        }
    const int m = wm * 32 + l31;
    const int pty = m / TW, ptx = m % TW;
    const int aoff = ((2 * pty) * IW + 2 * ptx) * LDH + 8 * lh;
    const int col = n0 + wn * 32 + l31;
    const int colc = col < Nn ? col : 0;
    const uint4* wq = reinterpret_cast<const uint4*>(a.Wp16) + (size_t)lh * Nn + colc;
    const size_t plane_q = (size_t)a.w16_plane / 8;

    const int cper = (CA / CK + nsplit - 1) / nsplit;
    const int ch0 = split * cper;
    const int nchunks = min(CA / CK, ch0 + cper);

    KFrag<NKS, NPL> b0, b1, b2, b3, a0, a1;
    // wave-uniform base (SGPR pair, scalar arithmetic) + one 32-bit per-lane offset: no 64-bit VALU add per load
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.Wp16), 0, 0xffffffff, 0x00020000);
    const unsigned lb = (unsigned)(wq - reinterpret_cast<const uint4*>(a.Wp16)) * 16u;      // byte offsets, 32 bits: the packed weights of a layer are < 4 GB
    const unsigned plane_b = (unsigned)plane_q * 16u;
    auto loadB = [&](KFrag<NKS, NPL>& b, int tap, int c0) {
        const unsigned u = (unsigned)((tap * (CA / 8) + c0 / 8) * Nn) * 16u;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) b.p[p][j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u + (unsigned)p * plane_b);
    };

    auto loadA = [&](KFrag<NKS, NPL>& f, int tap) {
        const int toff = ((tap / 5) * IW + (tap % 5)) * LDH;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) f.p[p][j] = *reinterpret_cast<const uint4*>(sPl + p * PLANE + aoff + toff + 16 * j);
    };
    loadB(b0, 0, ch0 * CK);
    loadB(b1, 1, ch0 * CK);
    loadB(b2, 2, ch0 * CK);

    v16f acc0, acc1, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; acc2[r] = 0.f; }

    const int gy0 = 2 * ty0 - 1, gx0 = 2 * tx0 - 1;

    // ---- this thread's share of the halo tile: elements (pixel pix0 + u DP, channel quad cq), the same for every chunk ----
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    constexpr int DP = NT / CQ;
    static_assert(NT % CQ == 0 && (PER - 1) * DP < IH * IW, "only a thread's LAST element can fall off the tile");
    const int cq = tid % CQ, pix0 = tid / CQ;
    unsigned voff[PER];                        // byte offset inside the sample (FB 2: of the pixel's 4-byte word), 2^31 when the element is padding
    unsigned voffg[FB == 1 ? PER : 1];         // FB 1 only: the pixel's word of d objective / d x_hat beside its channel quad
    unsigned bad = 0;                          // bit u: element u is padding (zero AFTER the activation)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int pix = pix0 + u * DP, iy = pix / IW, ix = pix % IW;
        const int gy = gy0 + iy, gx = gx0 + ix;
        const bool ok = (u + 1 < PER || pix < IH * IW) && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
        const unsigned gp = (unsigned)(gy * AW + gx);
        voff[u] = ok ? (fbb ? gp * 4u : (gp * (unsigned)CA + (unsigned)(cq * 4)) * 4u) : 0x80000000u;
        if (FB == 1) voffg[FB == 1 ? u : 0] = ok ? gp * 4u : 0x80000000u;
        bad |= (ok ? 0u : 1u) << u;
    }
    // LDS byte address of element u's hi store = lds_b + u DP LDH 2 (an instruction immediate), lo plane IH IW LDH 2 bytes further; a last element
    // that is off the tile lands in pixel 0's pad bytes (never read) instead of being branched around
    const unsigned lds_b = (unsigned)(pix0 * LDH + cq * 4) * 2u;
    const unsigned lds_last = (pix0 + (PER - 1) * DP < IH * IW) ? lds_b + (unsigned)((PER - 1) * DP * LDH) * 2u : (unsigned)CK * 2u;
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.A) + (size_t)n * AH * AW * CA), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.xf.fb_dxhat) + (size_t)n * AH * AW), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<unsigned*>(a.xf.fb_bits) + (size_t)n * AH * AW), 0, 0x80000000u, 0x00020000);
    __syncthreads();

    // The activation tile of chunk ch+1 is fetched into registers while chunk ch is contracted (the tile's two dependent
    // HBM/L2 latencies were ~60 % of a workgroup's lifetime); conversion + LDS store happen once every wave has left chunk ch.
    uint4 pf[fbb ? 1 : PER];
    float pg[fb ? PER : 1];                  // fb mode: the pixel's d objective / d x_hat, fetched with the tile
    unsigned pb[fbb ? PER : 1];              // bits mode: the pixel's activation-pattern word
    auto issue_stage = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (fbb) pb[fbb ? u : 0] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(brs, (int)voff[u], 0, 0);
            else pf[fbb ? 0 : u] = buf_load16(irs, voff[u], (unsigned)c0 * 4u);
            if (fb) pg[fb ? u : 0] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(grs, (int)(FB == 1 ? voffg[FB == 1 ? u : 0] : voff[u]), 0, 0));
        }
    };
    auto convert_stage = [&](int c0) __attribute__((always_inline)) {
        // this thread's channel quad is the same for every element (NT % CQ == 0): its table rows are read once per chunk, not once per element
        const float4 t_sc = (xf || fb) ? *reinterpret_cast<const float4*>(s_xf + c0 + cq * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 t_sh = (xf || FB == 1) ? *reinterpret_cast<const float4*>(s_xf + XF_LDS_CH + c0 + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 t_wf = fb ? *reinterpret_cast<const float4*>(s_xf + 2 * XF_LDS_CH + c0 + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const unsigned bshift = (unsigned)(c0 + cq * 4);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const uint4 q = pf[fbb ? 0 : u];
            float4 t = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
            if (fbb) {
#pragma clang fp contract(off)      // (the products are rounded before the hi | lo split subtracts from them, as when a padding select stood between the two)
                // the same from the pattern word the fused forward epilogue left: the derivative side of every channel is one bit
                const float4 sc = t_sc, wf = t_wf;
                const float g = pg[fb ? u : 0];          // padding: 0 through the descriptor's range check -> the products are zeros
                const unsigned b = pb[fbb ? u : 0] >> bshift;
                t.x = g * wf.x * ((b & 1u) ? sc.x : sc.x * a.xf.alpha);
                t.y = g * wf.y * ((b & 2u) ? sc.y : sc.y * a.xf.alpha);
                t.z = g * wf.z * ((b & 4u) ? sc.z : sc.z * a.xf.alpha);
                t.w = g * wf.w * ((b & 8u) ? sc.w : sc.w * a.xf.alpha);
            } else if (fb) {
#pragma clang fp contract(off)
                // final-backward on load: t = dxhat[pixel] * wf * lrelu'(bn(c)) * scale  (see UadXform::fb_*)
                const float4 sc = t_sc, sh = t_sh, wf = t_wf;
                const float g = pg[fb ? u : 0];
                t.x = g * wf.x * (__builtin_fmaf(t.x, sc.x, sh.x) > 0.f ? sc.x : sc.x * a.xf.alpha);
                t.y = g * wf.y * (__builtin_fmaf(t.y, sc.y, sh.y) > 0.f ? sc.y : sc.y * a.xf.alpha);
                t.z = g * wf.z * (__builtin_fmaf(t.z, sc.z, sh.z) > 0.f ? sc.z : sc.z * a.xf.alpha);
                t.w = g * wf.w * (__builtin_fmaf(t.w, sc.w, sh.w) > 0.f ? sc.w : sc.w * a.xf.alpha);
            } else if (xf) {
                t = keep4(!((bad >> u) & 1u), xform4(t, t_sc, t_sh, a.xf.alpha));      // padding is zero AFTER the activation
            }
            uint2 pl[NPL];
            split_planes<NPL>(t, pl);
            const unsigned o = (u + 1 < PER) ? lds_b + (unsigned)(u * DP * LDH) * 2u : lds_last;
#pragma unroll
            for (int p = 0; p < NPL; ++p) *reinterpret_cast<uint2*>(dsm + o + (unsigned)(p * PLANE) * 2u) = pl[p];
        }
    };
    issue_stage(ch0 * CK);
    for (int ch = ch0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        if (ch > ch0) __syncthreads();
        convert_stage(c0);
        if (ch + 1 < nchunks) issue_stage(c0 + CK);
        __syncthreads();
        loadA(a0, 0);
        const bool more = ch + 1 < nchunks;
        auto unit = [&](const KFrag<NKS, NPL>& bc, KFrag<NKS, NPL>& bpf, const KFrag<NKS, NPL>& ac, KFrag<NKS, NPL>& an, const int t) {
            if (t + 3 < 25) loadB(bpf, t + 3, c0);
            else if (more) loadB(bpf, t + 3 - 25, c0 + CK);
            if (t + 1 < 25) loadA(an, t + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NKS; ++j) {
                acc0 = mfma_bf16(ac.p[0][j], bc.p[0][j], acc0);
                acc1 = mfma_bf16(ac.p[0][j], bc.p[1][j], acc1);
                acc2 = mfma_bf16(ac.p[1][j], bc.p[0][j], acc2);
                if constexpr (NPL == 3) {      // bf16x6: + a0 w2, a2 w0, a1 w1
                    acc1 = mfma_bf16(ac.p[0][j], bc.p[2][j], acc1);
                    acc2 = mfma_bf16(ac.p[2][j], bc.p[0][j], acc2);
                    acc1 = mfma_bf16(ac.p[1][j], bc.p[1][j], acc1);
                }
            }
        };
#pragma unroll
        for (int g4 = 0; g4 < 7; ++g4) {
            if (4 * g4 + 0 < 25) unit(b0, b3, a0, a1, 4 * g4 + 0);
            if (4 * g4 + 1 < 25) unit(b1, b0, a1, a0, 4 * g4 + 1);
            if (4 * g4 + 2 < 25) unit(b2, b1, a0, a1, 4 * g4 + 2);
            if (4 * g4 + 3 < 25) unit(b3, b2, a1, a0, 4 * g4 + 3);
        }
        // 25 = 6*4 + 1: the ring advanced by one slot; rotate so the next chunk starts at slot 0 again
        b0 = b1; b1 = b2; b2 = b3;
    }

    // ---- epilogue: transpose through a wave-private LDS tile, 16-byte accesses (see conv5_d16_kernel) ----
    __syncthreads();
    constexpr int EPI_LD = 36;
    static_assert((size_t)WGM * WGN * 32 * EPI_LD * 4 <= (size_t)NPL * IH * IW * LDH * 2, "epilogue tile fits in the activation tile");
    const bool bwd = (a.ep.kind == UAD_EPI_BWD_ACT);
    float* etile = s_epi + wave * 32 * EPI_LD;
    const int ec4 = (lane & 7) * 4, erow = lane >> 3;
    const int ecol = n0 + wn * 32 + ec4;
    v16f o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = acc0[r] + (acc1[r] + acc2[r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) etile[((r & 3) + 8 * (r >> 2) + 4 * lh) * EPI_LD + l31] = o[r];
    __builtin_amdgcn_wave_barrier();
    float4 v[4];
    size_t off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = erow + 8 * k;
        v[k] = *reinterpret_cast<const float4*>(etile + row * EPI_LD + ec4);
        const int mm = wm * 32 + row;
        off[k] = ((size_t)(n * d.HS + ty0 + mm / TW) * d.WS + tx0 + mm % TW) * Nn + ecol;
    }
    float* outp = a.Out;
    if (nsplit > 1) {
        if (!a.sk_counter) {
            float* slab = a.Out + (size_t)split * a.out_elems;
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(slab + off[k]) = v[k];
            return;
        }
        const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.Out, 0, 0xffffffff, 0x00020000);
#pragma unroll
        for (int k = 0; k < 4; ++k) sk_store16(srs, (unsigned)(((size_t)split * a.out_elems + off[k]) * 4), v[k]);
        const unsigned slot = (blockIdx.y * gridDim.x + blockIdx.x) * (gridDim.z / nsplit) + blockIdx.z / nsplit;
        if (!sk_last_arriver(a.sk_counter + slot, nsplit, reinterpret_cast<int*>(s_red), tid)) return;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int sp = 0; sp < nsplit; sp += 2) {          // nsplit is a power of two >= 2; two slabs (8 loads) in flight
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
        __syncthreads();      // s_red[0] carried the flag; it is reused below
    }
    if (!bwd) {
        float4 e_a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.ep.bias) e_a = *reinterpret_cast<const float4*>(a.ep.bias + ecol);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 t = v[k];
            t.x += e_a.x; t.y += e_a.y; t.z += e_a.z; t.w += e_a.w;
            if (a.ep.mul) { const float4 q = *reinterpret_cast<const float4*>(a.ep.mul + off[k]); t.x *= q.x; t.y *= q.y; t.z *= q.z; t.w *= q.w; }
            if (a.ep.add) { const float4 q = *reinterpret_cast<const float4*>(a.ep.add + off[k]); t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w; }
            if (outp) *reinterpret_cast<float4*>(outp + off[k]) = t;
        }
        return;
    }
    float4 e_a = *reinterpret_cast<const float4*>(a.ep.escale + ecol);
    e_a.x *= a.ep.emult; e_a.y *= a.ep.emult; e_a.z *= a.ep.emult; e_a.w *= a.ep.emult;
    const float4 e_b = *reinterpret_cast<const float4*>(a.ep.eshift + ecol);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
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
        const float4 o4 = make_float4(oo[0], oo[1], oo[2], oo[3]);
        if (outp) *reinterpret_cast<float4*>(outp + off[k]) = o4;
    }
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

template <int TH, int TW, int CK, int WGM, int WGN, int NPL = 2>
constexpr size_t conv5_f16_lds_bytes() {
    return (size_t)NPL * (2 * TH + 3) * (2 * TW + 3) * (CK + 8) * 2 + (size_t)3 * XF_LDS_CH * 4 + (size_t)WGM * 2 * 32 * WGN * 4;
}

template <int TH, int TW, int CK, int WGM, int WGN, int FB, bool XF, int NPL>
void launch_conv5_f16_v(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    constexpr size_t lds = conv5_f16_lds_bytes<TH, TW, CK, WGM, WGN, NPL>();
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_f16_kernel<TH, TW, CK, WGM, WGN, FB, XF, NPL>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    UAD_SPATIAL_LAUNCH(any_order, (conv5_f16_kernel<TH, TW, CK, WGM, WGN, FB, XF, NPL>), grid, dim3(64 * WGM * WGN), lds, st, a);
}
template <int TH, int TW, int CK, int WGM, int WGN, int NPL = 2>
void launch_conv5_f16(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    if (a.xf.fb_bits || a.xf.fb_dxhat) {
        if (!a.xf.scale) { fprintf(stderr, "uad: final-backward on load needs the block's scale / shift tables\n"); abort(); }
        if (a.xf.fb_bits && a.CA > 32) { fprintf(stderr, "uad: the pattern-word form holds one bit per channel of a 32-bit word (CA = %d)\n", a.CA); abort(); }
        if (a.xf.fb_bits) launch_conv5_f16_v<TH, TW, CK, WGM, WGN, 2, true, NPL>(a, grid, any_order, st);
        else launch_conv5_f16_v<TH, TW, CK, WGM, WGN, 1, true, NPL>(a, grid, any_order, st);
    } else if (a.xf.scale) launch_conv5_f16_v<TH, TW, CK, WGM, WGN, 0, true, NPL>(a, grid, any_order, st);
    else launch_conv5_f16_v<TH, TW, CK, WGM, WGN, 0, false, NPL>(a, grid, any_order, st);
}

}  // namespace

void uad_conv5_f16_launch(const ConvGemmArgs& a, dim3 grid, int bn, bool any_order, hipStream_t st) {
    if (a.npl == 3) {      // bf16x6: 16-channel chunks in the 64-column instance too (three planes of a 32-channel 19 x 19 halo = 87 KB: one workgroup per CU)
        if (bn == 64) {
            if (a.xf.fb_bits || a.xf.fb_dxhat) { fprintf(stderr, "uad: final-backward on load runs on the 32-column instance (CA <= 32)\n"); abort(); }
            if (a.xf.scale) launch_conv5_f16_v<8, 8, 16, 2, 2, 0, true, 3>(a, grid, any_order, st); else launch_conv5_f16_v<8, 8, 16, 2, 2, 0, false, 3>(a, grid, any_order, st);
        } else launch_conv5_f16<8, 16, 16, 4, 1, 3>(a, grid, any_order, st);
    } else if (bn == 64) launch_conv5_f16<8, 8, 32, 2, 2>(a, grid, any_order, st);
    else launch_conv5_f16<8, 16, 16, 4, 1>(a, grid, any_order, st);
}

void uad_conv5_f32_launch(const ConvGemmArgs& a, dim3 grid, int bn, bool any_order, hipStream_t st) {
    if (bn == 64) UAD_SPATIAL_LAUNCH(any_order, (conv5_f_kernel<8, 8, 32, 2, 2>), grid, dim3(256), 0, st, a);
    else UAD_SPATIAL_LAUNCH(any_order, (conv5_f_kernel<8, 16, 16, 4, 1>), grid, dim3(256), 0, st, a);
}
