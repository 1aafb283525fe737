// Part of uad_gemm_d16s.hip (textually included inside its anonymous namespace; helpers: uad_gemm_common.h).
//
// Round-3 generation of the bf16x3 k5 s2 kernels: "lane = pixel".
//
// The second-generation kernels (conv5_d16_kernel / conv5_f16_kernel) run the MFMA with A = activations (rows = pixels) and
// B = weights (columns = output channels), so a lane of the 32x32 accumulator owns ONE channel of 16 pixels.  Every fused epilogue of this
// path wants the opposite -- several channels of one pixel: 16-byte NHWC stores, per-pixel dot products (the final 1x1 conv), per-pixel
// pattern words -- which is why those kernels push every accumulator tile through a wave-private LDS transpose (16 ds_write + 4 ds_read +
// 2 wave barriers + a 3-step DPP butterfly per pixel for the final conv's dot, per parity class).  The round-2 SQ counters put that
// epilogue at ~1500 of the ~2075 VALU instructions a dec3.fwd wave executes for its 150 MFMAs.
//
// Here the operands are swapped: A = weights (rows = output channels), B = activations (columns = pixels).  The fragments are the same
// registers (both are "index = lane & 31, eight consecutive k per lane"), only the order in the intrinsic changes; the accumulator then has
//      lane (l31, lh)  ->  pixel l31 of the wave's 32-pixel fragment,
//      register r      ->  channel 8 (r >> 2) + 4 lh + (r & 3)        (four groups of four CONSECUTIVE channels),
// i.e. a lane already owns 16-byte channel groups of its own pixel: stores and cprev loads are 16-byte accesses straight from the
// accumulator registers (a pixel's 32 channels = 128 contiguous bytes written by lanes l31 / l31 + 32 in four instructions), the final conv's
// dot product is 16 in-lane FMAs + ONE cross-half exchange, BN / LeakyReLU parameters are per-register values, the per-channel sums of the
// backward (dgamma, dbeta, dbias, dW_final) are per-register accumulators reduced over the lanes once per wave at the end of the kernel
// instead of once per parity class, and the s_epi transpose tile (18 KB of LDS per workgroup) is gone.

// Sum over the 32 lanes that share lh (lanes 0-31 / 32-63), DPP only (no LDS round trip: 48 serialized ds_bpermute waits were 2.6 us of a
// 15.7 us dec3.fwd workgroup): four butterfly steps leave every lane of a 16-lane row with the row's sum, row_bcast:15 adds row 0's into
// row 1 (and row 2's into row 3).  The result is valid in lanes 16-31 and 48-63 (`sum32_valid`).
__device__ __forceinline__ float sum32_half(float v) {
    v += __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v)));       // quad_perm [1,0,3,2]
    v += __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v)));       // quad_perm [2,3,0,1]
    v += __uint_as_float(dpp_u32<0x141>(__float_as_uint(v)));      // row_half_mirror
    v += __uint_as_float(dpp_u32<0x140>(__float_as_uint(v)));      // row_mirror
    v += __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1, 3
    return v;
}
__device__ __forceinline__ bool sum32_valid(int lane) { return (lane & 16) != 0; }

// value of lane L combined with the value of lane L ^ 32 (the other 16 channels of the same pixel): one v_permlane32_swap + one VALU op
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ unsigned xhalf_or(unsigned v) {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return r[0] | r[1];
}

#ifndef UAD_D16S_NACC
#define UAD_D16S_NACC 1        // 3 = the round-3 form (MF = 1 only), for A/B builds: hipcc -DUAD_D16S_NACC=3
#endif
template <int TH, int TW, int CST, int WGM, int WGN, int NPL = 2>
constexpr size_t conv5_d16s_lds_bytes(int epi) {
    return (size_t)NPL * (TH + 2) * (TW + 2) * (CST + 8) * 2      // activation halo tile, NPL bf16 planes
           + (size_t)2 * CST * 4                                  // activation-on-load tables of this workgroup's channel range
           + (size_t)4 * 32 * WGN * 4                             // epilogue parameter rows
           + (size_t)WGM * WGN * (3 * 32 + 2) * 4                 // per-wave partial sums
           + (epi == UAD_EPI_FINAL ? (size_t)5 * 4 * TH * TW * 4 : 0);
}

// MF = 32-pixel fragments per wave.  With MF = 2 a weight fragment (global -> VGPR, an L2 hit: a layer's planes exceed the L1) feeds twice
// the MFMA work: at MF = 1 the step streams 4 KB of weight fragments per 6 MFMAs and wave -- chip-wide more L2 time than MFMA time -- and the
// three products of a fragment go to ONE accumulator (the two fragments' chains interleave, so no MFMA waits for its predecessor).
template <int MF, int NPL>
struct AFrag16 { uint4 p[NPL][MF][2]; };      // NPL bf16 planes (2: bf16x3, 3: bf16x6) of MF pixel fragments, two k-octet pairs each

// (A "ping-pong" form -- two groups of waves per workgroup held one phase apart by raw s_barriers -- and start-offset ("stagger") bits were
// measured in round 3: no gain; removed, see tools/experiments/r03_pruned_opt_in_paths.patch.)
// XF: activation-on-load of the staged tile (template parameter since round 6: as a run-time flag it put a branch around every element's transform).
// GRAD (EPI_FINAL only): training pass -- pattern word, sign and the per-channel gradient sums; false = reconstruction only.
// NPL: bf16 planes per operand (2: bf16x3 products; 3: bf16x6 -- six products per K slice, fp32-grade, the VAE family's third math mode).
template <int TH, int TW, int CST, int WGM, int WGN, int MF, int EPI, bool XF, bool GRAD, int NPL = 2>
__global__ void __launch_bounds__(64 * WGM * WGN) __attribute__((amdgpu_waves_per_eu(2))) conv5_d16s_kernel(const ConvGemmArgs a) {
    constexpr int NT = 64 * WGM * WGN, NW = WGM * WGN;
    constexpr int IH = TH + 2, IW = TW + 2;
    constexpr int LDH = CST + 8;                // ushorts per pixel row (+16 B pad)
    constexpr int NCH = CST / 32, CQ = CST / 4;
    constexpr int BN = 32 * WGN;
    // accumulators per fragment.  Round 5: ONE (the three products of a unit chain into the same accumulator).  With three (round 3: "one fragment alone
    // needs independent chains") every parity class ended with 32 v_add per wave to fold them -- 128 of a wave's ~900-2000 VALU instructions in kernels whose time
    // tracks their VALU count (tools/issue_ubench.hip) -- while the SIMD's second wave already fills the matrix pipe between two dependent MFMAs of this one.
    // Three planes (bf16x6) keep TWO: the leading product in one, the five correction products in the other.  Measured per launch (tests/test_gpu_ops_spatial.py,
    // DESIGN section 23): chained into the accumulator of the leading product, the corrections left every output element ~4.5e-9 of the tensor max too low (the
    // rms error of the exact-fp32 kernel, but a one-sided mean: small products folded into a large accumulator lose their low bits in one direction), which a column
    // sum over 32768 elements turns into 3.4e-6 -- six times the exact-fp32 kernel's S1 error.  In an accumulator of their own magnitude the loss is 2^-8 of that.
    // (Three accumulators, conv5_f16_kernel's form, cure it too but do not fit under the 256 registers of two waves per SIMD: seven instances spilled.  Two fit once
    // the activation-backward epilogue stops holding its cprev prefetch through the class: PREF below.)
    constexpr int NACC = (NPL == 3 && MF == 1) ? 2 : UAD_D16S_NACC;
    constexpr int C1 = NACC > 1 ? 1 : 0, C2 = NACC == 3 ? 2 : C1;      // accumulators of the w_lo a_hi family and of the w_hi a_lo family
    constexpr bool PREF = NACC == 1;                                  // BWD: request cprev when the class starts (16 registers held through it) or at its end
    constexpr bool FIN = EPI == UAD_EPI_FINAL, BWD = EPI == UAD_EPI_BWD_ACT, PLAIN = EPI == UAD_EPI_BIAS;
    constexpr int FL = 3 * 32 + 2;              // floats of one wave's partial-sum row
    static_assert(TH * TW == 32 * MF * WGM, "MF 32-pixel fragments per wave along M");
    static_assert(CST % 32 == 0, "32-channel weight-fragment units");
    static_assert(MF == 1 || MF == 2, "one or two fragments per wave");
    static_assert(NACC == 1 || ((NACC == 2 || NACC == 3) && MF == 1), "several accumulators only with one fragment per wave");
    static_assert(!FIN || WGN == 1, "the fused final conv needs every output channel of a pixel in one wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    constexpr int PLANE = IH * IW * LDH;
    unsigned short* sPl = reinterpret_cast<unsigned short*>(dsm);          // NPL planes of IH x IW x LDH
    float* s_xf = reinterpret_cast<float*>(sPl + NPL * PLANE);             // [2][CST]
    float* s_par = s_xf + 2 * CST;                                          // [4][BN]
    float* s_red = s_par + 4 * BN;                                          // [waves][FL]
    float* s_fx = s_red + NW * FL;              // EPI_FINAL: target | reconstruction | L1 | pattern word | d objective / d x_hat of the 2TH x 2TW block
    float* s_fo = s_fx + 4 * TH * TW;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int tilesx = d.WS / TW;
    const int ty0 = (blockIdx.x / tilesx) * TH, tx0 = (blockIdx.x % tilesx) * TW;
    const int n = (int)blockIdx.y;
    const int nsplit = a.nsplit;
    const int n0 = (blockIdx.z / nsplit) * BN;
    const int split = blockIdx.z % nsplit;
    const int CA = a.CA, Nn = a.Nn;
    const int cbase = split * CST;
    const int AH = d.HS, AW = d.WS;

    constexpr bool xf = XF;

    // own pixels: fragment f of this wave = tile positions (wm MF + f) 32 + l31
    int aoff[MF], eoff00[MF], lidx00[MF];
    const int cl = wn * 32 + 4 * lh;                       // first own channel inside the column block (s_par index)
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const int m = (wm * MF + f) * 32 + l31;
        const int pty = m / TW, ptx = m % TW;
        aoff[f] = ((pty + 1) * IW + ptx + 1) * LDH + 8 * lh;
        // element offset of (own pixel of parity class (0,0), first own channel) inside the sample's [HB][WB][Nn] output
        eoff00[f] = ((2 * (ty0 + pty)) * d.WB + 2 * (tx0 + ptx)) * Nn + n0 + cl;
        lidx00[f] = (2 * pty) * (2 * TW) + 2 * ptx;        // own pixel inside the 2TH x 2TW output block (EPI_FINAL tiles)
    }
    const int col = n0 + wn * 32 + l31;
    const int colc = col < Nn ? col : 0;
    const size_t plane_q = (size_t)a.w16_plane / 8;

    // operand pipeline as in conv5_d16_kernel: weight fragments global -> a VGPR ring of four, three units ahead; activation fragments
    // LDS -> VGPR one unit ahead
    constexpr int NUNIT = 25 * NCH;
    constexpr int RING = (MF == 1 && NPL == 2) ? 4 : 3;       // weight-fragment slots: RING - 1 units ahead (a unit is 6 MF MFMAs; 12 MF in bf16x6)
    KFrag<2, NPL> bq[RING];
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.Wp16), 0, 0xffffffff, 0x00020000);
    const unsigned lb = (unsigned)(lh * Nn + colc) * 16u;
    const unsigned plane_b = (unsigned)plane_q * 16u;
    auto loadB = [&](KFrag<2, NPL>& b, int unit) __attribute__((always_inline)) {
        const int tap = kTapOrderD.tap[unit / NCH], c0 = cbase + (unit % NCH) * 32;
        const unsigned u = (unsigned)((tap * (CA / 8) + c0 / 8) * Nn) * 16u;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) b.p[p][j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u + (unsigned)p * plane_b);
    };
    auto loadA = [&](AFrag16<MF, NPL>& fr, int unit) __attribute__((always_inline)) {
        const int tap = kTapOrderD.tap[unit / NCH], kc = unit % NCH;
        const int ky = tap / 5, kx = tap % 5;
        const int py = (ky + 1) & 1, px = (kx + 1) & 1;
        const int dy = (py + 1 - ky) / 2, dx = (px + 1 - kx) / 2;
        const int toff = (dy * IW + dx) * LDH;
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int p = 0; p < NPL; ++p) fr.p[p][f][j] = *reinterpret_cast<const uint4*>(sPl + p * PLANE + aoff[f] + toff + kc * 32 + 16 * j);
    };
#pragma unroll
    for (int u = 0; u < RING - 1; ++u)
        if (u < NUNIT) loadB(bq[u], u);

    // ---- stage the whole halo tile of this workgroup's channel range ----
    // Every global load of the prologue is issued before anything waits: the tile (up to 13 x 16 bytes per thread), then the per-channel
    // tables.  In round 2's order -- tables -> barrier -> tile in batches of four -> convert -- a workgroup went through four dependent
    // memory round trips (4.6 us of a 15.7 us dec3.fwd workgroup) before its first MFMA.
    const int gy0 = ty0 - 1, gx0 = tx0 - 1;
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    constexpr int PB = PER <= 13 ? PER : (PER + 1) / 2;       // 16-byte loads in flight per thread
    constexpr int NPB = (PER + PB - 1) / PB;
    uint4 tv[PB];
    const size_t sample_q = (size_t)AH * AW * (CA / 4);
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.A) + (size_t)n * sample_q * 4), 0,
                                                                          (unsigned)(sample_q * 16), 0x00020000);
    // element j of this thread = (pixel pix0 + j DP, channel quad cq_t): the quad is the same for every element (NT % CQ == 0) and the pixel
    // coordinates advance by a compile-time step with one wrap (round 6: was two divisions by IW and one by CQ per element, in the issue AND in the
    // store pass); out-of-image pixels read through the buffer's bounds check (-> zeros); `bad` remembers them for the activated form
    constexpr int DP = NT / CQ, DIY = DP / IW, DIX = DP % IW;
    static_assert(NT % CQ == 0 && (PER - 1) * DP < IH * IW, "only a thread's LAST element can fall off the tile");
    const int cq_t = tid % CQ, pix0 = tid / CQ;
    const unsigned chan_b = (unsigned)(cbase + cq_t * 4) * 4u;
    int s_iy = pix0 / IW, s_ix = pix0 % IW;
    unsigned bad = 0;
    auto tile_issue = [&](int bt) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const int j = bt * PB + u;
            if (j >= PER) continue;
            const int gy = gy0 + s_iy, gx = gx0 + s_ix;
            const bool ok = (j + 1 < PER || pix0 + j * DP < IH * IW) && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
            const unsigned off = ok ? (unsigned)(gy * AW + gx) * (unsigned)(CA * 4) + chan_b : 0x80000000u;
            if (XF) bad |= (ok ? 0u : 1u) << j;
            tv[u] = buf_load16(irs, off, 0);
            s_ix += DIX; s_iy += DIY;
            if (s_ix >= IW) { s_ix -= IW; ++s_iy; }
        }
    };
    // LDS byte address of element j's hi store = lds_b + j DP LDH 2 (an instruction immediate); a last element that is off the tile lands in pixel 0's pad bytes
    const unsigned lds_b = (unsigned)(pix0 * LDH + cq_t * 4) * 2u;
    const unsigned lds_last = (pix0 + (PER - 1) * DP < IH * IW) ? lds_b + (unsigned)((PER - 1) * DP * LDH) * 2u : (unsigned)CST * 2u;
    auto tile_store = [&](int bt) __attribute__((always_inline)) {
        // this thread's channel quad is the same for every element: its table rows are read once, not once per element
        const float4 t_sc = xf ? *reinterpret_cast<const float4*>(s_xf + cq_t * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 t_sh = xf ? *reinterpret_cast<const float4*>(s_xf + CST + cq_t * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const int j = bt * PB + u;
            if (j >= PER) continue;
            // the producer's BN + (Leaky)ReLU on load, then the bf16 hi | lo split
            float4 t = make_float4(__uint_as_float(tv[u].x), __uint_as_float(tv[u].y), __uint_as_float(tv[u].z), __uint_as_float(tv[u].w));
            if (xf) t = keep4(!((bad >> j) & 1u), xform4(t, t_sc, t_sh, a.xf.alpha));      // padding is zero AFTER the activation
            uint2 pl[NPL];
            split_planes<NPL>(t, pl);
            const unsigned o = (j + 1 < PER) ? lds_b + (unsigned)(j * DP * LDH) * 2u : lds_last;
#pragma unroll
            for (int p = 0; p < NPL; ++p) *reinterpret_cast<uint2*>(dsm + o + (unsigned)(p * PLANE) * 2u) = pl[p];
        }
    };
    tile_issue(0);
    // per-channel tables, behind the tile loads in the memory pipeline:
    //   s_xf : activation-on-load scale | shift of this workgroup's channel range
    //   s_par: epilogue rows (per output channel of this workgroup's column block)
    //     PLAIN: bias | - | - | -
    //     BWD  : escale * emult | eshift | - | -
    //     FINAL: scale' | shift' = bias * scale' + shift | final 1x1 kernel | bias
    if (xf)
        for (int c = tid; c < CST; c += NT) {
            s_xf[c] = a.xf.scale[cbase + c] * a.xf.mult;
            s_xf[CST + c] = a.xf.shift[cbase + c];
        }
    if (tid < BN) {
        const int c = n0 + tid;
        if (PLAIN) {
            s_par[tid] = a.ep.bias ? a.ep.bias[c] : 0.f;
        } else if (BWD) {
            s_par[tid] = a.ep.escale[c] * a.ep.emult;
            s_par[BN + tid] = a.ep.eshift[c];
        } else {
            const float sc = a.ep.escale[c] * a.ep.emult, b = a.ep.bias ? a.ep.bias[c] : 0.f;
            s_par[tid] = sc;
            s_par[BN + tid] = fmaf(b, sc, a.ep.eshift[c]);
            s_par[2 * BN + tid] = a.ep.fin_wf[c];
            s_par[3 * BN + tid] = b;
        }
    }
    if (FIN)
        for (int idx = tid; idx < 4 * TH * TW; idx += NT) {
            const int yl = idx / (2 * TW), xl = idx % (2 * TW);
            s_fx[idx] = a.ep.fin_x[((size_t)n * d.HB + 2 * ty0 + yl) * d.WB + 2 * tx0 + xl];
        }
    if (xf) __syncthreads();                  // s_xf complete
#pragma unroll
    for (int bt = 0; bt < NPB; ++bt) {
        if (bt > 0) tile_issue(bt);
        tile_store(bt);
    }
    __syncthreads();

    // ---- epilogue state.  Lane (l31, lh) owns, per fragment, one pixel and its channels cg + 8 g + e (g, e < 4), cg = n0 + 32 wn + 4 lh ----
    const size_t sample_e = (size_t)d.HB * d.WB * Nn;
    const float alpha = a.ep.ealpha;
    float s1[16], s2[16], dwf[FIN ? 16 : 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) { s1[r] = 0.f; s2[r] = 0.f; }
    if (FIN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dwf[FIN ? r : 0] = 0.f;
    }
    float rec = 0.f, dbf = 0.f;
    const float f_bf = FIN ? a.ep.fin_bf[0] : 0.f;
    float4 cpre[BWD ? 4 : 1];                              // BWD: fragment 0's cprev groups of the current class, requested when the class starts
    const float* cprev_b = BWD ? a.ep.cprev + (size_t)n * sample_e : nullptr;
    constexpr bool want_grad = FIN && GRAD;
    // split launch: the slabs are private scratch, so they are laid out for the lanes, not for the image: every 16-byte store / load of a
    // wave covers 1 KB of consecutive addresses ([tile][wave][fragment][class][group][lane]); the natural NHWC layout gives 32-byte pieces,
    // which as write-through (sc1) stores cost four times the requests
    const unsigned slot = (blockIdx.y * gridDim.x + blockIdx.x) * (gridDim.z / nsplit) + blockIdx.z / nsplit;
    const unsigned sk_lane = (slot * (unsigned)(NW * MF) + (unsigned)(wave * MF)) * 4096u + (unsigned)lane * 4u;   // floats; + ((f 4 + cls) 4 + g) 256

    // tail of a parity class for one fragment: v[g] = the class's raw contraction for channel group g of the own pixel
    auto class_tail = [&](float4 (&v)[4], const int eoff, const int lidx, const float4* cp4) __attribute__((always_inline)) {
        if constexpr (PLAIN) {
            float* outb = nsplit > 1 ? a.out_final : a.Out;
            if (outb) outb += (size_t)n * sample_e;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bi = *reinterpret_cast<const float4*>(s_par + cl + 8 * g);
                float4 t = v[g];
                t.x += bi.x; t.y += bi.y; t.z += bi.z; t.w += bi.w;
                if (a.ep.mul) { const float4 q = *reinterpret_cast<const float4*>(a.ep.mul + (size_t)n * sample_e + eoff + 8 * g); t.x *= q.x; t.y *= q.y; t.z *= q.z; t.w *= q.w; }
                if (a.ep.add) { const float4 q = *reinterpret_cast<const float4*>(a.ep.add + (size_t)n * sample_e + eoff + 8 * g); t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w; }
                if (outb) *reinterpret_cast<float4*>(outb + eoff + 8 * g) = t;
            }
        } else if constexpr (BWD) {
            float* outb = (nsplit > 1 ? a.out_final : a.Out);
            if (outb) outb += (size_t)n * sample_e;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 cp = cp4[g];
                const float4 sc = *reinterpret_cast<const float4*>(s_par + cl + 8 * g);
                const float4 sh = *reinterpret_cast<const float4*>(s_par + BN + cl + 8 * g);
                const float vv[4] = {v[g].x, v[g].y, v[g].z, v[g].w}, cc[4] = {cp.x, cp.y, cp.z, cp.w};
                const float aa[4] = {sc.x, sc.y, sc.z, sc.w}, bb[4] = {sh.x, sh.y, sh.z, sh.w};
                float oo[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float bn = fmaf(aa[e], cc[e], bb[e]);
                    const float dbn = bn > 0.f ? vv[e] : vv[e] * alpha;
                    oo[e] = dbn * aa[e];
                    s1[4 * g + e] += dbn;
                    s2[4 * g + e] = fmaf(dbn, cc[e], s2[4 * g + e]);
                }
                const float4 o4 = make_float4(oo[0], oo[1], oo[2], oo[3]);
                if (outb) *reinterpret_cast<float4*>(outb + eoff + 8 * g) = o4;
            }
        } else {
            // last decoder block: BN + LeakyReLU, final 1x1 conv (C -> 1), L1 loss and, in training, the compressed loss gradient
            // (models/customlayers.py:35-37, trainers/VAE.py:36-40)
            float av[16];
            float dot = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 sc = *reinterpret_cast<const float4*>(s_par + cl + 8 * g);
                const float4 sh = *reinterpret_cast<const float4*>(s_par + BN + cl + 8 * g);
                const float4 wf = *reinterpret_cast<const float4*>(s_par + 2 * BN + cl + 8 * g);
                const float vv[4] = {v[g].x, v[g].y, v[g].z, v[g].w};
                const float aa[4] = {sc.x, sc.y, sc.z, sc.w}, bb[4] = {sh.x, sh.y, sh.z, sh.w}, ww[4] = {wf.x, wf.y, wf.z, wf.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = fmaf(vv[e], aa[e], bb[e]);          // BN of (contraction + bias): the bias is folded into shift'
                    av[4 * g + e] = fmaxf(t, t * alpha);               // LeakyReLU, 0 <= alpha <= 1 (checked by the launcher)
                    dot = fmaf(av[4 * g + e], ww[e], dot);
                }
            }
            dot = xhalf_sum(dot);                                       // + the pixel's other 16 channels
            const float xh = dot + f_bf;
            const float diff = xh - s_fx[lidx];
            const float ad = fabsf(diff);
            rec += ad;
            float sgn = 0.f;
            unsigned word = 0u;
            if (a.Out) {        // restoration pass: the TV term needs the pre-BN output once more
                float* outb = a.Out + (size_t)n * sample_e;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bi = *reinterpret_cast<const float4*>(s_par + 3 * BN + cl + 8 * g);
                    *reinterpret_cast<float4*>(outb + eoff + 8 * g) = make_float4(v[g].x + bi.x, v[g].y + bi.y, v[g].z + bi.z, v[g].w + bi.w);
                }
            }
            if constexpr (want_grad) {
                sgn = (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * a.ep.fin_inv_batch;
                const float sgna = sgn * alpha;
                dbf += sgn;
                unsigned w16 = 0u;
#pragma unroll
                for (int g = 3; g >= 0; --g) {
                    const float4 bi = *reinterpret_cast<const float4*>(s_par + 3 * BN + cl + 8 * g);
                    const float vv[4] = {v[g].x, v[g].y, v[g].z, v[g].w}, bv[4] = {bi.x, bi.y, bi.z, bi.w};
#pragma unroll
                    for (int e = 3; e >= 0; --e) {
                        const int r = 4 * g + e;
                        const bool pos = av[r] > 0.f;                    // = (BN output > 0): the activation keeps the sign
                        const float sel = pos ? sgn : sgna;             // d loss / d bn of this element = sel * w_f[channel]
                        w16 = w16 + w16 + (pos ? 1u : 0u);              // bit 4 g + e = pos
                        s1[r] += sel;
                        s2[r] = fmaf(sel, vv[e] + bv[e], s2[r]);
                        dwf[FIN ? r : 0] = fmaf(sgn, av[r], dwf[FIN ? r : 0]);
                    }
                }
                // nibble g of w16 belongs to channels 8 g + 4 lh .. + 3 of the pattern word (bit ch = BN output > 0)
                word = ((w16 & 0xFu) | ((w16 & 0xF0u) << 4) | ((w16 & 0xF00u) << 8) | ((w16 & 0xF000u) << 12)) << (4 * lh);
                word = xhalf_or(word);
            }
            // the two lanes of a pixel hold the same four per-pixel values: lane lh = 0 stores x_hat and |diff|, lh = 1 the pattern word and sign
            float* q = s_fo + lh * (2 * 4 * TH * TW) + lidx;           // s_fo | s_fl | s_fb | s_fg are adjacent
            q[0] = lh ? __uint_as_float(word) : xh;
            q[4 * TH * TW] = lh ? sgn : ad;
        }
    };

    auto class_epilogue = [&](v16f (&acc)[MF][NACC], const int py, const int px) __attribute__((always_inline)) {
        const int coff = (py * d.WB + px) * Nn;
        float4 cnext[BWD ? 4 : 1];
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            float4 v[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if constexpr (NACC == 2) {
                    v[g].x = acc[f][0][4 * g + 0] + acc[f][1][4 * g + 0];
                    v[g].y = acc[f][0][4 * g + 1] + acc[f][1][4 * g + 1];
                    v[g].z = acc[f][0][4 * g + 2] + acc[f][1][4 * g + 2];
                    v[g].w = acc[f][0][4 * g + 3] + acc[f][1][4 * g + 3];
                } else if constexpr (NACC == 3) {
                    v[g].x = acc[f][0][4 * g + 0] + (acc[f][1][4 * g + 0] + acc[f][2][4 * g + 0]);
                    v[g].y = acc[f][0][4 * g + 1] + (acc[f][1][4 * g + 1] + acc[f][2][4 * g + 1]);
                    v[g].z = acc[f][0][4 * g + 2] + (acc[f][1][4 * g + 2] + acc[f][2][4 * g + 2]);
                    v[g].w = acc[f][0][4 * g + 3] + (acc[f][1][4 * g + 3] + acc[f][2][4 * g + 3]);
                } else {
                    v[g] = make_float4(acc[f][0][4 * g + 0], acc[f][0][4 * g + 1], acc[f][0][4 * g + 2], acc[f][0][4 * g + 3]);
                }
            }
            const int eoff = eoff00[f] + coff;
            if (nsplit > 1) {
                // raw partial tile -> this split's slab; the tile's last workgroup sums the slabs below
                const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.Out, 0, 0xffffffff, 0x00020000);
                const unsigned base = (unsigned)((size_t)split * a.out_elems) + sk_lane + (unsigned)((f * 4 + py * 2 + px) * 4) * 256u;
#pragma unroll
                for (int g = 0; g < 4; ++g) sk_store16(srs, (base + (unsigned)g * 256u) * 4u, v[g]);
                continue;
            }
            if constexpr (BWD) {
                // fragment 0's cprev groups were requested when the class started; the next fragment's are requested now, before this one is processed
                if constexpr (MF > 1) {
                    if (f + 1 < MF) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) cnext[g] = *reinterpret_cast<const float4*>(cprev_b + eoff00[f + 1 < MF ? f + 1 : f] + coff + 8 * g);
                    }
                }
                if constexpr (!PREF) {
                    if (f == 0) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) cpre[BWD ? g : 0] = *reinterpret_cast<const float4*>(cprev_b + eoff + 8 * g);
                    }
                }
                if (f == 0) class_tail(v, eoff, 0, cpre);
                else class_tail(v, eoff, 0, cnext);
            } else {
                class_tail(v, eoff, lidx00[f] + py * (2 * TW) + px, nullptr);
            }
        }
    };

    // ---- the unit sequence, expanded at compile time ----
    v16f acc[MF][NACC];
    AFrag16<MF, NPL> aq[2];
    loadA(aq[0], 0);
    auto unit = [&](auto S) __attribute__((always_inline)) {
        constexpr int sidx = decltype(S)::value;
        const KFrag<2, NPL>& bc = bq[sidx % RING];
        KFrag<2, NPL>& bpf = bq[(sidx + RING - 1) % RING];
        const AFrag16<MF, NPL>& ac = aq[sidx % 2];
        AFrag16<MF, NPL>& an = aq[(sidx + 1) % 2];
        constexpr int t = sidx / NCH, kc = sidx % NCH;
        constexpr int tap = kTapOrderD.tap[t];
        constexpr int ky = tap / 5, kx = tap % 5;
        constexpr int py = (ky + 1) & 1, px = (kx + 1) & 1;
        constexpr int cls = py * 2 + px;
        constexpr bool first = (kc == 0 && t == kTapOrderD.start[cls]);
        constexpr bool last = (kc == NCH - 1 && t + 1 == kTapOrderD.start[cls + 1]);
        if constexpr (sidx + RING - 1 < NUNIT) loadB(bpf, sidx + RING - 1);
        if constexpr (sidx + 1 < NUNIT) loadA(an, sidx + 1);
        if constexpr (BWD && first && PREF) {
            if (nsplit == 1) {
                const int eoff = eoff00[0] + (py * d.WB + px) * Nn;
#pragma unroll
                for (int g = 0; g < 4; ++g) cpre[BWD ? g : 0] = *reinterpret_cast<const float4*>(cprev_b + eoff + 8 * g);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // A = weights (rows = output channels), B = activations (columns = pixels).  Products: w_hi a_hi, w_lo a_hi, w_hi a_lo.
        const v16f z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int f = 0; f < MF; ++f) acc[f][0] = mfma_bf16(bc.p[0][j], ac.p[0][f][j], (first && j == 0) ? z : acc[f][0]);
#pragma unroll
            for (int f = 0; f < MF; ++f) acc[f][C1] = mfma_bf16(bc.p[1][j], ac.p[0][f][j], (first && j == 0 && NACC > 1) ? z : acc[f][C1]);
#pragma unroll
            for (int f = 0; f < MF; ++f) acc[f][C2] = mfma_bf16(bc.p[0][j], ac.p[1][f][j], (first && j == 0 && NACC == 3) ? z : acc[f][C2]);
            if constexpr (NPL == 3) {      // bf16x6: + w2 a0, w0 a2, w1 a1
#pragma unroll
                for (int f = 0; f < MF; ++f) acc[f][C1] = mfma_bf16(bc.p[2][j], ac.p[0][f][j], acc[f][C1]);
#pragma unroll
                for (int f = 0; f < MF; ++f) acc[f][C2] = mfma_bf16(bc.p[0][j], ac.p[2][f][j], acc[f][C2]);
#pragma unroll
                for (int f = 0; f < MF; ++f) acc[f][C1] = mfma_bf16(bc.p[1][j], ac.p[1][f][j], acc[f][C1]);
            }
        }
        if constexpr (last) {
            class_epilogue(acc, py, px);
        }
    };
    static_for<0, NUNIT>([&](auto S) __attribute__((always_inline)) { unit(S); });

    if (nsplit > 1) {
        if (!sk_last_arriver(a.sk_counter + slot, nsplit, reinterpret_cast<int*>(s_red), tid)) return;
        const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.Out, 0, 0xffffffff, 0x00020000);
#pragma unroll 1
        for (int fc = 0; fc < MF * 4; ++fc) {
            const int f = fc >> 2, py = (fc >> 1) & 1, px = fc & 1;
            const int eoff = (MF == 1 ? eoff00[0] : (f ? eoff00[MF - 1] : eoff00[0])) + (py * d.WB + px) * Nn;
            float4 v[4], cp[BWD ? 4 : 1];
            if constexpr (BWD) {
#pragma unroll
                for (int g = 0; g < 4; ++g) cp[g] = *reinterpret_cast<const float4*>(cprev_b + eoff + 8 * g);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) v[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            const unsigned base = sk_lane + (unsigned)(fc * 4) * 256u;
            for (int sp = 0; sp < nsplit; sp += 2) {          // split order, two slabs in flight
                float4 t[4][2];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int h = 0; h < 2; ++h) t[g][h] = sk_load16(srs, ((unsigned)((size_t)(sp + h) * a.out_elems) + base + (unsigned)g * 256u) * 4u);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int h = 0; h < 2; ++h) { v[g].x += t[g][h].x; v[g].y += t[g][h].y; v[g].z += t[g][h].z; v[g].w += t[g][h].w; }
            }
            class_tail(v, eoff, (MF == 1 ? lidx00[0] : (f ? lidx00[MF - 1] : lidx00[0])) + py * (2 * TW) + px, cp);
        }
        __syncthreads();                      // s_red[0] carried the ticket flag; it is reused below
    }

    if constexpr (FIN) {
        // workgroup partials in the final kernel's layout: red_partial[tile][3C+1] = {dwf[C], S1[C], S2[C], dbf}, rec_partial[tile]
        __syncthreads();
        float* s_fl = s_fo + 4 * TH * TW;
        const unsigned* s_fb = reinterpret_cast<const unsigned*>(s_fl + 4 * TH * TW);
        const float* s_fg = s_fl + 2 * 4 * TH * TW;
        for (int idx = tid; idx < 4 * TH * TW; idx += NT) {
            const int yl = idx / (2 * TW), xl = idx % (2 * TW);
            const size_t pix = ((size_t)n * d.HB + 2 * ty0 + yl) * d.WB + 2 * tx0 + xl;
            a.ep.fin_xhat[pix] = s_fo[idx];
            if (a.ep.fin_l1) a.ep.fin_l1[pix] = s_fl[idx];
            if (a.ep.fin_bits) { a.ep.fin_bits[pix] = s_fb[idx]; a.ep.fin_dxhat[pix] = s_fg[idx]; }
        }
        float* fr = s_red + wave * FL;
        if constexpr (want_grad) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t0 = sum32_half(dwf[FIN ? r : 0]), t1 = sum32_half(s1[r]), t2 = sum32_half(s2[r]);
                if (l31 == 16) {
                    const int c = 8 * (r >> 2) + 4 * lh + (r & 3);
                    const float wfc = s_par[2 * BN + c];
                    fr[c] = t0;                       // d loss / d w_f
                    fr[32 + c] = wfc * t1;            // S1 = sum d bn
                    fr[64 + c] = wfc * t2;            // S2 = sum d bn * c
                }
            }
        }
        float r0 = rec, r1 = dbf;
        r0 = sum32_half(r0); r1 = sum32_half(r1);     // both halves of a pixel carry the same value: use lh = 0
        if (lane == 16) { fr[96] = r1; fr[97] = r0; }
        __syncthreads();
        // the partial arrays are laid out for 8 x 16 tiles ([sample][HS / 8][WS / 16]: what their consumers sum over); a 16 x 16 workgroup writes its sums
        // into its upper half's slot and zeros into the lower half's
        static_assert(TW == 16 && (TH == 8 || TH == 16), "partial-sum slots of the fused final epilogue are 8 x 16 tiles");
        const int slots_x = d.WS / 16;
        const size_t tile = ((size_t)n * (d.HS / 8) + ty0 / 8) * slots_x + tx0 / 16;
        if (tid < FL) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += s_red[w * FL + tid];
            if (tid == 97) a.ep.fin_rec_partial[tile] = t;
            else if (want_grad) a.ep.fin_red_partial[tile * 97 + tid] = t;
            if constexpr (TH == 16) {
                if (tid == 97) a.ep.fin_rec_partial[tile + slots_x] = 0.f;
                else if (want_grad) a.ep.fin_red_partial[(tile + slots_x) * 97 + tid] = 0.f;
            }
        }
        return;
    }
    if constexpr (BWD) {
        float* fr = s_red + wave * FL;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float t1 = sum32_half(s1[r]), t2 = sum32_half(s2[r]);
            if (l31 == 16) {
                const int c = 8 * (r >> 2) + 4 * lh + (r & 3);
                fr[c] = t1;
                fr[32 + c] = t2;
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, c = tid % BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) t += s_red[(w * WGN + c / 32) * FL + which * 32 + (c & 31)];
            const size_t tile = (size_t)n * gridDim.x + blockIdx.x;
            if (n0 + c < Nn) a.ep.colpart[(tile * 2 + which) * Nn + n0 + c] = t;
        }
    }
}

template <int TH, int TW, int CST, int WGM, int WGN, int MF, int EPI, bool XF, bool GRAD, int NPL>
void launch_conv5_d16s_e(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    constexpr size_t lds = conv5_d16s_lds_bytes<TH, TW, CST, WGM, WGN, NPL>(EPI);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_d16s_kernel<TH, TW, CST, WGM, WGN, MF, EPI, XF, GRAD, NPL>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    UAD_SPATIAL_LAUNCH(any_order, (conv5_d16s_kernel<TH, TW, CST, WGM, WGN, MF, EPI, XF, GRAD, NPL>), grid, dim3(64 * WGM * WGN), lds, st, a);
}
// true when the lane = pixel kernel takes this launch (else: conv5_d16_kernel).  Instantiated (each instance is a fully unrolled 25 x CST / 32-unit kernel;
// round 6 halved the list for compile time): plain epilogue WITH activation-on-load (every decoder block of the model reads its producer's BN), backward
// epilogue WITHOUT (the gradient stream is plain), the fused final epilogue with it.  The other two combinations -- op-level calls -- run on conv5_d16_kernel.
inline bool conv5_d16s_takes(const ConvGemmArgs& a) {
    static const bool off = getenv("UAD_NO_D16S") != nullptr;
    if (off) return false;
    if (a.Nn % 32) return false;
    if (a.nsplit > 1 && !a.sk_counter) return false;        // its slab layout is private: the reducer is the kernel's own last workgroup
    const bool xf = a.xf.scale != nullptr;
    if (a.ep.kind == UAD_EPI_FINAL) return a.ep.fin_dc == nullptr && a.ep.ealpha >= 0.f && a.ep.ealpha <= 1.f && xf;
    if (a.ep.kind == UAD_EPI_BWD_ACT) return !xf;
    return xf;
}
// the fused final's training form on 16 x 16 tiles (the two-plane 8 x 16 instance with a 32-channel range asks; uad_op_conv_plan reports the answer)
inline bool conv5_d16s_t16(const ConvGemmArgs& a) {
    static const bool t16 = getenv("UAD_NO_D16S_T16") == nullptr;
    return t16 && a.ep.fin_bits && a.nsplit == 1 && a.d.HS % 16 == 0;
}
template <int TH, int TW, int CST, int WGM, int WGN, int MF, int NPL>
void launch_conv5_d16s_n(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    if (a.ep.kind == UAD_EPI_BWD_ACT) launch_conv5_d16s_e<TH, TW, CST, WGM, WGN, MF, UAD_EPI_BWD_ACT, false, false, NPL>(a, grid, any_order, st);
    else if (a.ep.kind == UAD_EPI_FINAL) {
        if constexpr (WGN == 1) {
            // round 6 (late): the training instance of the 32-channel last block on 16 x 16 tiles, two pixel fragments per wave -- half the workgroups, a weight
            // fragment feeds two MFMA chains, 27 % instead of 41 % halo overhead in the staged tile: dec3.fwd 67.8 -> 62.2 us same box.  UAD_NO_D16S_T16: 8 x 16.
            if constexpr (TH == 8 && TW == 16 && CST == 32 && WGM == 4 && MF == 1 && NPL == 2) {
                if (conv5_d16s_t16(a)) {
                    grid.x = (a.d.HS / 16) * (a.d.WS / 16);
                    launch_conv5_d16s_e<16, 16, 32, 4, 1, 2, UAD_EPI_FINAL, true, true, 2>(a, grid, any_order, st);
                    return;
                }
            }
            if (a.ep.fin_bits) launch_conv5_d16s_e<TH, TW, CST, WGM, WGN, MF, UAD_EPI_FINAL, true, true, NPL>(a, grid, any_order, st);
            else launch_conv5_d16s_e<TH, TW, CST, WGM, WGN, MF, UAD_EPI_FINAL, true, false, NPL>(a, grid, any_order, st);
        }
    } else launch_conv5_d16s_e<TH, TW, CST, WGM, WGN, MF, UAD_EPI_BIAS, true, false, NPL>(a, grid, any_order, st);
}
template <int TH, int TW, int CST, int WGM, int WGN, int MF>
void launch_conv5_d16s(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    launch_conv5_d16s_n<TH, TW, CST, WGM, WGN, MF, UAD_D16S_NPL>(a, grid, any_order, st);      // one plane count per translation unit (uad_gemm_d16s.hip / uad_gemm_d16s3.hip)
}
// tile 8 x 16 (32 output channels per workgroup) / 8 x 8 (64)
template <int CST>
void launch_conv5_d16s_bn32(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    launch_conv5_d16s<8, 16, CST, 4, 1, 1>(a, grid, any_order, st);       // (MF = 2 with half the waves measured slower on every layer: profiles/README.md, round 3)
}
template <int CST>
void launch_conv5_d16s_bn64(const ConvGemmArgs& a, dim3 grid, bool any_order, hipStream_t st) {
    launch_conv5_d16s<8, 8, CST, 2, 2, 1>(a, grid, any_order, st);
}
