// Part of uad_conv_k3.hip (textually included inside its anonymous namespace; argument block, choosers and tap lists: uad_conv_launch.h, uad_conv_k3_plan.h).
//
// Round 4: "tap-list" bf16x3 spatial kernel for the k3 contractions of the ResNet f-AnoGAN graph (models/fanogan_schlegl.py:31-55,70-94:
// Conv2D k3 s1 / s2, Conv2DTranspose k3 s1 / s2 at 64-512 channels) -- until now on the generic per-tap-gather fp32 kernels.
//
// One kernel shape covers every data-path contraction of those layers.  A launch walks an ITERATION GRID of MH x MW positions per sample;
// iteration (y, x) reads the input pixels (SIN y + y0 + hy_t, SIN x + x0 + hx_t) of a short tap list t < NTAPS and writes the output pixel
// (os y + oy, os x + ox):
//   Conv2D k3 s1 forward / its adjoint-pass forms (F, 3,1,1): grid = output, SIN 1, 9 taps at halo offsets (ky, kx), origin -1
//   Conv2D k3 s2 forward, ConvT k3 s2 data gradient (F, 3,2,0): grid = small image, SIN 2, 9 taps at (ky, kx), origin 0
//   Conv2D k3 s1 data gradient, ConvT k3 s1 forward (D, 3,1,1): grid = big image, SIN 1, 9 taps at (2 - ky, 2 - kx), origin -1, D-packed weights
//   ConvT k3 s2 forward, Conv2D k3 s2 data gradient (D, 3,2,0): one launch per output-parity class (py, px) -- 4 / 2 / 2 / 1 taps, grid = small
//   image, os 2, (oy, ox) = (py, px): big(2 i + ky) <-> small(i), so an even big row takes ky 0 (small row i) and ky 2 (row i - 1), an odd one ky 1.
// Structure as conv5_f16_kernel (halo tile of one 32-channel chunk staged in LDS as bf16 hi | lo planes, the next chunk's tile fetched into
// registers while this one is contracted, every tap contracted from LDS, weight fragments global -> a four-deep VGPR ring three units ahead
// through the chunk boundary, activation fragments LDS -> VGPR one tap ahead), with the OPERAND ORDER of the lane = pixel kernel
// (uad_conv16s.inc): A = weights, B = activations, so a lane's accumulator registers are 4 x 4 consecutive channels of its own pixel and the
// epilogue (bias + optional addend: the residual stream) stores 16 bytes per instruction straight from the registers, no LDS transpose.
// Identity activation on load (the ResNet graph materialises its LayerNorm + ReLU outputs: they are the filter-gradient operands too).
//
// NPL = 3 ("bf16x6"): fp32-grade products for the passes that must not carry bf16x3's ~2^-18 relative round-off (g_conv_f / g_conv_d in
// uad_gan.hip: the penalty-value passes, the generator / encoder phases).  Both operands are split THREE ways, x = h + m + l with h = bf16(x),
// m = bf16(x - h), l = bf16(x - h - m) (|x - h - m - l| <= 2^-27 |x|), and a product keeps the six terms down to 2^-18: h h', h m', m h', h l', l h',
// m m' -- the dropped m l', l m', l l' are <= 2^-26 |x x'|, below fp32's own rounding -- on six 32-cycle bf16 MFMAs per K = 16 instead of eight
// 64-cycle fp32 MFMAs (192 vs 512 matrix-pipe cycles), fp32 accumulation as the exact-fp32 kernels have it.

// (KFrag<NKS, NPL> and split_planes<NPL> live in uad_gemm_common.h: the k5 kernels use them too since round 6)
#ifndef K3_ABL
#define K3_ABL 0          // tools/k3_ubench.hip: kernel-tuning ablations (results are wrong): 1 no weight loads in the loop | 2 no LDS fragment reads | 4 no staging | 8 no MFMAs | 16 no barrier
#endif
template <int TH, int TW, int CK, int WGM, int WGN, int SIN, int EXT, int NTAPS, int NPL, bool TPF>
__global__ void __launch_bounds__(64 * WGM * WGN) __attribute__((amdgpu_waves_per_eu(2))) convk16_kernel(const ConvKArgs a) {
    // NPL: bf16 planes per operand (2: bf16x3 products, 3: bf16x6); TPF: the next chunk's tile is fetched into registers while this one is contracted
    constexpr int RING = NPL == 3 ? 3 : 4;            // weight-fragment slots: RING - 1 units ahead
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = SIN * (TH - 1) + EXT + 1, IW = SIN * (TW - 1) + EXT + 1;
    constexpr int LDH = CK + 8;
    constexpr int NKS = CK / 16, CQ = CK / 4;
    constexpr int BN = 32 * WGN;
    static_assert(TH * TW == 32 * WGM, "one 32-pixel fragment per wave along M");
    static_assert(NT % CQ == 0, "a thread's channel quad is the same for every element it stages");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* sPl = reinterpret_cast<unsigned short*>(dsm);      // NPL planes of IH x IW x LDH
    constexpr int PLANE = IH * IW * LDH;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int l31 = lane & 31, lh = lane >> 5;
    const int tilesx = a.MW / TW;
    const int ty0 = (blockIdx.x / tilesx) * TH, tx0 = (blockIdx.x % tilesx) * TW;
    const int n = blockIdx.y;
    const int n0 = blockIdx.z * BN;
    const int CA = a.CA, Nn = a.Nn, AH = a.AH, AW = a.AW;

    const int mpix = wm * 32 + l31;
    const int pty = mpix / TW, ptx = mpix % TW;
    const int aoff = ((SIN * pty) * IW + SIN * ptx) * LDH + 8 * lh;
    const int col = n0 + wn * 32 + l31;

    // weight fragments (MFMA operand A: rows = output channels): lane l31 = channel, eight consecutive k per lane, k-octet 2 j + lh of the chunk
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.Wp16), 0, 0xffffffff, 0x00020000);
    const unsigned lb = (unsigned)(lh * Nn + col) * 16u;
    const unsigned plane_b = (unsigned)((size_t)a.w16_plane / 8) * 16u;
    auto loadB = [&](KFrag<NKS, NPL>& b, const int tap, const int c0) __attribute__((always_inline)) {
        const unsigned u = (unsigned)((a.widx[tap] * (CA / 8) + c0 / 8) * Nn) * 16u;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) b.p[p][j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u + (unsigned)p * plane_b);
    };
    auto loadA = [&](KFrag<NKS, NPL>& f, const int tap) __attribute__((always_inline)) {
        const int toff = a.toff[tap] * LDH;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) f.p[p][j] = *reinterpret_cast<const uint4*>(sPl + p * PLANE + aoff + toff + 16 * j);
    };

    const int nchunks = CA / CK;
    KFrag<NKS, NPL> bq[RING], aq[2];
    // ring prologue: units 0 .. RING - 2 (unit u = tap u % NTAPS of chunk u / NTAPS)
    static_for<0, RING - 1>([&](auto U) __attribute__((always_inline)) {
        constexpr int u = decltype(U)::value;
        if (u / NTAPS < nchunks) loadB(bq[u], u % NTAPS, (u / NTAPS) * CK);
    });

    v16f acc0, acc1, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; acc2[r] = 0.f; }

    // ---- staging: element f of the tile = (pixel f / CQ, channel quad f % CQ); out-of-image pixels read through the buffer's bounds check ----
    const int gy0 = SIN * ty0 + a.y0, gx0 = SIN * tx0 + a.x0;
    const size_t sample_b = (size_t)AH * AW * CA * 4;
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.A) + (size_t)n * AH * AW * CA), 0,
                                                                          (unsigned)sample_b, 0x00020000);
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    uint4 pf[PER];
    const int cq_t = tid % CQ;
    auto issue_stage = [&](const int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int f = tid + u * NT;
            const int pix = f / CQ;
            const int iy = pix / IW, ix = pix % IW;
            const int gy = gy0 + iy, gx = gx0 + ix;
            const bool ok = (f < TOT) && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
            const unsigned off = ok ? (unsigned)(((gy * AW + gx) * CA + c0 + cq_t * 4) * 4) : 0x80000000u;
            pf[u] = buf_load16(irs, off, 0);
        }
    };
    auto convert_stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int f = tid + u * NT;
            if (f >= TOT) continue;
            const int pix = f / CQ;
            const float4 t = make_float4(__uint_as_float(pf[u].x), __uint_as_float(pf[u].y), __uint_as_float(pf[u].z), __uint_as_float(pf[u].w));
            uint2 pl[NPL];
            split_planes<NPL>(t, pl);
#pragma unroll
            for (int p = 0; p < NPL; ++p) *reinterpret_cast<uint2*>(sPl + p * PLANE + pix * LDH + cq_t * 4) = pl[p];
        }
    };

    if (TPF) issue_stage(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        if (ch > 0) __syncthreads();              // every wave is done with the previous chunk's tile
        if (!(K3_ABL & 4) || ch == 0) {
        if (!TPF) issue_stage(c0);
        convert_stage();
        if (TPF && ch + 1 < nchunks) issue_stage(c0 + CK);
        }
        __syncthreads();
        loadA(aq[0], 0);
        static_for<0, NTAPS>([&](auto T) __attribute__((always_inline)) {
            constexpr int t = decltype(T)::value;
            const KFrag<NKS, NPL>& bc = bq[t % RING];
            KFrag<NKS, NPL>& bpf = bq[(t + RING - 1) % RING];
            const KFrag<NKS, NPL>& ac = aq[t % 2];
            constexpr int up = t + RING - 1;      // the unit RING - 1 ahead: tap up % NTAPS of chunk ch + up / NTAPS
            if (!(K3_ABL & 1)) if (ch + up / NTAPS < nchunks) loadB(bpf, up % NTAPS, c0 + (up / NTAPS) * CK);
            if (!(K3_ABL & 2)) if constexpr (t + 1 < NTAPS) loadA(aq[(t + 1) % 2], t + 1);
            __builtin_amdgcn_sched_barrier(0);
            // A = weights (rows = output channels), B = activations (columns = pixels).  bf16x3: w0 a0 | w1 a0 | w0 a1; bf16x6 adds w2 a0, w0 a2, w1 a1.
            if (!(K3_ABL & 8))
#pragma unroll
            for (int j = 0; j < NKS; ++j) {
                acc0 = mfma_bf16(bc.p[0][j], ac.p[0][j], acc0);
                acc1 = mfma_bf16(bc.p[1][j], ac.p[0][j], acc1);
                acc2 = mfma_bf16(bc.p[0][j], ac.p[1][j], acc2);
                if constexpr (NPL == 3) {
                    acc1 = mfma_bf16(bc.p[2][j], ac.p[0][j], acc1);
                    acc2 = mfma_bf16(bc.p[0][j], ac.p[2][j], acc2);
                    acc1 = mfma_bf16(bc.p[1][j], ac.p[1][j], acc1);
                }
            }
        });
        // the ring advanced by NTAPS slots: rotate so that the next chunk's first unit sits in slot 0 again (NTAPS % RING == 0: nothing to move)
        if constexpr (NTAPS % RING != 0) {
            constexpr int r = NTAPS % RING;
            KFrag<NKS, NPL> tmp[RING - 1];
#pragma unroll
            for (int i = 0; i < RING - 1; ++i) tmp[i] = bq[(i + r) % RING];
#pragma unroll
            for (int i = 0; i < RING - 1; ++i) bq[i] = tmp[i];
        }
    }

    // ---- epilogue: lane (l31, lh) owns pixel l31 of the wave's fragment and its channels n0 + 32 wn + 8 g + 4 lh + e (g, e < 4) ----
    const int oyp = a.os * (ty0 + pty) + a.oy, oxp = a.os * (tx0 + ptx) + a.ox;
    const size_t obase = (((size_t)n * a.OH + oyp) * a.OW + oxp) * Nn + n0 + wn * 32 + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float4 v;
        v.x = acc0[4 * g + 0] + (acc1[4 * g + 0] + acc2[4 * g + 0]);
        v.y = acc0[4 * g + 1] + (acc1[4 * g + 1] + acc2[4 * g + 1]);
        v.z = acc0[4 * g + 2] + (acc1[4 * g + 2] + acc2[4 * g + 2]);
        v.w = acc0[4 * g + 3] + (acc1[4 * g + 3] + acc2[4 * g + 3]);
        if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n0 + wn * 32 + 4 * lh + 8 * g); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
        if (a.add) { const float4 q = *reinterpret_cast<const float4*>(a.add + obase + 8 * g); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
        *reinterpret_cast<float4*>(a.Out + obase + 8 * g) = v;
    }
}

// XCD-aware workgroup renaming (guide T1): the dispatcher hands consecutive workgroup ids to the eight XCDs in turn, so in dispatch order every XCD's L2
// sees every output-channel block's weight slice (9.4 MB at 512 x 512 channels against 4 MB of L2: the fragment loads of the dominant shape fetched the
// tensor once per XCD, 75 of its 126 MB of counter traffic).  Renamed, XCD k works through ONE contiguous eighth of the (tile, sample, channel-block) order:
// one or two channel blocks per XCD, their weight slices L2-resident.  A bijection for any workgroup count; results do not depend on it.
#ifndef K3_NOSWZ
#define K3_NOSWZ 0
#endif
__device__ __forceinline__ void xcd_block(unsigned& bx, unsigned& by, unsigned& bz) {
    bx = blockIdx.x; by = blockIdx.y; bz = blockIdx.z;
    if (K3_NOSWZ) return;
    const unsigned gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * gridDim.z;
    const unsigned bid = bx + gx * (by + gy * bz);
    const unsigned q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    const unsigned L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
    bx = L % gx; by = (L / gx) % gy; bz = L / (gx * gy);
}

// Round 6: the same contraction with a PIPELINED chunk loop (same tile, same fragments, same summation order: bit-identical outputs).  The micro-benchmark
// (tools/k3_ubench.hip, profiles/r06_g_k3_ablations.md) put the first kernel's matrix-pipe share at 0.33 with every other phase ADDING to the MFMA time
// rather than hiding under it: two barriers per 32-channel chunk with the convert pass between them, exec-masked staging branches that made the compiler's
// vmcnt bookkeeping conservative, all of a unit's memory instructions issued in one clump ahead of its MFMAs, and 212 VGPRs (two workgroups per CU: 768
// workgroups of the dominant shape = 1.5 rounds).  Here: the halo tile is DOUBLE-BUFFERED in LDS -- chunk c + 1 is converted into the other buffer in the
// middle of chunk c's MFMA phase, the global loads of chunk c + 2 follow it, ONE barrier per chunk; the chunk body is straight-line code (tile elements past
// the halo go to a dump slot, loads past the last chunk re-load an in-range chunk); a three-slot weight ring (NTAPS % RING == 0: no rotation copies, 164 VGPRs
// -> three workgroups per CU); per unit one weight-fragment load and one activation-fragment read are scheduled behind each MFMA (sched_group_barrier).
template <int TH, int TW, int CK, int WGM, int WGN, int SIN, int EXT, int NTAPS, int NPL>
__global__ void __launch_bounds__(64 * WGM * WGN) convk16p_kernel(const ConvKArgs a) {
    constexpr int RING = NTAPS % 3 == 0 ? 3 : (NTAPS % 4 == 0 ? 4 : 2);
    static_assert(NTAPS % RING == 0 || NTAPS == 1, "the ring returns to slot 0 at every chunk boundary (one tap: a two-slot ring, one fragment copy per chunk)");
    constexpr int NT = 64 * WGM * WGN;
    constexpr int IH = SIN * (TH - 1) + EXT + 1, IW = SIN * (TW - 1) + EXT + 1;
    constexpr int LDH = CK + 8;
    constexpr int NKS = CK / 16, CQ = CK / 4;
    constexpr int BN = 32 * WGN;
    static_assert(TH * TW == 32 * WGM, "one 32-pixel fragment per wave along M");
    static_assert(NT % CQ == 0, "a thread's channel quad is the same for every element it stages");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* sPl = reinterpret_cast<unsigned short*>(dsm);      // two buffers of NPL planes of IH x IW x LDH, then the dump slot
    constexpr int PLANE = IH * IW * LDH, BUF = NPL * PLANE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int l31 = lane & 31, lh = lane >> 5;
    const int tilesx = a.MW / TW;
    unsigned bx, by, bz;
    xcd_block(bx, by, bz);
    const int ty0 = ((int)bx / tilesx) * TH, tx0 = ((int)bx % tilesx) * TW;
    const int n = (int)by;
    const int n0 = (int)bz * BN;
    const int CA = a.CA, Nn = a.Nn, AH = a.AH, AW = a.AW;

    const int mpix = wm * 32 + l31;
    const int pty = mpix / TW, ptx = mpix % TW;
    const int aoff = ((SIN * pty) * IW + SIN * ptx) * LDH + 8 * lh;
    const int col = n0 + wn * 32 + l31;

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.Wp16), 0, 0xffffffff, 0x00020000);
    const unsigned lb = (unsigned)(lh * Nn + col) * 16u;
    const unsigned plane_b = (unsigned)((size_t)a.w16_plane / 8) * 16u;
    auto loadB = [&](KFrag<NKS, NPL>& b, const int tap, const int c0) __attribute__((always_inline)) {
        const unsigned u = (unsigned)((a.widx[tap] * (CA / 8) + c0 / 8) * Nn) * 16u;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) b.p[p][j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u + (unsigned)p * plane_b);
    };
    auto loadA = [&](KFrag<NKS, NPL>& f, const int tap, const int buf) __attribute__((always_inline)) {
        const int o = buf + aoff + a.toff[tap] * LDH;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) f.p[p][j] = *reinterpret_cast<const uint4*>(sPl + o + p * PLANE + 16 * j);
    };

    const int nchunks = CA / CK;
    KFrag<NKS, NPL> bq[RING], aq[2];
    static_for<0, RING - 1>([&](auto U) __attribute__((always_inline)) {
        constexpr int u = decltype(U)::value;
        loadB(bq[u], u % NTAPS, (u / NTAPS < nchunks) ? (u / NTAPS) * CK : 0);
    });

    v16f acc0, acc1, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; acc2[r] = 0.f; }

    // ---- staging: element f of the tile = (pixel f / CQ, channel quad f % CQ); out-of-image pixels read through the buffer's bounds check ----
    const int gy0 = SIN * ty0 + a.y0, gx0 = SIN * tx0 + a.x0;
    const size_t sample_b = (size_t)AH * AW * CA * 4;
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.A) + (size_t)n * AH * AW * CA), 0,
                                                                          (unsigned)sample_b, 0x00020000);
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    uint4 pf[PER];
    unsigned goff[PER];          // byte offset of the element's channel quad in chunk 0 (2^31: outside the image or past the tile)
    int soff[PER];               // its LDS index inside a buffer (the dump slot for an element past the tile)
    const int cq_t = tid % CQ;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int f = tid + u * NT;
        const int pix = f / CQ;
        const int iy = pix / IW, ix = pix % IW;
        const int gy = gy0 + iy, gx = gx0 + ix;
        const bool in = f < TOT;
        const bool ok = in && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
        goff[u] = ok ? (unsigned)(((gy * AW + gx) * CA + cq_t * 4) * 4) : 0x80000000u;
        soff[u] = in ? pix * LDH + cq_t * 4 : 2 * BUF + (tid & 63) * 4 - 0;
    }
    auto issue_stage = [&](const int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) pf[u] = buf_load16(irs, goff[u], (unsigned)c0 * 4u);
    };
    auto convert_stage = [&](const int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const float4 t = make_float4(__uint_as_float(pf[u].x), __uint_as_float(pf[u].y), __uint_as_float(pf[u].z), __uint_as_float(pf[u].w));
            uint2 pl[NPL];
            split_planes<NPL>(t, pl);
            const bool in = (u * NT + NT <= TOT) || tid + u * NT < TOT;
#pragma unroll
            for (int p = 0; p < NPL; ++p) *reinterpret_cast<uint2*>(sPl + soff[u] + (in ? buf + p * PLANE : 0)) = pl[p];
        }
    };

    issue_stage(0);
    convert_stage(0);
    issue_stage(nchunks > 1 ? CK : 0);
    __syncthreads();
    constexpr int MID = NTAPS / 2;                // the unit behind which the next chunk's tile is converted
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        const int cur = (ch & 1) * BUF;
        loadA(aq[0], 0, cur);
        __builtin_amdgcn_sched_barrier(0);        // (tap 0's reads go out together, ahead of the first unit's pipeline)
        static_for<0, NTAPS>([&](auto T) __attribute__((always_inline)) {
            constexpr int t = decltype(T)::value;
            const KFrag<NKS, NPL>& bc = bq[t % RING];
            KFrag<NKS, NPL>& bpf = bq[(t + RING - 1) % RING];
            const KFrag<NKS, NPL>& ac = aq[t % 2];
            constexpr int up = t + RING - 1;      // the unit RING - 1 ahead: tap up % NTAPS of chunk ch + up / NTAPS (past the end: a harmless re-load of chunk 0)
            if (!(K3_ABL & 1)) loadB(bpf, up % NTAPS, (ch + up / NTAPS < nchunks) ? c0 + (up / NTAPS) * CK : 0);
            if (!(K3_ABL & 2)) if constexpr (t + 1 < NTAPS) loadA(aq[(t + 1) % 2], t + 1, cur);
            // A = weights (rows = output channels), B = activations (columns = pixels).  bf16x3: w0 a0 | w1 a0 | w0 a1; bf16x6 adds w2 a0, w0 a2, w1 a1.
            if (!(K3_ABL & 8))
#pragma unroll
            for (int j = 0; j < NKS; ++j) {
                acc0 = mfma_bf16(bc.p[0][j], ac.p[0][j], acc0);
                acc1 = mfma_bf16(bc.p[1][j], ac.p[0][j], acc1);
                acc2 = mfma_bf16(bc.p[0][j], ac.p[1][j], acc2);
                if constexpr (NPL == 3) {
                    acc1 = mfma_bf16(bc.p[2][j], ac.p[0][j], acc1);
                    acc2 = mfma_bf16(bc.p[0][j], ac.p[2][j], acc2);
                    acc1 = mfma_bf16(bc.p[1][j], ac.p[1][j], acc1);
                }
            }
            constexpr int NM = NKS * (NPL == 3 ? 6 : 3), NP = NKS * NPL;
            static_for<0, NM>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                  // one MFMA
                if constexpr (i < NP) {
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                              // one VMEM read
                    if constexpr (t + 1 < NTAPS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); // one DS read
                }
            });
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (t == MID && !(K3_ABL & 4)) {
                convert_stage(BUF - cur);                                               // chunk ch + 1 (fetched during chunk ch - 1) -> the other buffer
                issue_stage(ch + 2 < nchunks ? c0 + 2 * CK : c0);                       // chunk ch + 2 (past the end: a harmless re-load)
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        if constexpr (NTAPS % RING != 0) bq[0] = bq[1];          // (one tap per chunk: the two-slot ring advances by one)
        if (!(K3_ABL & 16)) __syncthreads();          // chunk ch + 1's tile is complete, and every wave is done with chunk ch's (the next phase overwrites it)
    }

    // ---- epilogue: lane (l31, lh) owns pixel l31 of the wave's fragment and its channels n0 + 32 wn + 8 g + 4 lh + e (g, e < 4) ----
    const int oyp = a.os * (ty0 + pty) + a.oy, oxp = a.os * (tx0 + ptx) + a.ox;
    const size_t obase = (((size_t)n * a.OH + oyp) * a.OW + oxp) * Nn + n0 + wn * 32 + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float4 v;
        v.x = acc0[4 * g + 0] + (acc1[4 * g + 0] + acc2[4 * g + 0]);
        v.y = acc0[4 * g + 1] + (acc1[4 * g + 1] + acc2[4 * g + 1]);
        v.z = acc0[4 * g + 2] + (acc1[4 * g + 2] + acc2[4 * g + 2]);
        v.w = acc0[4 * g + 3] + (acc1[4 * g + 3] + acc2[4 * g + 3]);
        if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n0 + wn * 32 + 4 * lh + 8 * g); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
        if (a.add) { const float4 q = *reinterpret_cast<const float4*>(a.add + obase + 8 * g); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
        *reinterpret_cast<float4*>(a.Out + obase + 8 * g) = v;
    }
}

// Round 6, second step: the micro-benchmark's ablations of the pipelined kernel still ADD UP (MFMA-only 55 us, + weight-fragment loads 23, + activation-fragment
// reads 11, + staging 12 = the 96 us of the dominant shape): with a 32 x 32 wave tile every unit's six MFMAs (192 matrix-pipe cycles) need four 1-KB weight
// loads, and the CU's one texture-address path moves 64 B per clock -- 12 waves x 4 x 16 cycles = 768 cycles against the 576 matrix-pipe cycles of a SIMD's
// three waves: the kernel is bound by its fragment loads, not by the matrix pipe.  Here a wave owns ALL 64 pixels of the tile x 32 output channels (two
// M fragments): each weight fragment feeds twelve MFMAs (half the loads per MFMA), a workgroup is WGN waves = 32 WGN output channels over one staged tile
// (WGN 4: the input tile is staged once per 128 channels -- half the staging and half the tile re-reads), and the unit splits into two half-units
// (tap t, fragment m) so that only one fragment pair of activations is live beside the one being read.  Same products, same accumulators per output element,
// same order over (chunk, tap, k-step): bit-identical to convk16_kernel.
template <int TH, int TW, int CK, int WGN, int SIN, int EXT, int NTAPS, int NPL>
__global__ void __launch_bounds__(64 * WGN) convk16q_kernel(const ConvKArgs a) {
    constexpr int RING = NTAPS % 3 == 0 ? 3 : (NTAPS % 4 == 0 ? 4 : 2);
    static_assert(NTAPS % RING == 0 || NTAPS == 1, "the ring returns to slot 0 at every chunk boundary (one tap: a two-slot ring, one fragment copy per chunk)");
    static_assert(TH * TW == 64, "two 32-pixel fragments per wave");
    constexpr int NT = 64 * WGN;
    constexpr int IH = SIN * (TH - 1) + EXT + 1, IW = SIN * (TW - 1) + EXT + 1;
    constexpr int LDH = CK + 8;
    constexpr int NKS = CK / 16, CQ = CK / 4;
    constexpr int BN = 32 * WGN;
    static_assert(NT % CQ == 0, "a thread's channel quad is the same for every element it stages");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* sPl = reinterpret_cast<unsigned short*>(dsm);      // two buffers of NPL planes of IH x IW x LDH, then the dump slot
    constexpr int PLANE = IH * IW * LDH, BUF = NPL * PLANE;

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int tilesx = a.MW / TW;
    unsigned bx, by, bz;
    xcd_block(bx, by, bz);
    const int ty0 = ((int)bx / tilesx) * TH, tx0 = ((int)bx % tilesx) * TW;
    const int n = (int)by;
    const int n0 = (int)bz * BN;
    const int CA = a.CA, Nn = a.Nn, AH = a.AH, AW = a.AW;

    const int pty = l31 / TW, ptx = l31 % TW;                 // fragment 0's pixel; fragment 1's is 32 / TW rows below
    const int aoff = ((SIN * pty) * IW + SIN * ptx) * LDH + 8 * lh;
    constexpr int AOFF1 = (SIN * (32 / TW)) * IW * LDH;
    const int col = n0 + wn * 32 + l31;

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.Wp16), 0, 0xffffffff, 0x00020000);
    const unsigned lb = (unsigned)(lh * Nn + col) * 16u;
    const unsigned plane_b = (unsigned)((size_t)a.w16_plane / 8) * 16u;
    auto loadBj = [&](KFrag<NKS, NPL>& b, const int tap, const int c0, const int j) __attribute__((always_inline)) {
        const unsigned u = (unsigned)((a.widx[tap] * (CA / 8) + c0 / 8) * Nn) * 16u;
#pragma unroll
        for (int p = 0; p < NPL; ++p) b.p[p][j] = buf_load16(wrs, lb, u + (unsigned)(2 * j * Nn) * 16u + (unsigned)p * plane_b);
    };
    auto loadA = [&](KFrag<NKS, NPL>& f, const int tap, const int m, const int buf) __attribute__((always_inline)) {
        const int o = buf + aoff + m * AOFF1 + a.toff[tap] * LDH;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) f.p[p][j] = *reinterpret_cast<const uint4*>(sPl + o + p * PLANE + 16 * j);
    };

    const int nchunks = CA / CK;
    KFrag<NKS, NPL> bq[RING], aq[2];
    static_for<0, RING - 1>([&](auto U) __attribute__((always_inline)) {
        constexpr int u = decltype(U)::value;
#pragma unroll
        for (int j = 0; j < NKS; ++j) loadBj(bq[u], u % NTAPS, (u / NTAPS < nchunks) ? (u / NTAPS) * CK : 0, j);
    });

    v16f acc[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][k][r] = 0.f;

    // ---- staging: element f of the tile = (pixel f / CQ, channel quad f % CQ); out-of-image pixels read through the buffer's bounds check ----
    const int gy0 = SIN * ty0 + a.y0, gx0 = SIN * tx0 + a.x0;
    const size_t sample_b = (size_t)AH * AW * CA * 4;
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.A) + (size_t)n * AH * AW * CA), 0,
                                                                          (unsigned)sample_b, 0x00020000);
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    uint4 pf[PER];
    unsigned goff[PER];          // byte offset of the element's channel quad in chunk 0 (2^31: outside the image or past the tile)
    int soff[PER];               // its LDS index inside a buffer (the dump slot for an element past the tile)
    const int cq_t = tid % CQ;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int f = tid + u * NT;
        const int pix = f / CQ;
        const int iy = pix / IW, ix = pix % IW;
        const int gy = gy0 + iy, gx = gx0 + ix;
        const bool in = f < TOT;
        const bool ok = in && (unsigned)gy < (unsigned)AH && (unsigned)gx < (unsigned)AW;
        goff[u] = ok ? (unsigned)(((gy * AW + gx) * CA + cq_t * 4) * 4) : 0x80000000u;
        soff[u] = in ? pix * LDH + cq_t * 4 : 2 * BUF + (tid & 63) * 4;
    }
    auto issue_stage = [&](const int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) pf[u] = buf_load16(irs, goff[u], (unsigned)c0 * 4u);
    };
    auto convert_stage = [&](const int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const float4 t = make_float4(__uint_as_float(pf[u].x), __uint_as_float(pf[u].y), __uint_as_float(pf[u].z), __uint_as_float(pf[u].w));
            uint2 pl[NPL];
            split_planes<NPL>(t, pl);
            const bool in = (u * NT + NT <= TOT) || tid + u * NT < TOT;
#pragma unroll
            for (int p = 0; p < NPL; ++p) *reinterpret_cast<uint2*>(sPl + soff[u] + (in ? buf + p * PLANE : 0)) = pl[p];
        }
    };

    issue_stage(0);
    convert_stage(0);
    issue_stage(nchunks > 1 ? CK : 0);
    __syncthreads();
    constexpr int MID = NTAPS / 2;                // the unit behind which the next chunk's tile is converted
    constexpr int MPJ = NPL == 3 ? 6 : 3, NM = NKS * MPJ, NPA = NKS * NPL;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * CK;
        const int cur = (ch & 1) * BUF;
        loadA(aq[0], 0, 0, cur);
        __builtin_amdgcn_sched_barrier(0);        // (the first half-unit's reads go out together, ahead of its pipeline)
        static_for<0, 2 * NTAPS>([&](auto H) __attribute__((always_inline)) {
            constexpr int h = decltype(H)::value, t = h / 2, m = h % 2;
            const KFrag<NKS, NPL>& bc = bq[t % RING];
            KFrag<NKS, NPL>& bpf = bq[(t + RING - 1) % RING];
            const KFrag<NKS, NPL>& ac = aq[m];
            constexpr int up = t + RING - 1;      // the unit RING - 1 ahead: tap up % NTAPS of chunk ch + up / NTAPS (past the end: a harmless re-load of chunk 0)
            // this half-unit's memory instructions: half of the prefetched unit's weight fragment (k-steps of parity m), the next half-unit's activation fragment
            if (!(K3_ABL & 1))
#pragma unroll
            for (int j = m; j < NKS; j += 2) loadBj(bpf, up % NTAPS, (ch + up / NTAPS < nchunks) ? c0 + (up / NTAPS) * CK : 0, j);
            if (!(K3_ABL & 2)) if constexpr (h + 1 < 2 * NTAPS) loadA(aq[1 - m], (h + 1) / 2, (h + 1) % 2, cur);
            // A = weights (rows = output channels), B = activations (columns = pixels).  bf16x3: w0 a0 | w1 a0 | w0 a1; bf16x6 adds w2 a0, w0 a2, w1 a1.
            if (!(K3_ABL & 8))
#pragma unroll
            for (int j = 0; j < NKS; ++j) {
                acc[m][0] = mfma_bf16(bc.p[0][j], ac.p[0][j], acc[m][0]);
                acc[m][1] = mfma_bf16(bc.p[1][j], ac.p[0][j], acc[m][1]);
                acc[m][2] = mfma_bf16(bc.p[0][j], ac.p[1][j], acc[m][2]);
                if constexpr (NPL == 3) {
                    acc[m][1] = mfma_bf16(bc.p[2][j], ac.p[0][j], acc[m][1]);
                    acc[m][2] = mfma_bf16(bc.p[0][j], ac.p[2][j], acc[m][2]);
                    acc[m][1] = mfma_bf16(bc.p[1][j], ac.p[1][j], acc[m][1]);
                }
            }
            constexpr int NPB = (NKS / 2) * NPL;      // weight loads of this half-unit
            static_for<0, NM>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                      // one MFMA
                if constexpr (i < NPA && h + 1 < 2 * NTAPS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          // one DS read
                if constexpr (i >= NM - NPB) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                         // one VMEM read
            });
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (h == 2 * MID + 1 && !(K3_ABL & 4)) {
                convert_stage(BUF - cur);                                               // chunk ch + 1 (fetched during chunk ch - 1) -> the other buffer
                issue_stage(ch + 2 < nchunks ? c0 + 2 * CK : c0);                       // chunk ch + 2 (past the end: a harmless re-load)
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        if constexpr (NTAPS % RING != 0) bq[0] = bq[1];          // (one tap per chunk: the two-slot ring advances by one)
        if (!(K3_ABL & 16)) __syncthreads();          // chunk ch + 1's tile is complete, and every wave is done with chunk ch's (the next phase overwrites it)
    }

    // ---- epilogue: lane (l31, lh) owns pixel l31 of each fragment and its channels n0 + 32 wn + 8 g + 4 lh + e (g, e < 4) ----
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int oyp = a.os * (ty0 + pty + m * (32 / TW)) + a.oy, oxp = a.os * (tx0 + ptx) + a.ox;
        const size_t obase = (((size_t)n * a.OH + oyp) * a.OW + oxp) * Nn + n0 + wn * 32 + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 v;
            v.x = acc[m][0][4 * g + 0] + (acc[m][1][4 * g + 0] + acc[m][2][4 * g + 0]);
            v.y = acc[m][0][4 * g + 1] + (acc[m][1][4 * g + 1] + acc[m][2][4 * g + 1]);
            v.z = acc[m][0][4 * g + 2] + (acc[m][1][4 * g + 2] + acc[m][2][4 * g + 2]);
            v.w = acc[m][0][4 * g + 3] + (acc[m][1][4 * g + 3] + acc[m][2][4 * g + 3]);
            if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n0 + wn * 32 + 4 * lh + 8 * g); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
            if (a.add) { const float4 q = *reinterpret_cast<const float4*>(a.add + obase + 8 * g); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
            *reinterpret_cast<float4*>(a.Out + obase + 8 * g) = v;
        }
    }
}

// Optional HIP-event profiler of the k3 launches (uad_k3_profile_*: bench.py's roofline leg for configs[3], whose handle has no per-launch-group
// profiler): while enabled every convk16 / convk_w16 launch is bracketed by two events on its stream; the read-out sums the durations per launch
// shape.  key: kind (0 tap-list F / D, 1 filter gradient), SIN or S, EXT or NCB, NTAPS, NPL, N, MH, MW, CA, Nn, kernel form (tap-list: 0 first kernel, 1 convk16p,
// 2 / 3 convk16q with 64 / 128 channels per workgroup; filter gradient: 0 first kernel, 1 convk_w16p)
struct K3ProfRec { int key[11]; hipEvent_t a, b; };
static bool g_k3prof = false;
static std::vector<K3ProfRec> g_k3recs;
struct K3ProfScope {
    hipStream_t st; hipEvent_t b = nullptr;
    K3ProfScope(hipStream_t s, int kind, int p1, int p2, int ntaps, int npl, int N, int MH, int MW, int CA, int Nn, int form) : st(s) {
        if (!g_k3prof) return;
        K3ProfRec r{{kind, p1, p2, ntaps, npl, N, MH, MW, CA, Nn, form}, nullptr, nullptr};
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        (void)hipEventRecord(r.a, st);
        b = r.b;
        g_k3recs.push_back(r);
    }
    ~K3ProfScope() { if (b) (void)hipEventRecord(b, st); }
};

// (128-channel output blocks on eight waves -- half the input re-reads, the PMC passes put the 64-channel form at 3.6x its algorithmic bytes -- measured
// 9 % SLOWER over the configs[3] iteration, 60.3 vs 55.4 ms same box: one eight-wave workgroup per CU has nobody to overlap its staging with.)
// Kernel form of a launch: 0 convk16_kernel (first form), 1 convk16p (pipelined, 32 x 32 wave tiles), 2 / 3 convk16q with 64 / 128 output channels per
// workgroup (64 x 32 wave tiles).  tools/k3_ubench.hip over the shapes of configs[3] (profiles/r06_g_k3_forms.md): the 128-channel form wins wherever it
// still fills the chip (>= 256 workgroups), the 64-channel q form only on large grids (>= 1024 workgroups: its two-wave workgroups leave a small launch at
// one wave per SIMD), the pipelined 32 x 32 form everywhere else.  UAD_K3_FORM=<n> forces a form (A/B), tools/k3_ubench -DK3_FORM=<n> likewise.
#ifndef K3_FORM
#define K3_FORM -1
#endif
template <int SIN, int EXT, int NTAPS, int NPL>
void launch_convk16_p(const ConvKArgs& a, hipStream_t st) {
    constexpr int TH = 8, TW = 8, CK = 32;
    constexpr int IH = SIN * (TH - 1) + EXT + 1, IW = SIN * (TW - 1) + EXT + 1;
    dim3 grid((a.MH / TH) * (a.MW / TW), a.N, a.Nn / 64);
    constexpr size_t lds2 = (size_t)2 * NPL * IH * IW * (CK + 8) * 2 + 512;      // two tile buffers + the staging dump slot
    constexpr bool PIPE = (NTAPS % 3 == 0 || NTAPS == 4 || NTAPS == 2 || NTAPS == 1) && lds2 <= 52 * 1024;      // (three workgroups per CU)
    int form = 0;
    if constexpr (PIPE) {
        static const int forced = K3_FORM >= 0 ? K3_FORM : (getenv("UAD_K3_FORM") ? atoi(getenv("UAD_K3_FORM")) : -1);
        const long long wgs64 = (long long)grid.x * grid.y * grid.z;
        form = (a.Nn % 128 == 0 && wgs64 / 2 >= 256) ? 3 : ((a.Nn % 128 != 0 && wgs64 >= 1024) ? 2 : 1);
        if (NTAPS == 1 && a.CA < 128) form = 0;          // (a one-tap launch of two chunks has nothing to pipeline)
        if (forced >= 0) form = (forced == 3 && a.Nn % 128 != 0) ? 2 : forced;
    }
    K3ProfScope prof(st, 0, SIN, EXT, NTAPS, NPL, a.N, a.MH, a.MW, a.CA, a.Nn, form);
    if constexpr (PIPE) {
        if (form != 0) {
            static bool attr_set2 = false;
            if (!attr_set2) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(convk16p_kernel<TH, TW, CK, 2, 2, SIN, EXT, NTAPS, NPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(convk16q_kernel<TH, TW, CK, 2, SIN, EXT, NTAPS, NPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(convk16q_kernel<TH, TW, CK, 4, SIN, EXT, NTAPS, NPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
                attr_set2 = true;
            }
            if (form == 3) hipLaunchKernelGGL((convk16q_kernel<TH, TW, CK, 4, SIN, EXT, NTAPS, NPL>), dim3(grid.x, grid.y, a.Nn / 128), dim3(256), lds2, st, a);
            else if (form == 2) hipLaunchKernelGGL((convk16q_kernel<TH, TW, CK, 2, SIN, EXT, NTAPS, NPL>), grid, dim3(128), lds2, st, a);
            else hipLaunchKernelGGL((convk16p_kernel<TH, TW, CK, 2, 2, SIN, EXT, NTAPS, NPL>), grid, dim3(256), lds2, st, a);
            return;
        }
    }
    constexpr size_t lds = (size_t)NPL * IH * IW * (CK + 8) * 2;
    constexpr bool TPF = !(NPL == 3 && SIN == 2);      // (bf16x6 on the 17 x 17 stride-2 halo: 10 prefetch registers x 4 do not fit beside three planes of fragments)
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(convk16_kernel<TH, TW, CK, 2, 2, SIN, EXT, NTAPS, NPL, TPF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((convk16_kernel<TH, TW, CK, 2, 2, SIN, EXT, NTAPS, NPL, TPF>), grid, dim3(256), lds, st, a);
}
template <int SIN, int EXT, int NTAPS>
void launch_convk16(const ConvKArgs& a, int planes, hipStream_t st) {
    if (planes == 3) launch_convk16_p<SIN, EXT, NTAPS, 3>(a, st); else launch_convk16_p<SIN, EXT, NTAPS, 2>(a, st);
}

// k1 s2 transposed convolution (the generator's shortcut, models/fanogan_schlegl.py:40,47,54): only the even-even output pixels receive a
// contraction; every other pixel of the output is bias (+ addend)
__global__ void __launch_bounds__(256) k1s2_fill_kernel(float* __restrict__ out, const float* __restrict__ bias, const float* __restrict__ add,
                                                        int OW, int Nn, size_t total4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // float4 index over [N, OH, OW, Nn]
    if (i >= total4) return;
    const int c4 = (int)(i % (Nn / 4));
    const size_t pix = i / (Nn / 4);
    const int x = (int)(pix % OW), y = (int)((pix / OW) & 1);       // (row parity: OH is even, so pix / OW mod 2 is the row's parity)
    if (!((x & 1) | y)) return;
    float4 v = bias ? *reinterpret_cast<const float4*>(bias + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (add) { const float4 q = *reinterpret_cast<const float4*>(add + i * 4); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    *reinterpret_cast<float4*>(out + i * 4) = v;
}

// ------------------------------------------------------------------------------------------------
// Filter gradient of the k3 layers in bf16x3: dW[ky, kx][cb][cs] = sum over (n, i, j) big(S i - P + ky, S j - P + kx)[cb] * small(i, j)[cs]
// (S 1: P 1, big and small on the same grid; S 2: P 0, big = 2 x small).  Channel-major scheme of conv5_w_bf16_t_kernel: a workgroup owns
// 32 NCB big-side channels x 64 small-side channels and walks 8 x 8 tiles of small positions; per tile the big halo and the small tile are staged
// PIXEL-major (bf16 hi | lo planes, two 8-byte stores per float4) and the W-kind fragments -- lane = channel, eight consecutive positions -- are
// gathered by gfx950's transpose read (ds_read_b64_tr_b16: per 16-lane group four positions x 16 channels, per-lane row addresses, so the stride-2
// big pixels of a tap cost nothing extra).  (First version of this round: channel-major 16-bit scatter + segment reads, 12-20 % slower.)  Waves: one per (kernel row ky,
// cb block): 3 taps x 2 cs blocks = six 32 x 32 accumulators, contraction over the tile's 64 positions in four steps.  Slabs + fixed-order
// reduction like the k5 kernel (deterministic).
// ------------------------------------------------------------------------------------------------
template <int S, int NCB>
__global__ void __launch_bounds__(192 * NCB) __attribute__((amdgpu_waves_per_eu(2)))
convk_w16_kernel(const ConvWArgs a, int tiles_per_split, int total_tiles) {
    constexpr int TH = 8, TW = 8, IH = S * (TH - 1) + 3, IW = IH, CQ = 8 * NCB, NT = 192 * NCB, NCS = 2, CSQ = 8 * NCS;
    constexpr int LDH = 32 * NCB + 8;              // ushorts per big pixel
    constexpr int BIGP = IH * IW * LDH;            // ushorts per plane
    constexpr int LDQ = 32 * NCS + 8;              // ushorts per small position
    typedef short v4s __attribute__((ext_vector_type(4)));
    static_assert(NT % CQ == 0 && NT % CSQ == 0, "fixed channel quad per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* bHi = reinterpret_cast<unsigned short*>(dsm);
    unsigned short* bLo = bHi + BIGP;
    unsigned short* sHiT = bLo + BIGP;
    unsigned short* sLoT = sHiT + TH * TW * LDQ;

    const int tid = threadIdx.x, lane = tid & 63, wave_all = tid >> 6;
    const int ky = wave_all % 3, cbh = wave_all / 3;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int cb0 = blockIdx.x * 32 * NCB, cs0 = blockIdx.y * 32 * NCS;
    const int tilesx = d.WS / TW, tilesy = d.HS / TH;
    const int t_begin = blockIdx.z * tiles_per_split;
    const int t_end = min(t_begin + tiles_per_split, total_tiles);

    v16f acc[3][NCS];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < NCS; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][c][r] = 0.f;

    // fragments by transpose reads from PIXEL-major tiles (ds_read_b64_tr_b16, see conv5_w_bf16_tr_kernel in uad_conv5_w.hip): lane (i = l & 15,
    // chalf = (l >> 4) & 1, lh = l >> 5) supplies the address of position 8 lh + 4 t + i / 4 of the K = 16 step, channels 16 chalf + 4 (i & 3) .. + 3
    auto tr8 = [&](const unsigned short* plane, const int addr, const int step) __attribute__((always_inline)) {
        const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(const_cast<unsigned short*>(plane) + addr));
        const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(const_cast<unsigned short*>(plane) + addr + step));
        const uint2 lo2 = __builtin_bit_cast(uint2, r0), hi2 = __builtin_bit_cast(uint2, r1);
        return make_uint4(lo2.x, lo2.y, hi2.x, hi2.y);
    };
    auto mma3 = [&](v16f& c, uint4 ah, uint4 al, uint4 bh, uint4 bl) __attribute__((always_inline)) {
        c = mfma_bf16(ah, bh, c);
        c = mfma_bf16(ah, bl, c);
        c = mfma_bf16(al, bh, c);
    };

    // staging maps: element u of a thread is DP pixels further in the halo / DS positions further in the small tile
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    constexpr int DP = NT / CQ, DIY = DP / IW, DIX = DP % IW;
    const int cq = tid % CQ, pix0 = tid / CQ, iy0 = pix0 / IW, ix0 = pix0 % IW;
    constexpr int STOT = TH * TW * CSQ;
    constexpr int SPER = (STOT + NT - 1) / NT;
    float4 v[PER], sv[SPER];
    auto tile_origin = [&](int t, int& n, int& ty0, int& tx0) __attribute__((always_inline)) {
        tx0 = (t % tilesx) * TW;
        ty0 = ((t / tilesx) % tilesy) * TH;
        n = t / (tilesx * tilesy);
    };
    auto issue = [&](int t) __attribute__((always_inline)) {
        int n, ty0, tx0;
        tile_origin(t, n, ty0, tx0);
        const int gy0 = S * ty0 - d.P, gx0 = S * tx0 - d.P;
        const float* bigb = a.big + (size_t)n * d.HB * d.WB * d.CB + cb0 + cq * 4;
        int iy = iy0, ix = ix0;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int gy = gy0 + iy, gx = gx0 + ix;
            const bool ok = (tid + u * NT < TOT) && (unsigned)gy < (unsigned)d.HB && (unsigned)gx < (unsigned)d.WB;
            v[u] = ok ? *reinterpret_cast<const float4*>(bigb + (size_t)(gy * d.WB + gx) * d.CB) : make_float4(0.f, 0.f, 0.f, 0.f);
            ix += DIX; iy += DIY;
            if (ix >= IW) { ix -= IW; ++iy; }
        }
        const float* smb = a.small_ + ((size_t)(n * d.HS + ty0) * d.WS + tx0) * d.CS + cs0;
#pragma unroll
        for (int u = 0; u < SPER; ++u) {
            const int idx = tid + u * NT;
            const int pos = idx / CSQ, csq = idx % CSQ;
            sv[u] = (idx < STOT) ? *reinterpret_cast<const float4*>(smb + (size_t)((pos / TW) * d.WS + (pos % TW)) * d.CS + csq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto commit = [&]() __attribute__((always_inline)) {
        int iy = iy0, ix = ix0;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (tid + u * NT < TOT) {
                uint2 hi, lo;
                split_bf16(v[u], hi, lo);
                const int o = (iy * IW + ix) * LDH + cq * 4;
                *reinterpret_cast<uint2*>(bHi + o) = hi;
                *reinterpret_cast<uint2*>(bLo + o) = lo;
            }
            ix += DIX; iy += DIY;
            if (ix >= IW) { ix -= IW; ++iy; }
        }
#pragma unroll
        for (int u = 0; u < SPER; ++u) {
            const int idx = tid + u * NT;
            if (idx >= STOT) continue;
            const int pos = idx / CSQ, csq = idx % CSQ;
            uint2 hi, lo;
            split_bf16(sv[u], hi, lo);
            *reinterpret_cast<uint2*>(sHiT + pos * LDQ + csq * 4) = hi;
            *reinterpret_cast<uint2*>(sLoT + pos * LDQ + csq * 4) = lo;
        }
    };

    const int li = lane & 15, chalf = (lane >> 4) & 1;
    // big: pixel (S (2 js + lh) + ky, S (4 t + li / 4) + kx), channels cbh 32 + 16 chalf + 4 (li & 3); small: position 16 js + 8 lh + 4 t + li / 4
    const int a_base = ((S * lh + ky) * IW + S * (li >> 2)) * LDH + cbh * 32 + 16 * chalf + 4 * (li & 3);      // + (2 S js IW + kx + 4 S t) LDH
    const int b_base = (8 * lh + (li >> 2)) * LDQ + 16 * chalf + 4 * (li & 3);                                   // + (16 js + 4 t) LDQ + 32 c
    if (t_begin < t_end) issue(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                   // the previous tile's fragments are consumed
        commit();
        if (t + 1 < t_end) issue(t + 1);   // in flight across the barrier and the MFMA loop below
        __syncthreads();
#pragma unroll
        for (int js = 0; js < TH * TW / 16; ++js) {
            uint4 bh[NCS], bl[NCS];
#pragma unroll
            for (int c = 0; c < NCS; ++c) {
                bh[c] = tr8(sHiT, b_base + 16 * js * LDQ + 32 * c, 4 * LDQ);
                bl[c] = tr8(sLoT, b_base + 16 * js * LDQ + 32 * c, 4 * LDQ);
            }
            const int ao = a_base + (2 * S * js * IW) * LDH;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const uint4 ah = tr8(bHi, ao + kx * LDH, 4 * S * LDH), al = tr8(bLo, ao + kx * LDH, 4 * S * LDH);
#pragma unroll
                for (int c = 0; c < NCS; ++c) mma3(acc[kx][c], ah, al, bh[c], bl[c]);
            }
        }
    }

    // accumulators -> slab (register r of lane (l31, lh): cb = 8 (r >> 2) + 4 lh + (r & 3), cs = l31)
    const int CSi = d.CS;
    const int tapstride = d.CB * CSi;
    float* ob = a.partial + (size_t)blockIdx.z * a.Mtot * CSi + (size_t)(cb0 + cbh * 32 + 4 * lh) * CSi + cs0 + l31;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int c = 0; c < NCS; ++c) {
            float* ot = ob + (ky * 3 + kx) * tapstride + c * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[((r & 3) + 8 * (r >> 2)) * CSi] = acc[kx][c][r];
        }
}

// Round 6: the k3 s1 filter gradient with a PIPELINED tile loop.  The first kernel (convk_w16_kernel<1, 2>) allocates 212 VGPRs, so its six-wave workgroups run
// ONE per CU -- 1.5 waves per SIMD, two barriers per tile with the convert pass of every wave between them and nobody to overlap it with: 0.38 of the matrix
// peak (tools/k3_ubench.hip w1).  Here the same 64 x 64-channel workgroup tile is owned by TWELVE waves (kernel row ky x 32-channel big block x 32-channel
// small block: three 32 x 32 accumulators per wave instead of six -- three waves per SIMD, every SIMD the same load), both LDS tiles are double-buffered
// (tile t + 1 is converted into the other buffer in the middle of tile t's MFMA phase, the global loads of tile t + 2 follow it; one barrier per tile), the
// tile body is straight-line code (elements past the halo go to a dump slot; the loads run through one buffer descriptor whose range check returns the
// padding zeros).  Same fragments, same products, same order per output element: bit-identical slabs.
template <int S, int TH>
__global__ void __launch_bounds__(768) convk_w16p_kernel(const ConvWArgs a, int tiles_per_split, int total_tiles) {
    constexpr int NCB = 2, NCS = 2;
    // TH: rows of a sub-tile (8: the whole 8 x 8 tile; 4: its upper / lower half, in the first kernel's order of positions -- the 17 x 17 stride-2 halo
    // of a whole tile does not fit twice)
    constexpr int TW = 8, IH = S * (TH - 1) + 3, IW = S * (TW - 1) + 3, CQ = 8 * NCB, NT = 768, CSQ = 8 * NCS, NSUB = 8 / TH, NJS = TH * TW / 16;
    constexpr int LDH = 32 * NCB + 8;              // ushorts per big pixel
    constexpr int BIGP = IH * IW * LDH;            // ushorts per plane
    constexpr int LDQ = 32 * NCS + 8;              // ushorts per small position
    constexpr int SMP = TH * TW * LDQ;
    constexpr int BUFW = 2 * BIGP + 2 * SMP;       // one buffer: big hi | big lo | small hi | small lo
    typedef short v4s __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* lds = reinterpret_cast<unsigned short*>(dsm);      // two buffers, then the dump slot

    const int tid = threadIdx.x, lane = tid & 63, wave_all = tid >> 6;
    const int ky = wave_all % 3, cbh = (wave_all / 3) % 2, csh = wave_all / 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    unsigned bx, by, bz;
    xcd_block(bx, by, bz);      // (the (cb, cs) blocks of one split on one XCD: they read the same tiles)
    const int cb0 = (int)bx * 32 * NCB, cs0 = (int)by * 32 * NCS;
    const int tilesx = d.WS / TW, tilesy = d.HS / 8;
    const int t_begin = (int)bz * tiles_per_split * NSUB;          // in sub-tiles
    const int t_end = min((int)bz * tiles_per_split + tiles_per_split, total_tiles) * NSUB;

    v16f acc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    auto tr8 = [&](const int addr, const int step) __attribute__((always_inline)) {
        const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(lds + addr));
        const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(lds + addr + step));
        const uint2 lo2 = __builtin_bit_cast(uint2, r0), hi2 = __builtin_bit_cast(uint2, r1);
        return make_uint4(lo2.x, lo2.y, hi2.x, hi2.y);
    };

    // ---- staging maps (tile-invariant): element u of a thread = halo pixel (iy, ix), channel quad cq | small position pos, channel quad csq ----
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;
    constexpr int STOT = TH * TW * CSQ;
    constexpr int SPER = (STOT + NT - 1) / NT;
    constexpr int DUMP = 2 * BUFW;
    const size_t big_b = (size_t)d.N * d.HB * d.WB * d.CB * 4, small_b = (size_t)d.N * d.HS * d.WS * d.CS * 4;
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void*)const_cast<float*>(a.big), 0, (unsigned)big_b, 0x00020000);
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void*)const_cast<float*>(a.small_), 0, (unsigned)small_b, 0x00020000);
    int biy[PER], bix[PER], bso[PER];
    unsigned bco[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int f = tid + u * NT;
        const int pix = f / CQ, cq = f % CQ;
        biy[u] = pix / IW; bix[u] = pix % IW;
        bco[u] = (unsigned)(cb0 + cq * 4) * 4u;
        bso[u] = f < TOT ? pix * LDH + cq * 4 : -1;
    }
    int sso[SPER];
    unsigned sgo[SPER];
#pragma unroll
    for (int u = 0; u < SPER; ++u) {
        const int f = tid + u * NT;
        const int pos = f / CSQ, csq = f % CSQ;
        sgo[u] = f < STOT ? (unsigned)(((pos / TW) * d.WS + (pos % TW)) * d.CS + cs0 + csq * 4) * 4u : 0x80000000u;
        sso[u] = f < STOT ? pos * LDQ + csq * 4 : -1;
    }
    uint4 v[PER], sv[SPER];
    auto issue = [&](const int t) __attribute__((always_inline)) {
        const int t8 = t / NSUB, sub = t % NSUB;
        const int tx0 = (t8 % tilesx) * TW, ty0 = ((t8 / tilesx) % tilesy) * 8 + sub * TH, n = t8 / (tilesx * tilesy);
        const int gy0 = S * ty0 - d.P, gx0 = S * tx0 - d.P;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int gy = gy0 + biy[u], gx = gx0 + bix[u];
            const bool ok = bso[u] >= 0 && (unsigned)gy < (unsigned)d.HB && (unsigned)gx < (unsigned)d.WB;
            const unsigned off = ok ? (unsigned)(((n * d.HB + gy) * d.WB + gx) * d.CB) * 4u + bco[u] : 0x80000000u;
            v[u] = buf_load16(brs, off, 0);
        }
        const unsigned sbase = (unsigned)(((n * d.HS + ty0) * d.WS + tx0) * d.CS) * 4u;
#pragma unroll
        for (int u = 0; u < SPER; ++u) sv[u] = buf_load16(srs, sgo[u], sbase);
    };
    auto commit = [&](const int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            uint2 hi, lo;
            split_bf16(make_float4(__uint_as_float(v[u].x), __uint_as_float(v[u].y), __uint_as_float(v[u].z), __uint_as_float(v[u].w)), hi, lo);
            const int o = bso[u] >= 0 ? buf + bso[u] : DUMP + (tid & 63) * 4;
            *reinterpret_cast<uint2*>(lds + o) = hi;
            *reinterpret_cast<uint2*>(lds + o + (bso[u] >= 0 ? BIGP : 0)) = lo;
        }
#pragma unroll
        for (int u = 0; u < SPER; ++u) {
            uint2 hi, lo;
            split_bf16(make_float4(__uint_as_float(sv[u].x), __uint_as_float(sv[u].y), __uint_as_float(sv[u].z), __uint_as_float(sv[u].w)), hi, lo);
            const int o = sso[u] >= 0 ? buf + 2 * BIGP + sso[u] : DUMP + (tid & 63) * 4;
            *reinterpret_cast<uint2*>(lds + o) = hi;
            *reinterpret_cast<uint2*>(lds + o + (sso[u] >= 0 ? SMP : 0)) = lo;
        }
    };

    const int li = lane & 15, chalf = (lane >> 4) & 1;
    // big: pixel (S (2 js + lh) + ky, S (4 t + li / 4) + kx), channels cbh 32 + 16 chalf + 4 (li & 3); small: position 16 js + 8 lh + 4 t + li / 4
    const int a_base = ((S * lh + ky) * IW + S * (li >> 2)) * LDH + cbh * 32 + 16 * chalf + 4 * (li & 3);      // + (2 S js IW + kx + 4 S t) LDH
    const int b_base = 2 * BIGP + (8 * lh + (li >> 2)) * LDQ + 32 * csh + 16 * chalf + 4 * (li & 3);           // + (16 js + 4 t) LDQ
    if (t_begin < t_end) {
        issue(t_begin);
        commit(0);
        issue(min(t_begin + 1, t_end - 1));
        __syncthreads();
    }
#ifndef K3_WNODB
#define K3_WNODB 0      // tools/k3_ubench: single-buffered tiles, two barriers per tile (what the double buffer is worth at twelve waves)
#endif
    for (int t = t_begin; t < t_end; ++t) {
        const int cur = K3_WNODB ? 0 : ((t - t_begin) & 1) * BUFW;
        if (K3_WNODB && t > t_begin) { commit(0); issue(min(t + 1, t_end - 1)); __syncthreads(); }
#pragma unroll
        for (int js = 0; js < NJS; ++js) {
            const uint4 bh = tr8(cur + b_base + 16 * js * LDQ, 4 * LDQ), bl = tr8(cur + b_base + SMP + 16 * js * LDQ, 4 * LDQ);
            const int ao = cur + a_base + (2 * S * js * IW) * LDH;
            uint4 ah[3], al[3];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) { ah[kx] = tr8(ao + kx * LDH, 4 * S * LDH); al[kx] = tr8(ao + BIGP + kx * LDH, 4 * S * LDH); }
            // per accumulator the order of the first kernel (hi hi | hi lo | lo hi); the three kx chains interleave
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[kx] = mfma_bf16(ah[kx], bh, acc[kx]);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[kx] = mfma_bf16(ah[kx], bl, acc[kx]);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[kx] = mfma_bf16(al[kx], bh, acc[kx]);
            if (!K3_WNODB && js == NJS / 2 - 1) {      // (every wave converts at the same step; staggering the convert over the SIMD's three waves measured 5 % slower: abl_113608.log)
                __builtin_amdgcn_sched_barrier(0);
                commit(BUFW - cur);                                  // tile t + 1 (fetched during tile t - 1) -> the other buffer
                issue(min(t + 2, t_end - 1));                        // tile t + 2 (past the end: a harmless re-load)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();          // tile t + 1 is complete in LDS, and every wave is done with tile t's buffer
    }

    // accumulators -> slab (register r of lane (l31, lh): cb = 8 (r >> 2) + 4 lh + (r & 3), cs = l31)
    const int CSi = d.CS;
    const int tapstride = d.CB * CSi;
    float* ob = a.partial + (size_t)bz * a.Mtot * CSi + (size_t)(cb0 + cbh * 32 + 4 * lh) * CSi + cs0 + csh * 32 + l31;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        float* ot = ob + (ky * 3 + kx) * tapstride;
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[((r & 3) + 8 * (r >> 2)) * CSi] = acc[kx][r];
    }
}

template <int S, int TH>
constexpr size_t convk_w16p_lds_bytes() {
    constexpr int IH = S * (TH - 1) + 3, IW = S * 7 + 3;
    return 2 * ((size_t)2 * IH * IW * (32 * 2 + 8) * 2 + (size_t)2 * TH * 8 * (32 * 2 + 8) * 2) + 512;
}

template <int S, int NCB>
constexpr size_t convk_w16_lds_bytes() {
    constexpr int IH = S * 7 + 3;
    return (size_t)2 * IH * IH * (32 * NCB + 8) * 2 + (size_t)2 * 64 * (32 * 2 + 8) * 2;
}

#ifndef K3_WFORM
#define K3_WFORM -1
#endif
template <int S, int NCB>
void launch_convk_w16(const ConvWArgs& a, const WK3Choice& c, hipStream_t st) {
    dim3 grid(a.d.CB / (32 * NCB), a.d.CS / 64, c.splits);
    // pipelined twelve-wave form, 64 x 64 channels per workgroup (UAD_K3_WFORM=0 / tools/k3_ubench -DK3_WFORM=0: the first kernel)
    static const int forced = K3_WFORM >= 0 ? K3_WFORM : (getenv("UAD_K3_WFORM") ? atoi(getenv("UAD_K3_WFORM")) : -1);
    // (the pipelined kernel addresses each operand through ONE buffer descriptor and uses offset 2^31 as its out-of-range mark: tensors below 2 GB)
    const bool small_enough = (size_t)a.d.N * a.d.HB * a.d.WB * a.d.CB * 4 < (1ull << 31) && (size_t)a.d.N * a.d.HS * a.d.WS * a.d.CS * 4 < (1ull << 31);
    const bool pform = forced != 0 && small_enough && (NCB == 2 || (S == 2 && a.d.CB % 64 == 0));
    K3ProfScope prof(st, 1, S, NCB, 9, 2, a.d.N, a.d.HS, a.d.WS, a.d.CB, a.d.CS, pform ? 1 : 0);
    if (pform) {
#ifndef K3_WTH
#define K3_WTH 8          // (tools/k3_ubench: 4 = half-tile sub-steps for stride 1 too -- measured 7-11 % slower)
#endif
        constexpr int TH = S == 1 ? K3_WTH : 4;
        constexpr size_t ldsp = convk_w16p_lds_bytes<S, TH>();
        static bool attrp_set = false;
        if (!attrp_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(convk_w16p_kernel<S, TH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsp);
            attrp_set = true;
        }
        hipLaunchKernelGGL((convk_w16p_kernel<S, TH>), dim3(a.d.CB / 64, a.d.CS / 64, c.splits), dim3(768), ldsp, st, a, c.tiles_per_split, c.total_tiles);
        return;
    }
    constexpr size_t lds = convk_w16_lds_bytes<S, NCB>();
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(convk_w16_kernel<S, NCB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((convk_w16_kernel<S, NCB>), grid, dim3(192 * NCB), lds, st, a, c.tiles_per_split, c.total_tiles);
}

