// k5 s2 filter gradient: conv5_w_bf16_tr_kernel on bf16 planes (bf16x3 / bf16x6) and conv5_w_kernel in exact fp32.  uad_conv_plan.hip (uad_launch_conv_w)
// decides the instance and calls uad_conv5_w16_launch / uad_conv5_w32_launch below.
#include "uad_gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// k5 s2 SAME filter gradient, spatial form: one workgroup owns a 32(cb) x 32(cs) channel block and walks a list of
// 8x8 tiles of the small image.  Per tile the big halo tile [19x19][32] and the small tile [64][32] are staged in LDS
// once; wave w accumulates taps {w, w+4, ...} (7/6/6/6 independent 32x32 accumulators), contraction = the 64
// positions of the tile (A[m=cb][k=pos], B[k=pos][n=cs]: both read from LDS with conflict-free ds_read_b32).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv5_w_kernel(const ConvWArgs a, int tiles_per_split, int total_tiles) {
    constexpr int TH = 8, TW = 8, IH = 2 * TH + 3, IW = 2 * TW + 3, CK = 32, CQ = CK / 4, NT = 256;
    __shared__ __attribute__((aligned(16))) float sBig[IH * IW * CK];
    __shared__ __attribute__((aligned(16))) float sSmall[TH * TW * CK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int cb0 = blockIdx.x * 32, cs0 = blockIdx.y * 32;
    const int tilesx = d.WS / TW, tilesy = d.HS / TH;
    const int t_begin = blockIdx.z * tiles_per_split;
    const int t_end = min(t_begin + tiles_per_split, total_tiles);

    // this thread's channel quad is the same for every float4 it stages (NT % CQ == 0)
    const int cq = tid % CQ;
    const bool xfa = a.xfb.scale != nullptr, xfs = a.xfs.scale != nullptr;
    float4 scA = make_float4(1, 1, 1, 1), shA = make_float4(0, 0, 0, 0), scB = scA, shB = shA;
    if (xfa) {
        scA = *reinterpret_cast<const float4*>(a.xfb.scale + cb0 + cq * 4);
        shA = *reinterpret_cast<const float4*>(a.xfb.shift + cb0 + cq * 4);
        scA.x *= a.xfb.mult; scA.y *= a.xfb.mult; scA.z *= a.xfb.mult; scA.w *= a.xfb.mult;
    }
    if (xfs) {
        scB = *reinterpret_cast<const float4*>(a.xfs.scale + cs0 + cq * 4);
        shB = *reinterpret_cast<const float4*>(a.xfs.shift + cs0 + cq * 4);
        scB.x *= a.xfs.mult; scB.y *= a.xfs.mult; scB.z *= a.xfs.mult; scB.w *= a.xfs.mult;
    }

    // taps of this wave and their LDS offsets: taps {w, w+4, .., w+20} in full, and the 25th tap (24) for one quarter of
    // the tile's positions per wave (its four partial tiles are folded through LDS at the end) -> perfectly balanced
    constexpr int MAXT = 7;
    int aaddr[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        const int tap = (j < MAXT - 1) ? wave + 4 * j : 24;
        const int ky = tap / 5, kx = tap % 5;
        aaddr[j] = ((ky * IW + kx) + 2 * lh) * CK + l31;   // + lane part: pixel x offset 2*lh, channel l31
    }
    const int baddr = lh * CK + l31;

    v16f acc[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    for (int t = t_begin; t < t_end; ++t) {
        const int tx0 = (t % tilesx) * TW;
        const int ty0 = ((t / tilesx) % tilesy) * TH;
        const int n = t / (tilesx * tilesy);
        const float* bigb = a.big + (size_t)n * d.HB * d.WB * d.CB + cb0;
        const float* smb = a.small_ + ((size_t)(n * d.HS + ty0) * d.WS + tx0) * d.CS + cs0;
        const int gy0 = 2 * ty0 - 1, gx0 = 2 * tx0 - 1;
        __syncthreads();   // previous tile fully consumed
        {
            constexpr int TOT = IH * IW * CQ;   // 2888 float4
            constexpr int BATCH = 6;
            for (int f0 = tid; f0 < TOT; f0 += NT * BATCH) {
                float4 v[BATCH];
                bool ok[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int f = f0 + u * NT;
                    const int pix = f / CQ;
                    const int iy = pix / IW, ix = pix % IW;
                    const int gy = gy0 + iy, gx = gx0 + ix;
                    ok[u] = (f < TOT) && (unsigned)gy < (unsigned)d.HB && (unsigned)gx < (unsigned)d.WB;
                    const int gp = ok[u] ? (gy * d.WB + gx) : 0;
                    v[u] = *reinterpret_cast<const float4*>(bigb + (size_t)gp * d.CB + cq * 4);
                }
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int f = f0 + u * NT;
                    if (f >= TOT) continue;
                    float4 tv = v[u];
                    if (xfa) tv = xform4(tv, scA, shA, a.xfb.alpha);
                    *reinterpret_cast<float4*>(sBig + (f / CQ) * CK + cq * 4) = keep4(ok[u], tv);
                }
            }
            // small tile: 64 positions x 8 quads = 512 float4 -> 2 per thread
            float4 sv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int f = tid + u * NT;
                const int pos = f / CQ;
                sv[u] = *reinterpret_cast<const float4*>(smb + (size_t)((pos / TW) * d.WS + (pos % TW)) * d.CS + cq * 4);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int f = tid + u * NT;
                float4 tv = sv[u];
                if (xfs) tv = xform4(tv, scB, shB, a.xfs.alpha);
                *reinterpret_cast<float4*>(sSmall + (f / CQ) * CK + cq * 4) = tv;
            }
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < TH * TW / 2; ++st) {
            // positions 2*st + lh: row st/4, column 2*(st%4) + lh
            const int cst = ((2 * (st / 4)) * IW + 4 * (st % 4)) * CK;
            const float bv = sSmall[baddr + (2 * st) * CK];
#pragma unroll
            for (int j = 0; j < MAXT - 1; ++j) {
                const float av = sBig[aaddr[j] + cst];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
            }
            if ((st >> 3) == wave) {   // wave-uniform: this wave's quarter of tap 24
                const float av = sBig[aaddr[MAXT - 1] + cst];
                acc[MAXT - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[MAXT - 1], 0, 0, 0);
            }
        }
    }

    float* out = a.partial + (size_t)blockIdx.z * a.Mtot * d.CS;
#pragma unroll
    for (int j = 0; j < MAXT - 1; ++j) {
        const int tap = wave + 4 * j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cb = cb0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            out[((size_t)tap * d.CB + cb) * d.CS + cs0 + l31] = acc[j][r];
        }
    }
    // tap 24: fixed-order sum of the four waves' quarter-tile partials
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) sBig[(wave * 16 + r) * 64 + lane] = acc[MAXT - 1][r];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = (sBig[r * 64 + lane] + sBig[(16 + r) * 64 + lane]) + (sBig[(32 + r) * 64 + lane] + sBig[(48 + r) * 64 + lane]);
            const int cb = cb0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            out[((size_t)24 * d.CB + cb) * d.CS + cs0 + l31] = v;
        }
    }
}



// Transpose-read form (round 4).  gfx950's ds_read_b64_tr_b16 gathers, per 16-lane group, four rows of 16 bf16 columns -- each lane supplies the
// 8-byte-aligned address of four CONTIGUOUS columns of one row, row stride free -- and hands lane j column j's four row values (probe:
// tools/tr_probe.hip, profiles/r04_g_tr_probe.log).  With rows = positions and columns = channels that IS the W-kind MFMA fragment (lane = channel,
// eight consecutive positions per lane = two reads), read straight from a PIXEL-major tile: lane (i = l & 15, chalf = (l >> 4) & 1, lh = l >> 5) points
// at pixel (2 (2 js + lh) + ky, 2 (4 t + i / 4) + kx), channels 16 chalf + 4 (i & 3) .. + 3.  The big halo and the small tile are therefore staged
// exactly as the F-kind kernels stage theirs -- two 8-byte LDS stores per float4 instead of eight 2-byte scatter stores with their shifts -- and the
// taps need no segment shifting (v_alignbit) at all.  Bank check: the four rows of a group sit 160 B (big, pixel stride 2) / 144 B (small) apart,
// 32 B each: dword banks [0-7] [40-47] [16-23] [56-63] / [0-7] [36-43] [8-15] [44-51], disjoint.  Tap-to-wave assignment: wave w of a cs block owns kernel row w's
// five taps + tap (4, w) + a quarter of tap (4, 4) (folded through LDS in a fixed order); one [25][CB][CS] slab per workgroup, summed in split order by
// reduce_partials_kernel.  (Its predecessors -- the pixel-major gather kernel of round 2 and the channel-major scatter kernel of round 3, same bits -- were
// dropped in round 6; git history has them.)
template <int NCSB, bool FBB, bool XFA, bool XFS, int NPL = 2, bool DB = false>      // NPL: bf16 planes per operand (2: bf16x3 products, 3: bf16x6); DB: double-buffered tiles
__global__ void __launch_bounds__(256 * NCSB) __attribute__((amdgpu_waves_per_eu(2)))
conv5_w_bf16_tr_kernel(const ConvWArgs a, int tiles_per_split, int total_tiles) {
    // Round 6 ("VALU diet"): the staging half of this kernel issued ~45 VALU instructions per 16 bytes staged, a third of them 64-bit pointer
    // arithmetic and border compares redone per element in BOTH the load-issue and the convert phase, chopped into ~40 basic blocks per tile by
    // run-time switches (activation-on-load or not, tuning ablations, phase clocks).  Now: the switches are template parameters (one straight-line
    // block per phase); every tile-invariant quantity of a thread's elements is computed ONCE before the tile loop -- per-element byte offsets
    // (the loads go through buffer descriptors: wave-uniform base + wave-uniform tile offset + 32-bit lane offset, no 64-bit VALU), four
    // border-class bit masks, the transform rows of the thread's channel quad (registers, not LDS re-reads), LDS store addresses (one base +
    // instruction immediates); the tile coordinates advance incrementally (no divisions); the halo's zero padding comes from the descriptor's
    // range check (an out-of-image element's offset is replaced by 2^31 = the descriptor's size) and costs a select per VALUE only where an activation is applied on load.
    // Same elements to the same threads, same arithmetic per element, same MFMA order: the slabs are bit-identical to round 5's.
    constexpr int TH = 8, TW = 8, IH = 2 * TH + 3, IW = 2 * TW + 3, CK = 32, CQ = CK / 4, NT = 256 * NCSB, CSQ = 8 * NCSB;
    constexpr int LDH = CK + 8;                   // ushorts per big pixel (80 B: 64 B of channels + 16 B pad)
    constexpr int BIGP = IH * IW * LDH;           // ushorts per plane
    constexpr int LDQ = 32 * NCSB + 8;            // ushorts per small position (144 B at NCSB = 2)
    static_assert(!(FBB && XFA), "the pattern-word form replaces the big operand's transform");
    typedef short v4s __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    // DB (round 6, the eight-wave 64-column instances in bf16x3): both tiles double-buffered -- tile t + 1 is converted into the other buffer between the
    // second and the third position block of tile t's MFMAs, the global loads of tile t + 2 follow it, ONE barrier per tile.  (Round 4 measured this neutral on
    // the pre-diet kernel, profiles/r04_h_w_tr_ab.log; on the straight-line tile body it is what it was worth on the k3 kernel: profiles/r06_g_k3_forms.md.)
    // Same elements, same products, same order: bit-identical slabs.
    constexpr int SMALLP = TH * TW * LDQ;         // ushorts per small plane
    constexpr int BUFU = NPL * BIGP + NPL * SMALLP;      // ushorts per buffer
    unsigned short* bPl = reinterpret_cast<unsigned short*>(dsm);       // NPL big planes, then NPL small planes (DB: twice)
    unsigned short* sPlT = bPl + NPL * BIGP;
    float* sRed = reinterpret_cast<float*>(dsm);   // reused after the tile loop

    const unsigned long long dbg_t0 = a.dbgbuf ? wall_clock64() : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave_all = tid >> 6;
    const int wave = wave_all & 3;   // kernel row of this wave's taps
    const int csb = wave_all >> 2;    // its cs block
    const int l31 = lane & 31, lh = lane >> 5;
    const UadConvDesc& d = a.d;
    const int cb0 = blockIdx.x * 32, cs0 = blockIdx.y * 32 * NCSB;
    const int tilesx = d.WS / TW, tilesy = d.HS / TH;
    const int t_begin = blockIdx.z * tiles_per_split;
    const int t_end = min(t_begin + tiles_per_split, total_tiles);

    // ---- this thread's share of a tile: elements (pixel pix0 + u DP, channel quad cq), u < PER, of the 19 x 19 halo; (position pos0 + 32 u,
    // channel quad csq), u < SPER, of the 8 x 8 small tile.  Everything below is the same for every tile. ----
    constexpr int TOT = IH * IW * CQ;
    constexpr int PER = (TOT + NT - 1) / NT;          // 16-byte elements of the big tile per thread: 12 (NT 256) or 6 (NT 512)
    constexpr int DP = NT / CQ;                       // pixels between a thread's consecutive elements
    constexpr int SPER = TH * TW * CSQ / NT;          // 16-byte elements of the small tile per thread (2)
    static_assert(NT % CQ == 0 && NT % CSQ == 0 && (PER - 1) * DP < IH * IW, "only a thread's LAST element can fall off the tile");
    const int cq = tid % CQ, pix0 = tid / CQ;
    const int csq = tid % CSQ, pos0 = tid / CSQ;
    unsigned voff[PER];                               // byte offset of element u from the halo's origin pixel (FBB: of its pixel's 4-byte word)
    unsigned clsT = 0, clsB = 0, clsL = 0, clsR = 0;  // bit u: element u lies in halo row 0 | rows 17, 18 | column 0 | columns 17, 18
    const unsigned pixbytes = FBB ? 4u : (unsigned)d.CB * 4u;
    const unsigned chanbytes = FBB ? 0u : (unsigned)(cb0 + cq * 4) * 4u;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int p = pix0 + u * DP, iy = p / IW, ix = p % IW;
        const bool valid = u + 1 < PER || p < IH * IW;
        voff[u] = valid ? (unsigned)(iy * d.WB + ix) * pixbytes + chanbytes : 0x80000000u;
        clsT |= (iy == 0 ? 1u : 0u) << u; clsB |= (iy >= IH - 2 ? 1u : 0u) << u;
        clsL |= (ix == 0 ? 1u : 0u) << u; clsR |= (ix >= IW - 2 ? 1u : 0u) << u;
    }
    // LDS byte address of element u's hi store = lds_b + u * DP * LDH * 2 (an instruction immediate); the lo plane is BIGP * 2 bytes further.  A thread
    // whose last element is off the tile stores it into pixel 0's pad bytes (never read) instead of branching around the store.
    const unsigned lds_b = (unsigned)(pix0 * LDH + cq * 4) * 2u;
    const bool last_valid = pix0 + (PER - 1) * DP < IH * IW;
    const unsigned lds_last = last_valid ? lds_b + (unsigned)((PER - 1) * DP * LDH) * 2u : (unsigned)CK * 2u;
    unsigned svoff[SPER];
#pragma unroll
    for (int u = 0; u < SPER; ++u) {
        const int pos = pos0 + u * (NT / CSQ);
        svoff[u] = (unsigned)(((pos / TW) * d.WS + (pos % TW)) * d.CS + cs0 + csq * 4) * 4u;
    }
    const unsigned slds_b = (unsigned)(pos0 * LDQ + csq * 4) * 2u;       // + u * 32 * LDQ * 2; lo plane TH * TW * LDQ * 2 bytes further

    // activation-on-load rows of this thread's channel quads (registers)
    float4 bsc = make_float4(1.f, 1.f, 1.f, 1.f), bsh = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ssc = bsc, ssh = bsh;
    if (XFA) {
        const float4 g = *reinterpret_cast<const float4*>(a.xfb.scale + cb0 + cq * 4);
        bsc = make_float4(g.x * a.xfb.mult, g.y * a.xfb.mult, g.z * a.xfb.mult, g.w * a.xfb.mult);
        bsh = *reinterpret_cast<const float4*>(a.xfb.shift + cb0 + cq * 4);
    }
    if (XFS) {
        const float4 g = *reinterpret_cast<const float4*>(a.xfs.scale + cs0 + csq * 4);
        ssc = make_float4(g.x * a.xfs.mult, g.y * a.xfs.mult, g.z * a.xfs.mult, g.w * a.xfs.mult);
        ssh = *reinterpret_cast<const float4*>(a.xfs.shift + cs0 + csq * 4);
    }
    const float balpha = a.xfb.alpha, salpha = a.xfs.alpha;
    // Pattern-word form: element = (dxhat * w_f[ch]) * (bit ch ? scale : scale * alpha).  (Round 6 also tried the four selects of a channel quad as ONE
    // 16-byte LDS table row indexed by the quad's nibble of the word -- 133 fewer VALU instructions per tile and wave, same bits -- and measured it
    // SLOWER: dec3.wgrad 0.86 -> 0.89-0.91 of the round-5 kernel's time, with or without bank padding: profiles/r06_b_fb_nibble_table_ab.md.)
    float fb_wf[4] = {0.f, 0.f, 0.f, 0.f}, fb_s1[4] = {0.f, 0.f, 0.f, 0.f}, fb_s0[4] = {0.f, 0.f, 0.f, 0.f};
    if (FBB) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            fb_wf[e] = a.xfb.fb_wf[cb0 + cq * 4 + e];
            fb_s1[e] = a.xfb.scale[cb0 + cq * 4 + e] * a.xfb.mult;
            fb_s0[e] = fb_s1[e] * a.xfb.alpha;
        }
    }
    const unsigned fb_shift = (unsigned)(cb0 + cq * 4);

    constexpr int MAXT = 7;
    // fragment addressing (ushort indices): group g = lane >> 4 -> channel half g & 1, position half lh = g >> 1; lane i of the group -> row i >> 2
    // of the 4-position block, columns 4 (i & 3)
    const int li = lane & 15, chalf = (lane >> 4) & 1;
    const int a_base = ((2 * lh) * IW + 2 * (li >> 2)) * LDH + 16 * chalf + 4 * (li & 3);      // + (4 js IW + ky IW + kx + 8 t) LDH
    const int b_base = (8 * lh + (li >> 2)) * LDQ + csb * 32 + 16 * chalf + 4 * (li & 3);        // + (16 js + 4 t) LDQ

    v16f acc[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    auto tr8 = [&](const unsigned short* plane, const int addr, const int step) __attribute__((always_inline)) {      // 8 consecutive k of this lane's channel
        const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(const_cast<unsigned short*>(plane) + addr));
        const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(const_cast<unsigned short*>(plane) + addr + step));
        const uint2 lo2 = __builtin_bit_cast(uint2, r0), hi2 = __builtin_bit_cast(uint2, r1);
        return make_uint4(lo2.x, lo2.y, hi2.x, hi2.y);
    };
    struct Pl { uint4 p[NPL]; };
    auto trp = [&](const unsigned short* planes, const int plane_stride, const int addr, const int step) __attribute__((always_inline)) {
        Pl r;
#pragma unroll
        for (int p = 0; p < NPL; ++p) r.p[p] = tr8(planes + p * plane_stride, addr, step);
        return r;
    };
    auto mma3 = [&](v16f& c, const Pl& a_, const Pl& b_) __attribute__((always_inline)) {
        c = mfma_bf16(a_.p[0], b_.p[0], c);
        c = mfma_bf16(a_.p[0], b_.p[1], c);
        c = mfma_bf16(a_.p[1], b_.p[0], c);
        if constexpr (NPL == 3) {      // bf16x6: + a0 b2, a2 b0, a1 b1
            c = mfma_bf16(a_.p[0], b_.p[2], c);
            c = mfma_bf16(a_.p[2], b_.p[0], c);
            c = mfma_bf16(a_.p[1], b_.p[1], c);
        }
    };

    // ---- tile loop, software-pipelined: the global loads of tile t + 1 are in flight while tile t is contracted ----
    uint4 v[FBB ? 1 : PER];
    unsigned vb[FBB ? PER : 1];
    float vg[FBB ? PER : 1];
    uint4 sv[SPER];
    // coordinates of the NEXT tile to be issued (wave-uniform, advanced incrementally)
    int nx_tx0 = (t_begin % tilesx) * TW, nx_ty0 = ((t_begin / tilesx) % tilesy) * TH, nx_n = t_begin / (tilesx * tilesy);
    unsigned bad = 0;            // bit u: element u of the tile in flight is outside the image
    const size_t big_img = (size_t)d.HB * d.WB * (FBB ? 1 : d.CB);          // elements of one sample of the big operand (FBB: of the per-pixel words)
    const size_t origin_back = (size_t)(d.WB + 1) * (FBB ? 1 : d.CB);      // the halo's origin is one row and one column before the tile's first pixel
    auto issue = [&]() __attribute__((always_inline)) {
        const int tx0 = nx_tx0, ty0 = nx_ty0, n = nx_n;
        bad = ((ty0 == 0) ? clsT : 0u) | ((ty0 + TH == d.HS) ? clsB : 0u) | ((tx0 == 0) ? clsL : 0u) | ((tx0 + TW == d.WS) ? clsR : 0u);
        const unsigned tile_b = (unsigned)((2 * ty0) * d.WB + 2 * tx0) * pixbytes;
        if (FBB) {
            const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<unsigned*>(a.xfb.fb_bits) + (size_t)n * big_img - origin_back), 0, 0x80000000u, 0x00020000);
            const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.xfb.fb_dxhat) + (size_t)n * big_img - origin_back), 0, 0x80000000u, 0x00020000);
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const unsigned off = (bad >> u) & 1u ? 0x80000000u : voff[u];
                vb[FBB ? u : 0] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rb, (int)off, (int)tile_b, 0);
                vg[FBB ? u : 0] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(rg, (int)off, (int)tile_b, 0));
            }
        } else {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.big) + (size_t)n * big_img - origin_back), 0, 0x80000000u, 0x00020000);
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const unsigned off = (bad >> u) & 1u ? 0x80000000u : voff[u];
                v[FBB ? 0 : u] = buf_load16(rs, off, tile_b);
            }
        }
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)(const_cast<float*>(a.small_) + ((size_t)(n * d.HS + ty0) * d.WS + tx0) * d.CS), 0, 0x80000000u, 0x00020000);
#pragma unroll
        for (int u = 0; u < SPER; ++u) sv[u] = buf_load16(rq, svoff[u], 0);
        nx_tx0 += TW;
        if (nx_tx0 == d.WS) { nx_tx0 = 0; nx_ty0 += TH; if (nx_ty0 == d.HS) { nx_ty0 = 0; ++nx_n; } }
    };
    auto as_f4 = [](uint4 q) { return make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)); };
    auto lds_store8 = [&](unsigned byte_addr, uint2 q) __attribute__((always_inline)) { *reinterpret_cast<uint2*>(dsm + byte_addr) = q; };
    auto commit = [&](const unsigned bufb) __attribute__((always_inline)) {      // bufb: byte offset of the buffer written
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            float4 tv;
            if (FBB) {
#pragma clang fp contract(off)      // (the products are ROUNDED before the hi | lo split subtracts from them, as in round 5 where a select stood between the two)
                const unsigned b = vb[FBB ? u : 0] >> fb_shift;
                const float gq = vg[FBB ? u : 0];      // 0 outside the image (descriptor range check): the products below are zeros
                tv.x = gq * fb_wf[0] * ((b & 1u) ? fb_s1[0] : fb_s0[0]);
                tv.y = gq * fb_wf[1] * ((b & 2u) ? fb_s1[1] : fb_s0[1]);
                tv.z = gq * fb_wf[2] * ((b & 4u) ? fb_s1[2] : fb_s0[2]);
                tv.w = gq * fb_wf[3] * ((b & 8u) ? fb_s1[3] : fb_s0[3]);
            } else {
                tv = as_f4(v[FBB ? 0 : u]);
                if (XFA) tv = keep4(!((bad >> u) & 1u), xform4(tv, bsc, bsh, balpha));      // padding is zero AFTER the activation
            }
            uint2 pl[NPL];
            split_planes<NPL>(tv, pl);
            const unsigned o = (u + 1 < PER) ? lds_b + (unsigned)(u * DP * LDH) * 2u : lds_last;
#pragma unroll
            for (int p = 0; p < NPL; ++p) lds_store8(bufb + o + (unsigned)(p * BIGP) * 2u, pl[p]);
        }
#pragma unroll
        for (int u = 0; u < SPER; ++u) {
            float4 tv = as_f4(sv[u]);
            if (XFS) tv = xform4(tv, ssc, ssh, salpha);
            uint2 pl[NPL];
            split_planes<NPL>(tv, pl);
            const unsigned o = (unsigned)(NPL * BIGP) * 2u + slds_b + (unsigned)(u * (NT / CSQ) * LDQ) * 2u;
#pragma unroll
            for (int p = 0; p < NPL; ++p) lds_store8(bufb + o + (unsigned)(p * SMALLP) * 2u, pl[p]);
        }
    };
    if (t_begin < t_end) {
        issue();
        if (DB) { commit(0u); if (t_begin + 1 < t_end) issue(); __syncthreads(); }
    }
    for (int t = t_begin; t < t_end; ++t) {
        const int cur = DB ? ((t - t_begin) & 1) * BUFU : 0;      // ushort offset of the buffer read
        if (!DB) {
            __syncthreads();                   // the previous tile's fragments are consumed
            commit(0u);
            if (t + 1 < t_end) issue();        // in flight across the barrier and the MFMA loop below
            __syncthreads();
        }
        const unsigned short* bP = bPl + cur;
        const unsigned short* sP = sPlT + cur;
#pragma unroll
        for (int js = 0; js < TH * TW / 16; ++js) {
            // positions 16 js .. 16 js + 15 = tile rows 2 js (k half 0) and 2 js + 1 (k half 1)
            const int bo = b_base + 16 * js * LDQ;
            const Pl bq_ = trp(sP, SMALLP, bo, 4 * LDQ);
            const int ao = a_base + (4 * js * IW + wave * IW) * LDH;          // this wave's kernel row
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) mma3(acc[kx], trp(bP, BIGP, ao + kx * LDH, 8 * LDH), bq_);
            const int a4 = a_base + (4 * js * IW + 4 * IW) * LDH;             // kernel row 4
            mma3(acc[5], trp(bP, BIGP, a4 + wave * LDH, 8 * LDH), bq_);        // tap (4, wave)
            if (DB && js == 1) {
                // tile t + 1 (in registers since tile t - 1's MFMAs) -> the other buffer; then the loads of tile t + 2
                __builtin_amdgcn_sched_barrier(0);
                if (t + 1 < t_end) { commit((unsigned)(BUFU - cur) * 2u); if (t + 2 < t_end) issue(); }      // (unconditional, clamped forms measured the same)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        {
            // this wave's quarter of tap (4, 4) = position block js = wave, addressed by a run-time offset BEHIND the straight-line loop: with the
            // `if (js == wave)` inside it (round 4) every js step was its own basic block and the fragment reads of a block could not be hoisted
            // above the previous block's MFMAs.  acc[6] receives the same three products in the same order.
            const int bo = b_base + 16 * wave * LDQ;
            const int a4 = a_base + (4 * wave * IW + 4 * IW) * LDH;
            mma3(acc[6], trp(bP, BIGP, a4 + 4 * LDH, 8 * LDH), trp(sP, SMALLP, bo, 4 * LDQ));
        }
        if (DB) __syncthreads();          // tile t + 1 is complete in LDS, and every wave is done with tile t's buffer
    }

    // Accumulator block -> slab.  One 64-bit address per lane; everything else is a wave-uniform 32-bit offset (the plain form
    // `out[((size_t)tap * CB + cb) * CS + col]` cost ~400 quarter-rate 64-bit multiply-adds per wave: 8 of this kernel's ~47 us).
    const int CSi = d.CS;
    float* ob = a.partial + (size_t)blockIdx.z * a.Mtot * CSi + (size_t)(cb0 + 4 * lh) * CSi + cs0 + csb * 32 + l31;
    const int tapstride = d.CB * CSi;
    if (a.abl & 32) {       // stress test (tests/test_gpu_knobs.py): every workgroup idles ~100 us before it writes its slab, so that the filter gradient
                            // OUTLASTS the any-order data gradient launched behind it -- results stay correct, only the timing changes
        for (int i = 0; i < 32; ++i) __builtin_amdgcn_s_sleep(127);
    }
#pragma unroll
    for (int j = 0; j < MAXT - 1; ++j) {
        const int tap = j < 5 ? 5 * wave + j : 20 + wave;      // (row, 0..4), (4, row)
        float* ot = ob + tap * tapstride;
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[((r & 3) + 8 * (r >> 2)) * CSi] = acc[j][r];
    }
    // tap (4, 4): the four rows' shares are folded through LDS in a fixed order
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) sRed[((csb * 4 + wave) * 16 + r) * 64 + lane] = acc[MAXT - 1][r];
    __syncthreads();
    if (wave == 0) {
        float* ot = ob + 24 * tapstride;
        const float* q = sRed + (size_t)csb * 64 * 64;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            ot[((r & 3) + 8 * (r >> 2)) * CSi] = (q[r * 64 + lane] + q[(16 + r) * 64 + lane]) + (q[(32 + r) * 64 + lane] + q[(48 + r) * 64 + lane]);
    }
    if (a.dbgbuf && tid == 0) {
        const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.dbgbuf[2 * b] = dbg_t0;
        a.dbgbuf[2 * b + 1] = wall_clock64();
    }
}

constexpr size_t conv5_w_bf16_tr_lds_bytes(int ncsb, int npl = 2) { return (size_t)npl * 19 * 19 * 40 * 2 + (size_t)npl * 64 * (32 * ncsb + 8) * 2 + 192 * 4; }

template <int NCSB, bool FBB, bool XFA, bool XFS, int NPL>
void launch_w_tr_n(const ConvWArgs& a, dim3 grid, const W5Choice& w5, bool any_order, hipStream_t st) {
    if constexpr (NCSB == 2 && NPL == 2) {
        // double-buffered form: 2 x 76 KB of LDS, one eight-wave workgroup per CU as before (UAD_NO_W5_DB: the single-buffered loop)
        static const bool nodb = getenv("UAD_NO_W5_DB") != nullptr;
        if (!nodb) {
            constexpr size_t ldsd = 2 * conv5_w_bf16_tr_lds_bytes(NCSB, NPL);
            static bool attrd = false;
            if (!attrd) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_w_bf16_tr_kernel<NCSB, FBB, XFA, XFS, NPL, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsd); attrd = true; }
            UAD_W_LAUNCH(any_order, (conv5_w_bf16_tr_kernel<NCSB, FBB, XFA, XFS, NPL, true>), grid, dim3(256 * NCSB), ldsd, st, a, w5.tiles_per_split, w5.total_tiles);
            return;
        }
    }
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_w_bf16_tr_kernel<NCSB, FBB, XFA, XFS, NPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv5_w_bf16_tr_lds_bytes(NCSB, NPL)); attr = true; }
    UAD_W_LAUNCH(any_order, (conv5_w_bf16_tr_kernel<NCSB, FBB, XFA, XFS, NPL>), grid, dim3(256 * NCSB), conv5_w_bf16_tr_lds_bytes(NCSB, NPL), st, a, w5.tiles_per_split, w5.total_tiles);
}
template <int NCSB, bool FBB, bool XFA, bool XFS>
void launch_w_tr(const ConvWArgs& a, dim3 grid, const W5Choice& w5, bool any_order, hipStream_t st) {
    if constexpr (FBB ? XFS : (XFA != XFS)) { if (a.npl == 3) { launch_w_tr_n<NCSB, FBB, XFA, XFS, 3>(a, grid, w5, any_order, st); return; } }
    launch_w_tr_n<NCSB, FBB, XFA, XFS, 2>(a, grid, w5, any_order, st);
}
}  // namespace

void uad_conv5_w16_launch(const ConvWArgs& a, dim3 grid, int ncsb, bool fbb, bool xa, bool xs, const W5Choice& w5, bool any_order, hipStream_t st) {
    const bool two = ncsb == 2;
    // <cs blocks per workgroup, big operand from the pattern word, activation on load of big, ... of small>
    if (fbb) { if (two) { if (xs) launch_w_tr<2, true, false, true>(a, grid, w5, any_order, st); else launch_w_tr<2, true, false, false>(a, grid, w5, any_order, st); }
               else     { if (xs) launch_w_tr<1, true, false, true>(a, grid, w5, any_order, st); else launch_w_tr<1, true, false, false>(a, grid, w5, any_order, st); } }
    else if (two) { if (xa) { if (xs) launch_w_tr<2, false, true, true>(a, grid, w5, any_order, st); else launch_w_tr<2, false, true, false>(a, grid, w5, any_order, st); }
                    else    { if (xs) launch_w_tr<2, false, false, true>(a, grid, w5, any_order, st); else launch_w_tr<2, false, false, false>(a, grid, w5, any_order, st); } }
    else          { if (xa) { if (xs) launch_w_tr<1, false, true, true>(a, grid, w5, any_order, st); else launch_w_tr<1, false, true, false>(a, grid, w5, any_order, st); }
                    else    { if (xs) launch_w_tr<1, false, false, true>(a, grid, w5, any_order, st); else launch_w_tr<1, false, false, false>(a, grid, w5, any_order, st); } }
}

void uad_conv5_w32_launch(const ConvWArgs& a, dim3 grid, const W5Choice& w5, hipStream_t st) {
    hipLaunchKernelGGL(conv5_w_kernel, grid, dim3(256), 0, st, a, w5.tiles_per_split, w5.total_tiles);
}
