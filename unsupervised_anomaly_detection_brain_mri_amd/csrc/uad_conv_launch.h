// The boundary between the conv planner (uad_conv_plan.hip: host only, decides the instance of every uad_launch_conv_* call) and the kernel units, one
// per family, that own the instances: the argument blocks, which cross it by typed reference, and each family's launch functions, which take the
// selectors the planner decided.  None of this is exported (include/uad_hip.h is the library's surface).
#pragma once
#include <hip/hip_runtime.h>
#include "uad_kernels.h"

#define KIND_F 0
#define KIND_D 1

constexpr int XF_LDS_CH = 512;  // activation-on-load tables (gamma', beta) staged once per workgroup

struct ConvGemmArgs {
    const float* A;
    const float* W;
    const float* Wp;   // k-quad-interleaved copy of W for the spatial kernels (uad_launch_pack_weights)
    const unsigned short* Wp16;   // bf16 hi|lo planes, k-octet-interleaved (bf16x3 math mode)
    long long w16_plane;          // elements per plane
    float* Out;
    UadXform xf;
    UadEpilogue ep;
    UadConvDesc d;
    int M;         // N*HS*WS rows (small-image positions)
    int CA;        // channels of the A operand (contraction per tap)
    int Nn;        // output channels
    int lws, lhs;  // log2(WS), log2(HS) or -1 when not a power of two
    int nsplit;    // split-K factor (>1: raw partial tiles go to Out + split*out_elems, see splitk_epilogue_kernel)
    long long out_elems;
    unsigned* sk_counter;   // split-K with in-kernel reduction: arrival counters, one per (spatial tile, column block); null = splitk_epilogue_kernel
    float* out_final;       // ... and the real output (Out points at the slabs)
    unsigned long long* dbgbuf;   // per-phase clock stamps of a few workgroups (UAD_DBG & 8)
    int dbg;       // ablation switches for kernel tuning (UAD_DBG): 1 = no epilogue stores, 2 = no MFMA loop, 4 = no staging
    int math16;    // generic kernel: bf16x3 products (conv_gemm16_kernel) where the tile shape allows
    int npl = 2;   // bf16 planes behind Wp16 (2: bf16x3, 3: bf16x6 -- the F-kind and lane = pixel spatial kernels only)
};

// W-type: filter gradient.  GEMM M = (tap, cb) flattened, N = cs, K = positions (split over blockIdx.z).
struct ConvWArgs {
    const float* big;
    const float* small_;
    float* partial;
    UadXform xfb, xfs;
    UadConvDesc d;
    int Mtot;  // KS*KS*CB
    int Kt;    // N*HS*WS
    int kper;  // positions per split (multiple of BK)
    int lws, lhs;
    unsigned long long* dbgbuf;   // UAD_DBG & 32: per-workgroup start / end clocks
    int npl = 2;   // bf16 planes per operand of the k5 s2 kernel (2: bf16x3 products, 3: bf16x6)
    int abl = 0;   // UAD_W_ABL, kernel-tuning ablations (results are wrong): 1 no big-tile LDS stores | 2 no MFMAs | 4 no big-tile global loads | 8 no slab stores;
                   // 32 (results stay right): every workgroup sleeps before its slab store (ordering stress test)
};

// the k3 tap-list kernels (uad_convk16.inc)
struct ConvKArgs {
    const float* A;               // input [N, AH, AW, CA]
    const unsigned short* Wp16;   // hi plane of the tensor in the packed layout [tap][CA / 8][Nn][8]; the lo plane follows w16_plane elements later
    long long w16_plane;
    float* Out;                   // [N, OH, OW, Nn]
    const float* bias;            // [Nn] or null
    const float* add;             // layout of Out, or null
    int N, AH, AW, CA;
    int MH, MW;                   // iteration grid
    int OH, OW, Nn;
    int os, oy, ox;
    int y0, x0;                   // input pixel of halo element (0, 0) for the tile at the grid origin
    int toff[9];                  // per tap: hy * IW + hx inside the halo (IW = the instance's halo width)
    int widx[9];                  // per tap: its index in the weight tensor
};

// what the planner's choosers hand to a filter-gradient launch
struct W5Choice { bool ok; int splits, tiles_per_split, total_tiles; };
struct WK3Choice { bool ok; int ncb, splits, tiles_per_split, total_tiles; };

// block tile of the generic kernels: the planner sizes grids and split-K with it, uad_gemm_launch picks the instance by it
struct TileChoice { int BM, BN, BK; };
inline TileChoice choose_tile(long M, int Nn, int CA, int classes) {
    TileChoice t;
    t.BK = (CA % 32 == 0) ? 32 : (CA % 16 == 0) ? 16 : 8;
    t.BN = (Nn > 32) ? 64 : 32;
    auto nwg = [&](int bm) { return ((M + bm - 1) / bm) * ((Nn + t.BN - 1) / t.BN) * classes; };
    t.BM = (t.BK == 32 && nwg(128) >= 512) ? 128 : 64;
    return t;
}

// any_order: launch without the AQL barrier bit (hipExtAnyOrderLaunch).  The request itself lives in the planner (uad_conv_any_order_next /
// uad_conv_w_any_order_next); a launcher that takes the parameter honours it, every other launch is ordered.

// ---- uad_gemm.hip: generic implicit GEMM (any KS / S / P), fp32 and bf16x3; the split-K epilogue; the generic filter gradient
void uad_gemm_launch(const ConvGemmArgs& a, bool f_type, int classes, hipStream_t st);
void uad_gemm_launch_splitk_epilogue(const float* slabs, int nsplit, long long out_elems, int rows, int Nn, const UadEpilogue& ep, float* out, hipStream_t st);
void uad_gemm_launch_w(const ConvWArgs& a, dim3 grid, int BM, int BN, bool w16, hipStream_t st);
// ---- uad_conv5_f.hip: k5 s2 F kind.  bn: output channels per workgroup (64: 8 x 8 tile | 32: 8 x 16); on bf16 planes a.npl picks bf16x3 / bf16x6
void uad_conv5_f16_launch(const ConvGemmArgs& a, dim3 grid, int bn, bool any_order, hipStream_t st);
void uad_conv5_f32_launch(const ConvGemmArgs& a, dim3 grid, int bn, bool any_order, hipStream_t st);
// ---- uad_conv5_d.hip: k5 s2 D kind outside the lane = pixel family.  cst: channel range a workgroup stages whole; ck: channel chunk streamed through LDS
void uad_conv5_d16_launch(const ConvGemmArgs& a, dim3 grid, int bn, int cst, hipStream_t st);
void uad_conv5_dbf16_launch(const ConvGemmArgs& a, dim3 grid, int bn, int ck, hipStream_t st);
void uad_conv5_d32_launch(const ConvGemmArgs& a, dim3 grid, int bn, int ck, bool fin, bool any_order, hipStream_t st);
// ---- uad_gemm_d16s.hip / uad_gemm_d16s3.hip: k5 s2 D kind, lane = pixel (two / three bf16 planes)
bool uad_d16s_takes(const ConvGemmArgs& a);
bool uad_d16s_t16(const ConvGemmArgs& a, int bn, int cst, int npl);
void uad_d16s_launch_v2(const ConvGemmArgs& a, dim3 grid, int bn, int cst, bool any_order, hipStream_t st);
void uad_d16s_launch_v3(const ConvGemmArgs& a, dim3 grid, int bn, int cst, bool any_order, hipStream_t st);
// ---- uad_conv5_w.hip: k5 s2 filter gradient.  ncsb: 32-channel cs blocks per workgroup; fbb: big operand from the pattern word; xa / xs: activation on load
void uad_conv5_w16_launch(const ConvWArgs& a, dim3 grid, int ncsb, bool fbb, bool xa, bool xs, const W5Choice& w5, bool any_order, hipStream_t st);
void uad_conv5_w32_launch(const ConvWArgs& a, dim3 grid, const W5Choice& w5, hipStream_t st);
// ---- uad_conv_k3.hip: k3 / k1 tap-list family.  <sin, ext, ntaps>: input stride, halo extent and tap count of the instance
void uad_k3_launch(const ConvKArgs& a, int sin, int ext, int ntaps, int planes, hipStream_t st);
void uad_k3_launch_k1s2_fill(float* out, const float* bias, const float* add, int OW, int Nn, size_t total4, hipStream_t st);
void uad_k3_launch_w(const ConvWArgs& a, const WK3Choice& c, int S, int ncb, hipStream_t st);
