// The conv layer's planner: host code only.  Every uad_launch_conv_* call and every uad_conv_* query is answered here by one set of decision functions
// (choose_spatial, choose_w5, plan_gemm, x6_route, plan_for, d16_generation, ...); a plan becomes a launch in run_plan / uad_launch_conv_w, which call the launch
// function of the kernel family that owns the instance (uad_conv_launch.h) with the selectors they decided.  No kernel is defined or named in this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uad_conv_launch.h"
#include "uad_conv_k3_plan.h"

// Launches without the AQL barrier bit (hipExtAnyOrderLaunch).  Packets of a queue are still DEQUEUED in order, so such a kernel starts once
// everything before its predecessor has completed (the predecessor's own barrier bit saw to that) -- but it does not wait for the predecessor
// itself.  The backward uses it for the two launches per layer that do not depend on the kernel enqueued right before them: a layer's data
// gradient behind its filter gradient (both read d loss / d c, neither reads the other's output), and the first filter gradient behind the
// forward's single-workgroup loss.finalize.  The successor's workgroups fill the CUs the predecessor's last workgroups are still draining:
// -0.7 % per step (profiles/r03_y_gpurun11/12.log); unlike a second stream (+36 %) the predecessor is dispatched in full first.
// UAD_NO_ANYORDER=1 (read in uad_model.hip) keeps every launch ordered.
// The request is one flag per host thread (another thread's launch must not consume it), set by uad_conv_any_order_next / uad_conv_w_any_order_next and consumed
// by the next launch that honours it, which gets it as its any_order parameter: conv5_f16, conv5_f_kernel, conv5_d_kernel and the lane = pixel family on the
// F / D side, conv5_w_bf16_tr_kernel on the W side.  Every other launch (conv5_d16, conv5_bf16, conv5_w_kernel, the generic and the k3 kernels) is ordered and
// leaves the request standing.
namespace {
thread_local bool g_any_order_next = false;
thread_local bool g_any_order_w_next = false;      // ... the same for the next channel-major filter-gradient launch (the first one of a backward, behind loss.finalize)
inline bool take_request(bool& flag) { const bool on = flag; flag = false; return on; }

// eligibility + tile choice of the spatial kernels (shared by the launchers and the *_tiles() queries)
struct SpatialChoice { bool ok; int TH, TW, BN, CK; };
inline SpatialChoice choose_spatial(const UadConvDesc& d, int CA, int Nn, bool f_type = true) {
    SpatialChoice c{false, 0, 0, 0, 0};
    if (!(d.KS == 5 && d.S == 2 && d.P == 1)) return c;
    if (d.HB != 2 * d.HS || d.WB != 2 * d.WS) return c;
    if (CA > XF_LDS_CH) return c;
    if (Nn % 64 == 0 && CA % 32 == 0 && d.HS % 8 == 0 && d.WS % 8 == 0) { c = SpatialChoice{true, 8, 8, 64, 32}; return c; }
    // 8x16 tile, 32 output channels: the D-type halo (10x18) is small enough for 32-channel chunks, the F-type one is not
    if (Nn % 32 == 0 && CA % 16 == 0 && d.HS % 8 == 0 && d.WS % 16 == 0) {
        c = SpatialChoice{true, 8, 16, 32, (!f_type && CA % 32 == 0) ? 32 : 16};
        return c;
    }
    return c;
}

inline W5Choice choose_w5(const UadConvDesc& d, bool bf16 = true) {
    W5Choice c{false, 0, 0, 0};
    if (!(d.KS == 5 && d.S == 2 && d.P == 1 && d.HB == 2 * d.HS && d.WB == 2 * d.WS)) return c;
    if (d.CB % 32 || d.CS % 32 || d.HS % 8 || d.WS % 8) return c;
    c.total_tiles = d.N * (d.HS / 8) * (d.WS / 8);
    const int blocks = (d.CB / 32) * (d.CS / 32);
    // UAD_W5_TARGET (tuning knob): workgroup-slab target of a launch.  Every split costs one [25][CB][CS] slab written and re-read, every tile
    // ~2.6 us of a workgroup's life.  Default 448 (round 4, profiles/r04_i_w5_target_sweep.log): the kernel itself is fastest at 512 (two
    // workgroups on every CU: dec3.wgrad 61 us, 68 at 448), but the layer's data gradient is launched right behind it without the barrier bit and
    // fills the slots a 410-workgroup filter gradient leaves free -- the STEP is 2.5 % faster (0.916 -> 0.894 ms), and the slabs are a fifth smaller.
    // The exact-fp32 kernel (bf16 = false) is bound by the matrix pipe, not by latency: it keeps 512 (448 cost that mode 4 %: 1.704 -> 1.772 ms).
    static const int target_env = getenv("UAD_W5_TARGET") ? atoi(getenv("UAD_W5_TARGET")) : 0;
    // Round 6, double-buffered kernel: re-swept on two boxes (profiles/r06_i_w5_target_sweep_db.log) -- 384 is 1 % faster over the step than 448 in all four pairs
    // (0.822 / 0.830 vs 0.833 / 0.836 ms; 0.848 / 0.841 vs 0.856 / 0.852), although the kernels' own tags sum to 260 us instead of 250.
    const int target = target_env > 0 ? target_env : (bf16 ? 384 : 512);
    int splits = (target + blocks - 1) / blocks;
    if (splits > c.total_tiles) splits = c.total_tiles;
    if (splits < 1) splits = 1;
    c.tiles_per_split = (c.total_tiles + splits - 1) / splits;
    c.splits = (c.total_tiles + c.tiles_per_split - 1) / c.tiles_per_split;
    c.ok = true;
    return c;
}

inline int ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// split-K factor of the generic kernel: only when the plain grid cannot fill the chip and K is long enough
inline int choose_nsplit(long M, int Nn, int CA, int classes, int min_taps) {
    const TileChoice t = choose_tile(M, Nn, CA, classes);
    const long wgs = ((M + t.BM - 1) / t.BM) * ((Nn + t.BN - 1) / t.BN) * classes;
    const int nk_min = min_taps * (CA / t.BK);
    if (wgs >= 256 || nk_min < 8 || (Nn % 4)) return 1;
    long s = (512 + wgs - 1) / wgs;
    if (s > nk_min / 4) s = nk_min / 4;
    if (s > 16) s = 16;
    return s < 2 ? 1 : (int)s;
}

}  // namespace

namespace {
enum { PATH_GENERIC = 0, PATH_SPATIAL = 1, PATH_SPLITK = 2 };
struct GemmPlan { int path; SpatialChoice sc; int nsplit; int tiles; size_t ws_floats; long long out_elems; int out_rows; bool inkernel; };

// One decision procedure for launchers and for the colpart-tile / workspace queries.
// ncounters > 0: the caller runs the split-bf16 spatial kernels and owns that many arrival counters -> a split launch reduces its slabs in the
// kernel (last workgroup per tile) when the instance that will run supports it
inline GemmPlan plan_gemm(const UadConvDesc& d, bool f_type, bool have_pack, size_t ws_cap, int ncounters = 0) {
    GemmPlan p;
    p.inkernel = false;
    const int CA = f_type ? d.CB : d.CS, Nn = f_type ? d.CS : d.CB;
    const long M = (long)d.N * d.HS * d.WS;
    const int classes = f_type ? 1 : d.S * d.S;
    int min_taps = d.KS * d.KS;
    if (!f_type && d.S > 1) { const int t = d.KS / d.S; min_taps = t * t; }
    p.out_rows = f_type ? (int)M : d.N * d.HB * d.WB;
    p.out_elems = (long long)p.out_rows * Nn;
    p.sc = have_pack ? choose_spatial(d, CA, Nn, f_type) : SpatialChoice{false, 0, 0, 0, 0};
    p.nsplit = 1; p.ws_floats = 0;
    const TileChoice t = choose_tile(M, Nn, CA, classes);
    int ns = choose_nsplit(M, Nn, CA, classes, min_taps);
    if (ns > 1 && (size_t)ns * p.out_elems > ws_cap) ns = 1;
    if (p.sc.ok) {
        // the spatial kernels want >= 2 workgroups per CU (staging / epilogue of one overlaps the MFMA work of the other);
        // if the plain grid is smaller, split the channel chunks over workgroups (slabs + splitk_epilogue_kernel)
        const long wgs = (long)d.N * (d.HS / p.sc.TH) * (d.WS / p.sc.TW) * (Nn / p.sc.BN);
        const int chunks = CA / p.sc.CK;
        int sp = 1;
        // Workgroups a spatial launch is split up to.  Round 4, same-box sweep (profiles/r04_d_split_target_sweep.log): the gather (F) kernels
        // want two workgroups per CU (enc3.fwd 22 us at 512 / 23 at 256 / 30 unsplit); the class-sequential scatter (D) kernels stage their whole
        // channel range once and pay the slab exchange four times (once per parity class): they are faster with HALF the splits (dec0.fwd 30 -> 25,
        // dec1.fwd 37 -> 31, enc3.dgrad 35 -> 31, enc2.dgrad 38 -> 32 us).  UAD_SPLIT_TARGET=n overrides both (tuning knob).
        static const int split_env = getenv("UAD_SPLIT_TARGET") ? atoi(getenv("UAD_SPLIT_TARGET")) : 0;
        const int split_target = split_env > 0 ? split_env : (f_type ? 512 : 256);
        while (wgs * sp < split_target && sp * 2 <= chunks && (size_t)(sp * 2) * p.out_elems <= ws_cap) sp *= 2;
        // Fewest workgroups a spatial launch may have; below it the launch falls back to the generic implicit-GEMM kernel (+ a separate split-K epilogue
        // launch).  Round 5: 128 (was 256): at the 16-slice workloads of BASELINE configs[2] / [4] the 8 x 8 layers come to 128 workgroups after
        // splitting, and the spatial kernel with its in-kernel slab reduction beats generic + epilogue by 2x there (spatial-GMVAE restoration:
        // enc4.fwd 40 -> 16 us, dec0.dgrad 41 -> 17, the iteration 0.699 -> 0.632 ms; profiles/r05_e_planner_min_wgs.log).  UAD_SPATIAL_MIN_WGS=n overrides.
        static const int min_env = getenv("UAD_SPATIAL_MIN_WGS") ? atoi(getenv("UAD_SPATIAL_MIN_WGS")) : 0;
        // (only for SPLIT launches whose slabs are reduced inside the kernel -- bf16x3 handles with ticket counters: that is the case measured; unsplit
        // launches and the exact-fp32 kernels, which would still need the separate epilogue launch, keep 256)
        const int min_wgs = min_env > 0 ? min_env : ((ncounters > 0 && sp > 1) ? 128 : 256);
        if (wgs * sp >= (split_target < min_wgs ? split_target : min_wgs)) {
            p.path = PATH_SPATIAL;
            p.nsplit = sp;
            p.ws_floats = sp > 1 ? (size_t)sp * p.out_elems : 0;
            if (sp > 1 && ncounters > 0 && wgs <= ncounters && (size_t)sp * p.out_elems * 4 < ((size_t)1 << 32)) {
                static const bool off = getenv("UAD_NO_INKERNEL_SPLITK") != nullptr;
                const int cst = CA / sp;
                const bool inst = f_type || (CA % sp == 0 && (cst == 32 || cst == 64 || (cst == 128 && p.sc.BN == 64)));
                p.inkernel = !off && inst;
            }
            p.tiles = (sp > 1 && !p.inkernel) ? (p.out_rows + 63) / 64 : d.N * (d.HS / p.sc.TH) * (d.WS / p.sc.TW);
            return p;
        }
    }
    if (ns > 1) {
        p.path = PATH_SPLITK; p.nsplit = ns; p.ws_floats = (size_t)ns * p.out_elems;
        p.tiles = (p.out_rows + 63) / 64;
        return p;
    }
    p.path = PATH_GENERIC;
    p.tiles = (int)((M + t.BM - 1) / t.BM) * classes;
    return p;
}
}  // namespace

bool uad_conv_k3_takes(const UadConvDesc& d, bool f_type) { return convk16_shape_ok(d, f_type); }
bool uad_conv_spatial_ok(const UadConvDesc& d, bool f_type) {
    if (convk16_shape_ok(d, f_type)) return true;      // k3 tap-list kernel (bf16x3 planes only: the fp32 pack of such a tensor is simply not used)
    return f_type ? choose_spatial(d, d.CB, d.CS, true).ok : choose_spatial(d, d.CS, d.CB, false).ok;
}
namespace {
// bf16x6 (three-plane) launches run on the F-kind and the lane = pixel spatial kernels; every other launch of a handle in that mode takes the exact-fp32
// route (its fp32 pack is kept beside the planes).  One decision for the launchers and the tile queries.
bool x6_route(const UadConvDesc& d, bool f_type, const GemmPlan& p) {
    if (p.path != PATH_SPATIAL) return false;
    if (f_type) return true;       // (final-backward-on-load forms: the 32-column instance only -- they have CA <= 32, which the planner gives that instance)
    if (d.CB % 32) return false;
    if (p.nsplit > 1 && !p.inkernel) return false;
    const int cst = (d.CS % p.nsplit == 0) ? d.CS / p.nsplit : 0;
    return p.sc.BN == 64 ? (cst == 32 || cst == 64 || cst == 128) : (cst == 32 || cst == 64);
}
// the fused final epilogue: which plans the kernels on bf16 planes (conv5_d16 / conv5_d16s: whole channel range of 32 or 64 in one 32-column workgroup) and the
// exact-fp32 instance conv5_d_kernel<8,16,32,4,1,true> take.  One predicate each for uad_conv_d_can_fuse_final*, run_plan and uad_conv_d_kernel_query.
inline bool final_plan_ok16(const GemmPlan& p, const UadConvDesc& d) { return p.path == PATH_SPATIAL && p.nsplit == 1 && p.sc.BN == 32 && d.CB == 32 && (d.CS == 32 || d.CS == 64); }
inline bool final_plan_ok32(const GemmPlan& p, int Nn) { return p.path == PATH_SPATIAL && p.nsplit == 1 && p.sc.BN != 64 && p.sc.CK == 32 && Nn == 32; }
// inst_ok: the launch's epilogue / activation-on-load form has a three-plane instance (D kind: d_x6_form_ok; every F form has one).  *x6: the route taken.
GemmPlan plan_for(const UadConvDesc& d, bool f_type, bool have_pack, size_t ws_floats, int ncounters, int planes16, bool inst_ok = true, bool* x6 = nullptr) {
    GemmPlan p = plan_gemm(d, f_type, have_pack, ws_floats, ncounters);
    const bool take = planes16 == 3 && inst_ok && x6_route(d, f_type, p);
    if (planes16 == 3 && !take) p = plan_gemm(d, f_type, have_pack, ws_floats, 0);      // the exact-fp32 kernels: no in-kernel slab reduction
    if (x6) *x6 = take;
    return p;
}
// the lane = pixel data-gradient kernel's three-plane instance list (conv5_d16s_takes), by epilogue kind and activation on load
inline bool d_x6_form_ok(const UadEpilogue& ep, bool has_xf) {
    return ep.kind == UAD_EPI_FINAL ? (ep.fin_dc == nullptr && ep.ealpha >= 0.f && ep.ealpha <= 1.f && has_xf) : ep.kind == UAD_EPI_BWD_ACT ? !has_xf : has_xf;
}
}  // namespace
bool uad_conv_d_x6_form_ok(const UadEpilogue& ep, bool has_xf) { return d_x6_form_ok(ep, has_xf); }
bool uad_conv_x6_takes(const UadConvDesc& d, bool f_type, size_t ws_floats, int ncounters) { return x6_route(d, f_type, plan_gemm(d, f_type, true, ws_floats, ncounters)); }
int uad_conv_f_tiles(const UadConvDesc& d, bool have_pack, size_t ws_floats, int ncounters, int planes16) { return plan_for(d, true, have_pack, ws_floats, ncounters, planes16).tiles; }
int uad_conv_d_tiles(const UadConvDesc& d, bool have_pack, size_t ws_floats, int ncounters, int planes16) { return plan_for(d, false, have_pack, ws_floats, ncounters, planes16).tiles; }
bool uad_conv_f_supports_final_bwd(const UadConvDesc& d, bool have_pack16, size_t ws_floats) {
    if (!have_pack16) return false;
    const GemmPlan p = plan_gemm(d, true, true, ws_floats);
    return p.path == PATH_SPATIAL;
}
bool uad_conv_d_can_fuse_final(const UadConvDesc& d, bool have_pack16, size_t ws_floats) {
    if (!have_pack16 || getenv("UAD_NO_FUSED_FINAL")) return false;
    const GemmPlan p = plan_gemm(d, false, true, ws_floats);
    // conv5_d16_kernel<8,16,CST,4,1> with the whole channel range in one workgroup column block
    return final_plan_ok16(p, d);
}
// exact-fp32 mode: conv5_d_kernel<8,16,32,4,1,FIN> (UAD_NO_FUSED_FINAL_F32=1: the separate final_kernel pass)
bool uad_conv_d_can_fuse_final_f32(const UadConvDesc& d, bool have_pack, size_t ws_floats) {
    if (!have_pack || getenv("UAD_NO_FUSED_FINAL") || getenv("UAD_NO_FUSED_FINAL_F32")) return false;
    const GemmPlan p = plan_gemm(d, false, true, ws_floats);
    return final_plan_ok32(p, d.CB);
}
size_t uad_conv_ws_floats(const UadConvDesc& d, bool f_type, bool have_pack) { return plan_gemm(d, f_type, have_pack, (size_t)1 << 40).ws_floats; }
// tests (uad_debug_plan): what uad_launch_conv_f / _d would run, from the launchers' own decision functions.  out[10]:
// 0 path (0 generic | 1 spatial | 2 split-K generic), 1 splits, 2 slabs reduced inside the kernel, 3 column-block instance (64 | 32), 4 column-partial tiles,
// 5 bf16x6 three-plane route (1 taken | 0 refused: exact-fp32 fall-back | -1 not a bf16x6 launch), 6 -1 (the fused final is the caller's decision), 7 0,
// 8 workspace floats the plan needs, 9 0 (capacity: the caller's)
void uad_conv_plan_query(const UadConvDesc& d, bool f_type, bool have_pack, size_t ws_floats, int ncounters, int planes16, bool inst_ok, long long* out) {
    bool x6 = false;
    const GemmPlan p = plan_for(d, f_type, have_pack, ws_floats, ncounters, planes16, inst_ok, &x6);      // exactly the launchers' call
    const int CA = f_type ? d.CB : d.CS, Nn = f_type ? d.CS : d.CB;
    out[0] = p.path; out[1] = p.nsplit; out[2] = p.inkernel ? 1 : 0;
    out[3] = p.path == PATH_SPATIAL ? p.sc.BN : choose_tile((long)d.N * d.HS * d.WS, Nn, CA, f_type ? 1 : d.S * d.S).BN;
    out[4] = p.tiles;
    out[5] = planes16 == 3 ? (x6 ? 1 : 0) : -1;
    out[6] = -1; out[7] = 0; out[8] = (long long)p.ws_floats; out[9] = 0;
}

namespace {
// the split fields of a spatial launch's arguments, as the kernel selection below reads them (a.Out still the caller's output on entry)
inline void spatial_split_args(const GemmPlan& p, ConvGemmArgs& a, float* ws) {
    float* out = a.Out;
    a.nsplit = 1;
    if (p.nsplit > 1) { a.Out = ws; a.nsplit = p.nsplit; a.out_final = out; }
    if (!(p.nsplit > 1 && p.inkernel && a.Wp16)) a.sk_counter = nullptr;
}
// D kind of a spatial launch on bf16 planes: the kernel generation that runs and the channel range `cst` a workgroup stages (0: CA does not divide by the splits).
// One decision for run_plan and uad_conv_d_kernel_query; `a` after spatial_split_args.
inline bool d16_instance(int bn, int cst) { return bn == 64 ? (cst == 128 || cst == 64 || cst == 32) : (cst == 64 || cst == 32); }
inline int d16_generation(const GemmPlan& p, const ConvGemmArgs& a, int* cst_out) {
    const int cst = (a.CA % p.nsplit == 0) ? a.CA / p.nsplit : 0;
    *cst_out = cst;
    if (!d16_instance(p.sc.BN, cst)) return UAD_DGEN_BF16_D;        // conv5_bf16_kernel: channel chunks streamed through LDS
    return uad_d16s_takes(a) ? UAD_DGEN_LANE_PIXEL : UAD_DGEN_CLASS_SEQ;      // uad_conv16s.inc | conv5_d16_kernel (its fallback)
}
void run_plan(const GemmPlan& p, ConvGemmArgs& a, bool f_type, float* ws, hipStream_t st) {
    const UadConvDesc& d = a.d;
    a.nsplit = 1; a.out_elems = p.out_elems;
    a.dbg = 0; a.dbgbuf = nullptr;
    if (p.path == PATH_SPATIAL) {
        float* out = a.Out;
        spatial_split_args(p, a, ws);
        dim3 grid((d.HS / p.sc.TH) * (d.WS / p.sc.TW), d.N, (a.Nn / p.sc.BN) * p.nsplit);
        if (a.Wp16) {   // bf16x3 / bf16x6 math mode
            if (f_type) uad_conv5_f16_launch(a, grid, p.sc.BN, take_request(g_any_order_next), st);
            else {
                // class-sequential kernel whenever the workgroup's whole channel range fits in LDS (CA == cst * nsplit)
                int cst = 0;
                const int gen = d16_generation(p, a, &cst);
                if (gen == UAD_DGEN_LANE_PIXEL) {      // lane = pixel generation (uad_conv16s.inc)
                    if (a.npl == 3) uad_d16s_launch_v3(a, grid, p.sc.BN, cst, take_request(g_any_order_next), st);
                    else uad_d16s_launch_v2(a, grid, p.sc.BN, cst, take_request(g_any_order_next), st);
                } else if (a.npl == 3) { fprintf(stderr, "uad: a bf16x6 launch reached a kernel without the three-plane form (x6_route decides before run_plan)\n"); abort(); }
                else if (gen == UAD_DGEN_CLASS_SEQ) uad_conv5_d16_launch(a, grid, p.sc.BN, cst, st);      // class-sequential generation (conv5_d16_kernel): the fallback of the lane = pixel one
                else uad_conv5_dbf16_launch(a, grid, p.sc.BN, p.sc.CK, st);
            }
        } else if (f_type) uad_conv5_f32_launch(a, grid, p.sc.BN, take_request(g_any_order_next), st);
        else {
            const bool fin = a.ep.kind == UAD_EPI_FINAL;
            if (fin && !final_plan_ok32(p, a.Nn)) { fprintf(stderr, "uad: fused final epilogue asked of an exact-fp32 launch that cannot run it (check uad_conv_d_can_fuse_final_f32 first)\n"); abort(); }
            uad_conv5_d32_launch(a, grid, p.sc.BN, p.sc.CK, fin, take_request(g_any_order_next), st);
        }
        if (p.nsplit > 1 && !a.sk_counter) uad_gemm_launch_splitk_epilogue(ws, p.nsplit, p.out_elems, p.out_rows, a.Nn, a.ep, out, st);
        return;
    }
    const int classes = f_type ? 1 : d.S * d.S;
    if (p.path == PATH_SPLITK) {
        float* out = a.Out;
        a.Out = ws; a.nsplit = p.nsplit;
        uad_gemm_launch(a, f_type, classes, st);
        uad_gemm_launch_splitk_epilogue(ws, p.nsplit, p.out_elems, p.out_rows, a.Nn, a.ep, out, st);
        return;
    }
    uad_gemm_launch(a, f_type, classes, st);
}
}  // namespace

void uad_launch_conv_f(const UadConvDesc& d, const float* big_in, UadXform xf, const float* W, float* small_out,
                       UadEpilogue ep, hipStream_t st, const float* Wpacked, UadGemmWs ws, const unsigned short* Wp16,
                       long long w16_plane, bool generic_bf16x3, int planes16) {
    if (convk16_takes(d, true, xf, ep, Wp16)) { run_convk16(d, true, big_in, small_out, ep, Wp16, w16_plane, planes16, st); return; }      // k3 s1 / s2, bf16x3 / bf16x6
    ConvGemmArgs a;
    a.Wp = Wpacked; a.Wp16 = Wp16; a.w16_plane = w16_plane; a.math16 = generic_bf16x3 ? 1 : 0; a.npl = 2;
    a.A = big_in; a.W = W; a.Out = small_out; a.xf = xf; a.ep = ep; a.d = d;
    a.M = d.N * d.HS * d.WS; a.CA = d.CB; a.Nn = d.CS;
    a.lws = ilog2_exact(d.WS); a.lhs = ilog2_exact(d.HS); a.dbgbuf = nullptr;
    a.sk_counter = nullptr; a.out_final = nullptr;
    bool x6 = false;
    const GemmPlan p = plan_for(d, true, Wpacked != nullptr || Wp16 != nullptr, ws.ptr ? ws.floats : 0, (Wp16 && ws.counters) ? ws.ncounters : 0, planes16, true, &x6);
    if (planes16 == 3) {
        if (x6) a.npl = 3;
        else {      // bf16x6 handle, launch outside the three-plane kernels: the exact-fp32 route (plan_for planned it: needs the fp32 pack wherever a spatial kernel could run)
            if (!Wpacked && d.KS == 5) { fprintf(stderr, "uad: a bf16x6 launch outside the three-plane spatial kernels needs the fp32 pack (uad_conv_x6_takes / uad_conv_k3_takes)\n"); abort(); }
            a.Wp16 = nullptr;
        }
    }
    if (p.inkernel) a.sk_counter = ws.counters;
    run_plan(p, a, true, ws.ptr, st);
}

namespace {
// What uad_launch_conv_d settles between filling the arguments and run_plan: the plan, the three-plane route (or the exact-fp32 one in its place) and the arrival
// counters.  *no_pack: a bf16x6 launch outside the three-plane kernels found no fp32 pack (the launcher aborts).  Shared with uad_conv_d_kernel_query.
GemmPlan settle_conv_d(ConvGemmArgs& a, const UadGemmWs& ws, int planes16, bool* x6, bool* no_pack) {
    const UadConvDesc& d = a.d;
    const GemmPlan p = plan_for(d, false, a.Wp != nullptr || a.Wp16 != nullptr, ws.ptr ? ws.floats : 0, (a.Wp16 && ws.counters) ? ws.ncounters : 0, planes16,
                                d_x6_form_ok(a.ep, a.xf.scale != nullptr), x6);
    *no_pack = false;
    if (planes16 == 3) {
        if (*x6) a.npl = 3;
        else {
            if (!a.Wp && d.KS == 5) *no_pack = true;
            a.Wp16 = nullptr;
        }
    }
    if (p.inkernel) a.sk_counter = ws.counters;
    return p;
}
}  // namespace

void uad_launch_conv_d(const UadConvDesc& d, const float* small_in, UadXform xf, const float* W, float* big_out,
                       UadEpilogue ep, hipStream_t st, const float* Wpacked, UadGemmWs ws, const unsigned short* Wp16,
                       long long w16_plane, bool generic_bf16x3, int planes16) {
    if (convk16_takes(d, false, xf, ep, Wp16)) { run_convk16(d, false, small_in, big_out, ep, Wp16, w16_plane, planes16, st); return; }
    ConvGemmArgs a;
    a.Wp = Wpacked; a.Wp16 = Wp16; a.w16_plane = w16_plane; a.math16 = generic_bf16x3 ? 1 : 0; a.npl = 2;
    a.A = small_in; a.W = W; a.Out = big_out; a.xf = xf; a.ep = ep; a.d = d;
    a.M = d.N * d.HS * d.WS; a.CA = d.CS; a.Nn = d.CB;
    a.lws = ilog2_exact(d.WS); a.lhs = ilog2_exact(d.HS); a.dbgbuf = nullptr;
    a.sk_counter = nullptr; a.out_final = nullptr;
    bool x6 = false, no_pack = false;
    const GemmPlan p = settle_conv_d(a, ws, planes16, &x6, &no_pack);
    if (no_pack) { fprintf(stderr, "uad: a bf16x6 launch outside the three-plane spatial kernels needs the fp32 pack (uad_conv_x6_takes / uad_conv_k3_takes)\n"); abort(); }
    run_plan(p, a, false, ws.ptr, st);
}

// tests (uad_op_conv_plan): the kernel a D-kind launch with these operands would run, answered by the launcher's own code (settle_conv_d, spatial_split_args,
// d16_generation); nothing is launched and no pointer is read.  out3: 0 generation (UAD_DGEN_*; 0: not a spatial launch), 1 channel range per workgroup `cst`
// (bf16 planes only), 2 the launch would abort() (bf16x6 without the fp32 pack it needs, or a fused final epilogue the kernel that runs does not have), 3 the fused
// final's tile height (16 | 8; 0: another epilogue)
void uad_conv_d_kernel_query(const UadConvDesc& d, bool has_xf, const UadEpilogue& ep, bool have_pack32, bool have_pack16, UadGemmWs ws, int planes16, long long* out3) {
    static float some;      // stands for every operand that is only tested for presence
    ConvGemmArgs a;
    a.Wp = have_pack32 ? &some : nullptr; a.Wp16 = have_pack16 ? reinterpret_cast<const unsigned short*>(&some) : nullptr; a.npl = 2;
    a.ep = ep; a.d = d; a.xf = UadXform(); a.xf.scale = has_xf ? &some : nullptr; a.Out = &some;
    a.M = d.N * d.HS * d.WS; a.CA = d.CS; a.Nn = d.CB;
    a.sk_counter = nullptr; a.out_final = nullptr;
    bool x6 = false, no_pack = false;
    const GemmPlan p = settle_conv_d(a, ws, planes16, &x6, &no_pack);
    out3[0] = 0; out3[1] = 0; out3[2] = no_pack ? 1 : 0; out3[3] = 0;
    if (p.path != PATH_SPATIAL) return;
    spatial_split_args(p, a, &some);
    if (a.Wp16) {
        int cst = 0;
        out3[0] = d16_generation(p, a, &cst); out3[1] = cst;
        out3[3] = ep.kind != UAD_EPI_FINAL ? 0 : (out3[0] == UAD_DGEN_LANE_PIXEL && uad_d16s_t16(a, p.sc.BN, cst, a.npl)) ? 16 : 8;
        if (out3[0] != UAD_DGEN_LANE_PIXEL && a.npl == 3) out3[2] = 1;
        if (ep.kind == UAD_EPI_FINAL && !final_plan_ok16(p, d)) out3[2] = 1;
    } else {
        out3[0] = UAD_DGEN_F32; out3[3] = ep.kind == UAD_EPI_FINAL ? 8 : 0;
        if (ep.kind == UAD_EPI_FINAL && !final_plan_ok32(p, a.Nn)) out3[2] = 1;
    }
}

// ---- W-type host side -------------------------------------------------------------------------
namespace {
struct WChoice { int BM, BN, splits, kper; };
inline WChoice choose_w(const UadConvDesc& d) {
    WChoice c;
    const int Mtot = d.KS * d.KS * d.CB;
    const long Kt = (long)d.N * d.HS * d.WS;
    c.BM = (Mtot >= 128) ? 128 : 64;
    c.BN = (d.CS > 32) ? 64 : 32;
    const long tiles = (long)((Mtot + c.BM - 1) / c.BM) * ((d.CS + c.BN - 1) / c.BN);
    const long ksteps = (Kt + 31) / 32;
    long splits = (1024 + tiles - 1) / tiles;          // aim for >= ~1024 workgroups
    long max_splits = (ksteps + 7) / 8;                // but keep >= 8 K-steps per split
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    long steps_per = (ksteps + splits - 1) / splits;
    c.kper = (int)steps_per * 32;
    c.splits = (int)((Kt + c.kper - 1) / c.kper);
    return c;
}
}  // namespace

namespace {
// bf16x6 instances: the three operand forms the model's backward uses -- (pattern word | plain gradient, activated input) in the decoder, (activated input,
// plain gradient) in the encoder; w_tr_x6_takes() tells the launcher, other forms of a bf16x6 launch run on the exact-fp32 generic kernels
inline bool w_tr_x6_takes(bool fbb, bool xa, bool xs) { return fbb ? xs : (xa != xs); }
// the k5 s2 filter gradient of a launch in a split-bf16 mode runs on the bf16 kernel unless it is a bf16x6 launch of an operand form without a three-plane instance
inline bool w5_use16(bool math_bf16x3, int planes16, bool fbb, bool xa, bool xs) { return math_bf16x3 && !(planes16 == 3 && !w_tr_x6_takes(fbb, xa, xs)); }
// 32-channel cs blocks per workgroup of that kernel: two (512 threads) where the layer has them; the exact-fp32 kernel takes one
inline int w5_ncsb(const UadConvDesc& d, bool use16) { return (use16 && d.CS % 64 == 0) ? 2 : 1; }
inline bool wk3_takes(const WK3Choice& k3, bool any16, int planes16, bool defer_reduce, bool any_xf) { return k3.ok && any16 && planes16 != 3 && !defer_reduce && !any_xf; }
}  // namespace

bool uad_conv_w_supports_fb_bits(const UadConvDesc& d, bool math_bf16x3) {
    return math_bf16x3 && choose_w5(d).ok && d.CB == 32;
}

size_t uad_conv_w_partial_floats(const UadConvDesc& d) {
    const W5Choice w5 = choose_w5(d, false), w5b = choose_w5(d, true);      // (the launch's math mode picks one of the two: size for the larger)
    if (w5.ok) return (size_t)(w5.splits > w5b.splits ? w5.splits : w5b.splits) * d.KS * d.KS * d.CB * d.CS;
    const WChoice c = choose_w(d);
    const WK3Choice k3 = choose_wk3(d);      // (which of the two runs depends on the math mode of the launch: size for both)
    const int splits = (k3.ok && k3.splits > c.splits) ? k3.splits : c.splits;
    return (size_t)splits * d.KS * d.KS * d.CB * d.CS;
}

void uad_launch_conv_w(const UadConvDesc& d, const float* big, UadXform xfb, const float* small, UadXform xfs,
                       float* dW, float* partial, hipStream_t st, bool math_bf16x3, hipStream_t reduce_st, hipEvent_t ev, bool generic_bf16x3, bool defer_reduce, int planes16) {
    // planes16 == 3 (with math_bf16x3): bf16x6 products in the k5 s2 kernel; a shape that kernel does not take runs on the exact-fp32 generic kernels
    // reduce_st/ev (optional): run the split-K slab reduction on a second stream, ordered after the main kernel by `ev`.
    // defer_reduce: leave the reduction to a later uad_launch_conv_w_reduce (the caller orders it after this kernel with ONE event per layer:
    // every event recorded on the main stream costs a ~6 us bubble before its next kernel)
    auto hop = [&]() -> hipStream_t {
        if (!reduce_st) return st;
        (void)hipEventRecord(ev, st);
        (void)hipStreamWaitEvent(reduce_st, ev, 0);
        return reduce_st;
    };
    const W5Choice w5 = choose_w5(d, math_bf16x3);
    // (a bf16x6 launch outside the three-plane instances: the exact-fp32 k5 kernel on the SAME split -- uad_launch_conv_w_reduce is told the launch's math mode, not the kernel)
    const bool use16 = w5_use16(math_bf16x3, planes16, xfb.fb_bits != nullptr, xfb.scale != nullptr && !xfb.fb_bits, xfs.scale != nullptr);
    if (w5.ok && math_bf16x3 && !use16 && xfb.fb_bits) { fprintf(stderr, "uad: bf16x6 filter gradient from the pattern word needs the small operand's activation on load\n"); abort(); }
    if (w5.ok) {
        ConvWArgs a;
        a.big = big; a.small_ = small; a.partial = (w5.splits == 1) ? dW : partial;
        a.xfb = xfb; a.xfs = xfs; a.d = d;
        a.Mtot = d.KS * d.KS * d.CB; a.Kt = d.N * d.HS * d.WS; a.kper = 0; a.lws = a.lhs = -1; a.dbgbuf = nullptr;
        { static const int abl = getenv("UAD_W_ABL") ? atoi(getenv("UAD_W_ABL")) : 0; a.abl = abl; }
        a.npl = (use16 && planes16 == 3) ? 3 : 2;
        dim3 grid(d.CB / 32, d.CS / 32, w5.splits);
        static const int dbgw = getenv("UAD_DBG") ? atoi(getenv("UAD_DBG")) : 0;
        static unsigned long long* wbuf = nullptr;
        static int wcalls = 0;
        const bool dbg_this = (dbgw & 32) && wcalls < 8;
        constexpr size_t kWbuf = (size_t)2 * 2048 * 8;
        if (dbg_this) { if (!wbuf) (void)hipMalloc((void**)&wbuf, kWbuf); (void)hipMemsetAsync(wbuf, 0, kWbuf, st); a.dbgbuf = wbuf; }
        struct Dump { bool on; hipStream_t st; unsigned long long* buf; dim3* g; int* calls; UadConvDesc d;
            ~Dump() { if (!on) return; (void)hipStreamSynchronize(st); const int nb = g->x * g->y * g->z; static unsigned long long h[2 * 2048];
                (void)hipMemcpy(h, buf, sizeof h, hipMemcpyDeviceToHost); ++*calls;
                unsigned long long t0 = ~0ull, t1 = 0, dmin = ~0ull, dmax = 0, dsum = 0, smax = 0;
                for (int b = 0; b < nb && b < 2048; ++b) { if (h[2 * b] < t0) t0 = h[2 * b]; if (h[2 * b + 1] > t1) t1 = h[2 * b + 1]; }
                for (int b = 0; b < nb && b < 2048; ++b) { const unsigned long long dd = h[2 * b + 1] - h[2 * b]; dsum += dd; if (dd < dmin) dmin = dd; if (dd > dmax) dmax = dd; if (h[2 * b] - t0 > smax) smax = h[2 * b] - t0; }
                fprintf(stderr, "[w5 CB=%d CS=%d HS=%d grid=%d,%d,%d] span=%llu (100MHz ticks) wg dur min=%llu avg=%llu max=%llu latest start=%llu\n", d.CB, d.CS, d.HS, g->x, g->y, g->z,
                        t1 - t0, dmin, dsum / nb, dmax, smax); } } dump{dbg_this, st, wbuf, &grid, &wcalls, d};
        if (use16) {
            const int ncsb = w5_ncsb(d, true);       // two 32-channel cs blocks per workgroup (512 threads) where the layer has them
            if (ncsb == 2) grid.y = d.CS / 64;
            uad_conv5_w16_launch(a, grid, ncsb, xfb.fb_bits != nullptr, xfb.scale != nullptr && !xfb.fb_bits, xfs.scale != nullptr, w5, take_request(g_any_order_w_next), st);
        } else uad_conv5_w32_launch(a, grid, w5, st);
        if (w5.splits > 1 && !defer_reduce) uad_launch_reduce_partials(partial, w5.splits, a.Mtot * d.CS, 1.0f, dW, hop());
        return;
    }
    const WK3Choice k3 = choose_wk3(d);
    if (wk3_takes(k3, math_bf16x3 || generic_bf16x3, planes16, defer_reduce, xfb.scale || xfs.scale || xfb.fb_bits)) {
        // k3 s1 / s2 filter gradient in bf16x3 (uad_convk16.inc): channel-major LDS tiles, slabs + fixed-order reduction
        ConvWArgs a;
        a.big = big; a.small_ = small; a.partial = (k3.splits == 1) ? dW : partial;
        a.xfb = xfb; a.xfs = xfs; a.d = d;
        a.Mtot = 9 * d.CB; a.Kt = d.N * d.HS * d.WS; a.kper = 0; a.lws = a.lhs = -1; a.dbgbuf = nullptr;
        uad_k3_launch_w(a, k3, d.S, k3.ncb, st);
        if (k3.splits > 1) uad_launch_reduce_partials(partial, k3.splits, a.Mtot * d.CS, 1.0f, dW, hop());
        return;
    }
    const WChoice c = choose_w(d);
    ConvWArgs a;
    a.big = big; a.small_ = small; a.partial = (c.splits == 1) ? dW : partial;
    a.xfb = xfb; a.xfs = xfs; a.d = d;
    a.Mtot = d.KS * d.KS * d.CB; a.Kt = d.N * d.HS * d.WS; a.kper = c.kper;
    a.lws = ilog2_exact(d.WS); a.lhs = ilog2_exact(d.HS); a.dbgbuf = nullptr;
    dim3 grid((a.Mtot + c.BM - 1) / c.BM, (d.CS + c.BN - 1) / c.BN, c.splits);
    static const bool w16_ok = !getenv("UAD_NO_W16");
    const bool w16 = generic_bf16x3 && w16_ok && !xfb.scale && !xfs.scale && c.BN == 64 && d.CB % 4 == 0 && d.CS % 4 == 0;
    uad_gemm_launch_w(a, grid, c.BM, c.BN, w16, st);
    if (c.splits > 1 && !defer_reduce) uad_launch_reduce_partials(partial, c.splits, a.Mtot * d.CS, 1.0f, dW, hop());
}

void uad_conv_any_order_next(bool on) { g_any_order_next = on; }
void uad_conv_w_any_order_next(bool on) { g_any_order_w_next = on; }
void uad_launch_conv_w_reduce(const UadConvDesc& d, float* dW, float* partial, hipStream_t st, bool math_bf16x3) {
    const W5Choice w5 = choose_w5(d, math_bf16x3);
    const int splits = w5.ok ? w5.splits : choose_w(d).splits;
    if (splits > 1) uad_launch_reduce_partials(partial, splits, d.KS * d.KS * d.CB * d.CS, 1.0f, dW, st);
}
void uad_launch_conv_w_finish(const UadConvDesc& d, float* dW, float* partial, bool math_bf16x3, UadGradFinish a, hipStream_t st) {
    const W5Choice w5 = choose_w5(d, math_bf16x3);
    const int splits = w5.ok ? w5.splits : choose_w(d).splits;
    a.partial = splits > 1 ? partial : nullptr; a.S = splits > 1 ? splits : 0; a.L = d.KS * d.KS * d.CB * d.CS; a.dW = dW;
    uad_launch_grad_finish(a, st);
}

// tests (uad_debug_plan): what uad_launch_conv_w would run.  out[10]: 0 kernel (0 generic | 1 k5 s2 tile kernel, choose_w5 | 2 k3 tap-list kernel), 1 splits,
// 2 the last split is short, 3 32-channel cs blocks per workgroup (k5: 1 | 2; else 0), 4 work units (k5 / k3: 8 x 8 output tiles; generic: 32-position K steps),
// 5 bf16x6 three-plane kernel (1 | 0 exact-fp32 kernel | -1 not a bf16x6 launch), 6 -1, 7 units per split, 8 slab floats the launch writes, 9 0 (capacity: the caller's)
void uad_conv_w_plan_query(const UadConvDesc& d, bool math_bf16x3, int planes16, bool fbb, bool xa, bool xs, bool generic_bf16x3, bool defer_reduce, long long* out) {
    const long long slab = (long long)d.KS * d.KS * d.CB * d.CS;
    out[5] = -1; out[6] = -1; out[9] = 0;
    const W5Choice w5 = choose_w5(d, math_bf16x3);
    if (w5.ok) {
        const bool use16 = w5_use16(math_bf16x3, planes16, fbb, xa, xs);
        out[0] = 1; out[1] = w5.splits; out[2] = (w5.total_tiles % w5.tiles_per_split) ? 1 : 0; out[3] = w5_ncsb(d, use16); out[4] = w5.total_tiles;
        if (math_bf16x3 && planes16 == 3) out[5] = use16 ? 1 : 0;
        out[7] = w5.tiles_per_split; out[8] = w5.splits > 1 ? w5.splits * slab : 0;
        return;
    }
    const WK3Choice k3 = choose_wk3(d);
    if (wk3_takes(k3, math_bf16x3 || generic_bf16x3, planes16, defer_reduce, fbb || xa || xs)) {
        out[0] = 2; out[1] = k3.splits; out[2] = (k3.total_tiles % k3.tiles_per_split) ? 1 : 0; out[3] = 0; out[4] = k3.total_tiles;
        out[7] = k3.tiles_per_split; out[8] = k3.splits > 1 ? k3.splits * slab : 0;
        return;
    }
    const WChoice c = choose_w(d);
    const long long Kt = (long long)d.N * d.HS * d.WS;
    out[0] = 0; out[1] = c.splits; out[2] = (Kt % c.kper) ? 1 : 0; out[3] = 0; out[4] = (Kt + 31) / 32; out[7] = c.kper / 32; out[8] = c.splits > 1 ? c.splits * slab : 0;
}

