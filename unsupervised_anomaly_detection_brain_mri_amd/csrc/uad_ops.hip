// The part of the C-ABI (include/uad_hip.h) that takes no model handle: the library's error message and version, the stand-alone device ops
// (residual, counter-based random fill, clock probe, slice / mask gathers), the op-level entry points uad_op_* that run ONE launch of the
// kernels of the conv layer (uad_conv_plan.hip and its kernel units) / of the step's small-kernel units (uad_reduce.hip, uad_conv_first.hip, uad_loss.hip, uad_optim.hip) on caller-supplied tensors (weight packs and workspace built on the fly, synchronous: tests and
// tools), and the k3 kernel's in-kernel profile switch.  Host-only: no kernel is defined here.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "uad_handle.h"      // fail, no_xform, epi_bias (the launch-argument helpers the handles use too); no handle is touched here

static thread_local std::string g_err;

// records the message uad_last_error() returns; declared in uad_kernels.h for every launch layer
int uad_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" {

const char* uad_last_error(void) { return g_err.c_str(); }
const char* uad_version(void) { return "uad_hip 0.1 (gfx950, fp32 MFMA)"; }

int uad_k3_profile_enable(int on) { uad_k3_prof_enable(on != 0); return UAD_OK; }
int uad_k3_profile_read(char* buf, int cap) { return uad_k3_prof_read(buf, cap); }

int uad_residual(const float* x, const float* xr, const float* mask, int n, int hw, int pos_only, float prior_thresh,
                 float* out, float* l1err, void* stream) {
    if (!x || !xr || !out || n <= 0 || hw <= 0) return fail(UAD_ERR_INVALID, "uad_residual: bad arguments");
    uad_launch_residual(x, xr, mask, n, hw, pos_only, prior_thresh, out, l1err, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_rng_fill(const uad_rng_job_t* jobs, int njobs, int n, unsigned long long seed, unsigned long long step, long long sample0, void* stream) {
    if (!jobs || njobs <= 0 || njobs > 8 || n <= 0 || sample0 < 0) return fail(UAD_ERR_INVALID, "rng_fill: 1..8 jobs, n > 0, sample0 >= 0");
    UadRngJob js[8];
    for (int i = 0; i < njobs; ++i) {
        if (!jobs[i].out || jobs[i].per_sample <= 0 || (jobs[i].kind != UAD_RNG_NORMAL && jobs[i].kind != UAD_RNG_KEEP_MASK))
            return fail(UAD_ERR_INVALID, "rng_fill: job %d: null output, empty sample or unknown kind", i);
        if (jobs[i].kind == UAD_RNG_KEEP_MASK && !(jobs[i].rate >= 0.f && jobs[i].rate < 1.f)) return fail(UAD_ERR_INVALID, "rng_fill: dropout rate must be in [0, 1)");
        js[i] = UadRngJob{jobs[i].out, jobs[i].per_sample, jobs[i].kind, jobs[i].rate, jobs[i].stream};
    }
    uad_launch_rng_fill(js, njobs, n, seed, step, sample0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_clock_probe(unsigned long long* out2, unsigned long long ticks_100mhz, void* stream) {
    if (!out2 || ticks_100mhz == 0 || ticks_100mhz > 1000000000ull) return fail(UAD_ERR_INVALID, "clock_probe: null output or a duration outside (0, 10 s]");
    uad_launch_clock_probe(out2, ticks_100mhz, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_gather_slices(const float* src, const int* idx, int n, long long slice_elems, float* out, void* stream) {
    if (!src || !idx || !out || n <= 0 || slice_elems <= 0 || slice_elems % 4) return fail(UAD_ERR_INVALID, "gather_slices: bad arguments (slice elements must be a multiple of 4)");
    if (n > 65535) return fail(UAD_ERR_UNSUPPORTED, "gather_slices: at most 65535 slices per call");
    uad_launch_gather_slices(src, idx, n, slice_elems, out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
int uad_gather_mask(const unsigned char* labels, const int* idx, int n, long long slice_px, const unsigned char* lut256, float* out, void* stream) {
    if (!labels || !idx || !out || n <= 0 || slice_px <= 0) return fail(UAD_ERR_INVALID, "gather_mask: bad arguments");
    if (n > 65535) return fail(UAD_ERR_UNSUPPORTED, "gather_mask: at most 65535 slices per call");
    uad_launch_gather_mask(labels, idx, n, slice_px, lut256, out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

// ------------------------------------------------------------------------------------------------ op-level entry points
static UadConvDesc to_desc(const uad_conv_desc_t* d) { return UadConvDesc{d->N, d->HB, d->WB, d->CB, d->HS, d->WS, d->CS, d->KS, d->S, d->P}; }
static UadXform to_xf(const uad_xform_t* x) {
    UadXform r; r.scale = x ? x->scale : nullptr; r.shift = x ? x->shift : nullptr; r.alpha = x ? x->alpha : 1.f; r.mult = 1.f;
    return r;
}
static int check_gemm_desc(const uad_conv_desc_t* d, bool f_type) {
    if (!d) return fail(UAD_ERR_INVALID, "null desc");
    const int ca = f_type ? d->CB : d->CS, nn = f_type ? d->CS : d->CB;
    if (ca % 8 || nn % 4) return fail(UAD_ERR_UNSUPPORTED, "contraction channels must be a multiple of 8 and output channels of 4");
    return UAD_OK;
}

// op-level helpers: the spatial kernels need the packed weight copy; build it on the fly (synchronous, tests only)
// UAD_MATH of the op-level entry points: unset / "f32" = exact fp32, "bf16x3", or "bf16x6" = three-plane products on the k3 tap-list kernel and on the k5 s2
// spatial kernels where they take the launch (the exact-fp32 route for a k5 launch they refuse, everything else as bf16x3)
static bool op_bf16x6() { const char* e = getenv("UAD_MATH"); return e && !strcmp(e, "bf16x6"); }
static bool op_bf16x3() { const char* e = getenv("UAD_MATH"); return e && (!strcmp(e, "bf16x3") || !strcmp(e, "bf16x6")); }
static int op_math() { return op_bf16x6() ? UAD_MATH_BF16X6 : op_bf16x3() ? UAD_MATH_BF16X3 : UAD_MATH_F32; }
static bool op_k5(const UadConvDesc& d, bool f_type) { return d.KS == 5 && uad_conv_spatial_ok(d, f_type); }
// plain: identity activation on load, bias (+ addend) epilogue without `mul` -- what the k3 tap-list kernel takes besides the shape (uad_convk16.inc:
// convk16_takes); any other launch of a k3 shape runs the generic kernels, which understand TWO planes only.  A k5 s2 launch of the spatial kernels is handed
// three planes AND the fp32 pack: the launcher's own decision (plan_for / x6_route / d_x6_form_ok) picks the route, and no route is left without its operand.
static int op_planes(const UadConvDesc& d, bool f_type, bool plain) {
    if (!op_bf16x6()) return 2;
    return ((plain && uad_conv_k3_takes(d, f_type)) || op_k5(d, f_type)) ? 3 : 2;
}
// the workspace a launch is given: slabs + (behind them) the arrival counters of the in-kernel reduction -- the same path as the model handle.  Shape only (plan
// query), or allocated and zeroed (launch).
static const int kOpCounters = 16384;
static UadGemmWs op_ws_shape(const UadConvDesc& d, bool f_type, bool have_pack) {
    static float some;      // a plan query only tests the pointers for presence
    UadGemmWs ws;
    ws.ptr = nullptr; ws.floats = uad_conv_ws_floats(d, f_type, have_pack); ws.counters = nullptr; ws.ncounters = 0;
    if (ws.floats) { ws.ptr = &some; ws.counters = reinterpret_cast<unsigned*>(&some); ws.ncounters = kOpCounters; }
    return ws;
}
static int ws_for_op(const UadConvDesc& d, bool f_type, bool have_pack, UadGemmWs* ws) {
    *ws = op_ws_shape(d, f_type, have_pack);
    ws->ptr = nullptr; ws->counters = nullptr;
    if (ws->floats) {
        HIP_TRY(hipMalloc((void**)&ws->ptr, (ws->floats + kOpCounters) * sizeof(float)));
        HIP_TRY(hipMemset(ws->ptr + ws->floats, 0, kOpCounters * sizeof(float)));
        ws->counters = reinterpret_cast<unsigned*>(ws->ptr + ws->floats);
    }
    return UAD_OK;
}
// the packs of one tensor in the selected math mode: p32 (fp32 pack) and / or p16 (two or three bf16 planes), F and D layout each
struct OpPacks {
    float *f32 = nullptr, *d32 = nullptr, *f16 = nullptr, *d16 = nullptr;
    int planes = 2;
    void release() { (void)hipFree(f32); (void)hipFree(d32); (void)hipFree(f16); (void)hipFree(d16); f32 = d32 = f16 = d16 = nullptr; }
    bool any() const { return f32 || f16; }
};
static bool op_has32(const UadConvDesc& d, bool f_type, int planes) { return uad_conv_spatial_ok(d, f_type) && (!op_bf16x3() || (planes == 3 && op_k5(d, f_type))); }
static bool op_has16(const UadConvDesc& d, bool f_type) { return uad_conv_spatial_ok(d, f_type) && op_bf16x3(); }
static int pack_for_op(const UadConvDesc& d, const float* W, bool f_type, OpPacks* pk, hipStream_t st, bool plain = false) {
    *pk = OpPacks();
    pk->planes = op_planes(d, f_type, plain);
    const size_t n = (size_t)d.KS * d.KS * d.CB * d.CS;
    long long off = 0; int cb = d.CB, cs = d.CS, taps = d.KS * d.KS;
    if (op_has32(d, f_type, pk->planes)) {
        HIP_TRY(hipMalloc((void**)&pk->f32, n * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&pk->d32, n * sizeof(float)));
        uad_launch_pack_weights(W, pk->f32, pk->d32, &off, &cb, &cs, &taps, 1, st);
    }
    if (op_has16(d, f_type)) {
        HIP_TRY(hipMalloc((void**)&pk->f16, 2 * n * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&pk->d16, 2 * n * sizeof(float)));
        if (pk->planes == 3) uad_launch_pack_weights_bf16_3p(W, (unsigned short*)pk->f16, (unsigned short*)pk->d16, &off, &cb, &cs, &taps, 1, st);
        else uad_launch_pack_weights_bf16(W, (unsigned short*)pk->f16, (unsigned short*)pk->d16, &off, &cb, &cs, &taps, 1, st);
    }
    return UAD_OK;
}
// launch arguments for the op-level entry points in the selected math mode
#define OP_PACK_ARGS(pk, d, f) ((f) ? (pk).f32 : (pk).d32), ws, (const unsigned short*)((f) ? (pk).f16 : (pk).d16), \
                               (long long)(d).KS * (d).KS * (d).CB * (d).CS, op_bf16x3(), (pk).planes
static int finish_op(OpPacks& pk, hipStream_t st, float* wsp = nullptr) {
    if (pk.any() || wsp) { HIP_TRY(hipStreamSynchronize(st)); pk.release(); (void)hipFree(wsp); }
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

// What an F / D entry point would launch, from the launchers' own decision functions; out[12] as include/uad_hip.h describes uad_op_conv_plan.
// plain: see op_planes.  fb: F kind, final backward on load.
static void op_plan_fd(const UadConvDesc& d, bool f_type, const UadEpilogue& ep, bool has_xf, bool plain, bool fb, long long* out) {
    const int planes = op_planes(d, f_type, plain);
    const bool has32 = op_has32(d, f_type, planes), has16 = op_has16(d, f_type);
    const UadGemmWs ws = op_ws_shape(d, f_type, has32 || has16);
    for (int i = 0; i < 12; ++i) out[i] = 0;
    uad_conv_plan_query(d, f_type, has32 || has16, ws.ptr ? ws.floats : 0, (has16 && ws.counters) ? ws.ncounters : 0, planes,
                        f_type || uad_conv_d_x6_form_ok(ep, has_xf), out);
    out[6] = 0; out[7] = 0; out[9] = 0; out[10] = op_math(); out[11] = 0;
    const bool on16 = has16 && out[5] != 0;      // the launch runs on bf16 planes (a refused three-plane route runs on the fp32 pack)
    if (f_type) {
        // final backward on load: the F-kind spatial kernels on bf16 planes, one bit per channel of a 32-bit word, and no three-plane 64-column instance
        if (fb && !(on16 && out[0] == 1 && d.CB <= 32 && has_xf && !(out[5] == 1 && out[3] == 64))) out[9] = 1;
        return;
    }
    long long k[4];
    uad_conv_d_kernel_query(d, has_xf, ep, has32, has16, ws, planes, k);
    out[6] = k[0]; out[7] = k[1]; out[11] = k[3];
    if (k[2]) out[9] = 1;
    if (ep.kind == UAD_EPI_FINAL) {
        const bool ok = on16 ? uad_conv_d_can_fuse_final(d, true, ws.floats) : uad_conv_d_can_fuse_final_f32(d, has32, ws.floats);
        if (!ok || d.KS != 5) out[9] = 1;
        if (ep.fin_bits && !on16) out[9] = 1;      // the exact-fp32 kernel writes the uncompressed gradient only
    }
}

int uad_op_conv_plan(const uad_conv_desc_t* dd, int kind, int epi, int xf_flags, long long* out) {
    if (!dd || !out) return fail(UAD_ERR_INVALID, "null argument");
    const UadConvDesc d = to_desc(dd);
    static float some;      // presence of an operand is all a plan reads
    if (kind == 'F' || kind == 'D') {
        UadEpilogue e;
        memset(&e, 0, sizeof e);
        const bool has_xf = (xf_flags & UAD_OP_XF_IN) != 0, fb = kind == 'F' && (xf_flags & UAD_OP_XF_FINAL_BWD);
        if (epi == UAD_OP_EPI_BIAS) e.kind = UAD_EPI_BIAS;
        else if (epi == UAD_OP_EPI_BWD_ACT) e.kind = UAD_EPI_BWD_ACT;
        else if (kind == 'D' && (epi == UAD_OP_EPI_FINAL || epi == UAD_OP_EPI_FINAL_TRAIN || epi == UAD_OP_EPI_FINAL_DC)) {
            e.kind = UAD_EPI_FINAL; e.ealpha = 0.3f;
            if (epi == UAD_OP_EPI_FINAL_TRAIN) { e.fin_bits = reinterpret_cast<unsigned*>(&some); e.fin_dxhat = &some; }
            if (epi == UAD_OP_EPI_FINAL_DC) e.fin_dc = &some;
        } else return fail(UAD_ERR_INVALID, "unknown epilogue %d for kind %c", epi, kind);
        op_plan_fd(d, kind == 'F', e, has_xf || fb, epi == UAD_OP_EPI_BIAS && !has_xf && !fb, fb, out);      // (plain: a bias launch without activation on load; `mul` is not part of the query)
        return UAD_OK;
    }
    if (kind == 'W') {
        for (int i = 0; i < 12; ++i) out[i] = 0;
        const int planes = (op_bf16x6() && d.KS == 5) ? 3 : 2;
        uad_conv_w_plan_query(d, op_bf16x3(), planes, false, (xf_flags & UAD_OP_XF_IN) != 0, (xf_flags & UAD_OP_XF_SMALL) != 0, op_bf16x3(), false, out);
        out[6] = 0; out[9] = 0; out[10] = op_math(); out[11] = 0;
        return UAD_OK;
    }
    return fail(UAD_ERR_INVALID, "kind must be 'F', 'D' or 'W'");
}

static int op_conv_f(const uad_conv_desc_t* d, const float* big_in, UadXform xf, const float* W, const float* bias,
                     const float* mul, const float* add, float* small_out, void* stream) {
    if (int rc = check_gemm_desc(d, true)) return rc;
    const bool plain = !xf.scale && !mul, fb = xf.fb_bits != nullptr;
    long long q[12];
    op_plan_fd(to_desc(d), true, epi_bias(bias, mul, add), xf.scale != nullptr, plain, fb, q);
    if (q[9]) return fail(UAD_ERR_UNSUPPORTED, "final backward on load: no F-kind spatial instance takes this launch (uad_op_conv_plan)");
    OpPacks pk;
    if (int rc = pack_for_op(to_desc(d), W, true, &pk, (hipStream_t)stream, plain)) { pk.release(); return rc; }
    UadGemmWs ws;
    if (int rc = ws_for_op(to_desc(d), true, pk.any(), &ws)) { pk.release(); (void)hipFree(ws.ptr); return rc; }
    uad_launch_conv_f(to_desc(d), big_in, xf, W, small_out, epi_bias(bias, mul, add), (hipStream_t)stream, OP_PACK_ARGS(pk, *d, true));
    return finish_op(pk, (hipStream_t)stream, ws.ptr);
}
int uad_op_conv_f(const uad_conv_desc_t* d, const float* big_in, const uad_xform_t* xf, const float* W, const float* bias,
                  const float* mul, const float* add, float* small_out, void* stream) {
    return op_conv_f(d, big_in, to_xf(xf), W, bias, mul, add, small_out, stream);
}
int uad_op_conv_f_final_bwd(const uad_conv_desc_t* d, const unsigned* bits, const float* dxhat, const float* wf, const uad_xform_t* bn, const float* W,
                            const float* bias, const float* mul, const float* add, float* small_out, void* stream) {
    if (!bits || !dxhat || !wf || !bn || !bn->scale) return fail(UAD_ERR_INVALID, "final backward on load needs the pattern words, d / d x_hat, the final kernel and the block's scale / shift");
    UadXform xf = to_xf(bn);
    xf.fb_bits = bits; xf.fb_dxhat = dxhat; xf.fb_wf = wf;
    return op_conv_f(d, nullptr, xf, W, bias, mul, add, small_out, stream);
}
int uad_op_conv_d(const uad_conv_desc_t* d, const float* small_in, const uad_xform_t* xf, const float* W, const float* bias,
                  const float* mul, const float* add, float* big_out, void* stream) {
    if (int rc = check_gemm_desc(d, false)) return rc;
    OpPacks pk;
    const bool plain = !(xf && xf->scale) && !mul;
    long long q[12];
    op_plan_fd(to_desc(d), false, epi_bias(bias, mul, add), xf && xf->scale, plain, false, q);
    if (q[9]) return fail(UAD_ERR_UNSUPPORTED, "conv_d: the kernel this launch would run has no form for it (uad_op_conv_plan)");
    if (int rc = pack_for_op(to_desc(d), W, false, &pk, (hipStream_t)stream, plain)) { pk.release(); return rc; }
    UadGemmWs ws;
    if (int rc = ws_for_op(to_desc(d), false, pk.any(), &ws)) { pk.release(); (void)hipFree(ws.ptr); return rc; }
    uad_launch_conv_d(to_desc(d), small_in, to_xf(xf), W, big_out, epi_bias(bias, mul, add), (hipStream_t)stream, OP_PACK_ARGS(pk, *d, false));
    return finish_op(pk, (hipStream_t)stream, ws.ptr);
}

int uad_op_conv_d_final(const uad_conv_desc_t* dd, const float* small_in, const uad_xform_t* xf, const float* W, const float* bias, const uad_xform_t* bn,
                        const float* wf, const float* bf, const float* x, float inv_batch, float* x_hat, float* l1, float* rec_sum,
                        unsigned* bits, float* dxhat, float* dc, float* red, void* stream) {
    if (int rc = check_gemm_desc(dd, false)) return rc;
    if (!small_in || !W || !bn || !bn->scale || !bn->shift || !wf || !bf || !x || !x_hat || !rec_sum) return fail(UAD_ERR_INVALID, "conv_d_final: null argument");
    if ((bits != nullptr) != (dxhat != nullptr) || (bits && dc) || ((bits || dc) && !red)) return fail(UAD_ERR_INVALID, "conv_d_final: forms are forward only, (bits, dxhat, red) or (dc, red)");
    const UadConvDesc d = to_desc(dd);
    hipStream_t st = (hipStream_t)stream;
    UadEpilogue e;
    memset(&e, 0, sizeof e);
    e.kind = UAD_EPI_FINAL; e.bias = bias;
    e.escale = bn->scale; e.eshift = bn->shift; e.ealpha = bn->alpha; e.emult = 1.f;
    e.fin_wf = wf; e.fin_bf = bf; e.fin_x = x; e.fin_xhat = x_hat; e.fin_l1 = l1;
    e.fin_dc = dc; e.fin_bits = bits; e.fin_dxhat = dxhat; e.fin_inv_batch = inv_batch;
    long long q[12];
    op_plan_fd(d, false, e, xf && xf->scale, false, false, q);
    if (q[9]) return fail(UAD_ERR_UNSUPPORTED, "conv_d_final: no kernel with the fused final epilogue takes this launch (uad_op_conv_plan)");
    // partial sums: one slot per 8 x 16 tile of the small map (the layout every instance writes and uad_final_blocks_per_sample counts)
    const int T = d.N * (d.HS / 8) * (d.WS / 16), L = 3 * d.CB + 1;
    float *recp = nullptr, *redp = nullptr;
    HIP_TRY(hipMalloc((void**)&recp, (size_t)T * sizeof(float)));
    if (hipMalloc((void**)&redp, (size_t)T * L * sizeof(float)) != hipSuccess) { (void)hipFree(recp); return fail(UAD_ERR_HIP, "conv_d_final: out of device memory"); }
    e.fin_rec_partial = recp; e.fin_red_partial = redp;
    OpPacks pk;
    if (int rc = pack_for_op(d, W, false, &pk, st)) { pk.release(); (void)hipFree(recp); (void)hipFree(redp); return rc; }
    UadGemmWs ws;
    if (int rc = ws_for_op(d, false, pk.any(), &ws)) { pk.release(); (void)hipFree(ws.ptr); (void)hipFree(recp); (void)hipFree(redp); return rc; }
    uad_launch_conv_d(d, small_in, to_xf(xf), W, nullptr, e, st, OP_PACK_ARGS(pk, *dd, false));
    uad_launch_reduce_partials(recp, T, 1, 1.0f, rec_sum, st);
    if (red) uad_launch_reduce_partials(redp, T, L, 1.0f, red, st);
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(recp); (void)hipFree(redp);
    return finish_op(pk, st, ws.ptr);
}

static int bwdact_common(bool f_type, const uad_conv_desc_t* dd, const float* in, const float* W, const float* cprev,
                         const uad_xform_t* act, float* out, float* s1, float* s2, void* stream) {
    if (int rc = check_gemm_desc(dd, f_type)) return rc;
    if (!act || !act->scale) return fail(UAD_ERR_INVALID, "bwdact needs the activation scale/shift");
    UadConvDesc d = to_desc(dd);
    const int C = f_type ? d.CS : d.CB;
    UadEpilogue e;
    memset(&e, 0, sizeof e);
    e.kind = UAD_EPI_BWD_ACT; e.cprev = cprev; e.escale = act->scale; e.eshift = act->shift; e.ealpha = act->alpha;
    e.emult = 1.f;
    long long q[12];
    op_plan_fd(d, f_type, e, false, false, false, q);
    if (q[9]) return fail(UAD_ERR_UNSUPPORTED, "bwdact: the kernel this launch would run has no form for it (uad_op_conv_plan)");
    const int T = (int)q[4];      // column-partial tiles of the plan the launcher will make
    hipStream_t st = (hipStream_t)stream;
    OpPacks pk;
    if (int rc = pack_for_op(d, W, f_type, &pk, st)) { pk.release(); return rc; }
    UadGemmWs ws;
    if (int rc = ws_for_op(d, f_type, pk.any(), &ws)) { pk.release(); (void)hipFree(ws.ptr); return rc; }
    float* colpart = nullptr;
    if (hipMalloc((void**)&colpart, (size_t)T * 2 * C * sizeof(float)) != hipSuccess) { pk.release(); (void)hipFree(ws.ptr); return fail(UAD_ERR_HIP, "bwdact: out of device memory"); }
    e.colpart = colpart;
    if (f_type) uad_launch_conv_f(d, in, no_xform(), W, out, e, st, OP_PACK_ARGS(pk, *dd, true));
    else uad_launch_conv_d(d, in, no_xform(), W, out, e, st, OP_PACK_ARGS(pk, *dd, false));
    // rstd = 1, gamma unused for dbias=null: dbeta -> s1, dgamma -> s2
    uad_launch_bn_grad_finalize(colpart, T, C, act->scale, 1.0f, s2, s1, nullptr, st);
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(colpart);
    return finish_op(pk, st, ws.ptr);
}
int uad_op_conv_f_bwdact(const uad_conv_desc_t* d, const float* big_in, const float* W, const float* cprev,
                         const uad_xform_t* act, float* small_out, float* s1, float* s2, void* stream) {
    return bwdact_common(true, d, big_in, W, cprev, act, small_out, s1, s2, stream);
}
int uad_op_conv_d_bwdact(const uad_conv_desc_t* d, const float* small_in, const float* W, const float* cprev,
                         const uad_xform_t* act, float* big_out, float* s1, float* s2, void* stream) {
    return bwdact_common(false, d, small_in, W, cprev, act, big_out, s1, s2, stream);
}

int uad_op_conv_w(const uad_conv_desc_t* dd, const float* big, const uad_xform_t* xfb, const float* small_,
                  const uad_xform_t* xfs, float* dW, void* stream) {
    if (!dd) return fail(UAD_ERR_INVALID, "null desc");
    if (dd->CB % 4 || dd->CS % 4) return fail(UAD_ERR_UNSUPPORTED, "channels must be multiples of 4");
    UadConvDesc d = to_desc(dd);
    float* partial = nullptr;
    HIP_TRY(hipMalloc((void**)&partial, uad_conv_w_partial_floats(d) * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    // bf16x6: the k5 s2 kernel's three-plane instances where w_tr_x6_takes the operand forms, the exact-fp32 k5 kernel where it does not (uad_launch_conv_w decides;
    // the filter gradient reads no weight pack)
    const int planes = (op_bf16x6() && d.KS == 5) ? 3 : 2;
    uad_launch_conv_w(d, big, to_xf(xfb), small_, to_xf(xfs), dW, partial, st, op_bf16x3(), nullptr, nullptr, op_bf16x3(), false, planes);
    HIP_TRY(hipStreamSynchronize(st));
    hipFree(partial);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_op_conv_first_fwd(const uad_conv_desc_t* d, const float* x, const float* W, const float* bias, float* out, void* stream) {
    if (!d || d->CS % 8 || 256 % (d->CS / 8)) return fail(UAD_ERR_UNSUPPORTED, "first conv: Cout must be a multiple of 8 dividing 2048");
    uad_launch_conv_first_fwd(to_desc(d), x, W, bias, out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
int uad_op_conv_first_wgrad(const uad_conv_desc_t* dd, const float* x, const float* g, float* dW, void* stream) {
    if (!dd || !((dd->KS == 5 && (dd->CB == 1 || dd->CB == 3)) || (dd->KS == 3 && dd->CB == 1)) || 256 % dd->CS)
        return fail(UAD_ERR_UNSUPPORTED, "first wgrad: (KS=5, Cin in {1,3}) or (KS=3, Cin=1), Cout | 256");
    UadConvDesc d = to_desc(dd);
    float* partial = nullptr;
    HIP_TRY(hipMalloc((void**)&partial, uad_conv_first_wgrad_partial_floats(d) * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    uad_launch_conv_first_wgrad(d, x, g, dW, partial, st);
    HIP_TRY(hipStreamSynchronize(st));
    hipFree(partial);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
int uad_op_adam(float* p, const float* g, float* mm, float* v, long long n, float lr_t, float beta1, float beta2, float eps,
                float gscale, void* stream) {
    uad_launch_adam(p, g, mm, v, (size_t)n, lr_t, beta1, beta2, eps, gscale, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

long long uad_op_grad_finish_scratch_floats(void) { return (long long)uad_grad_finish_scratch_floats(); }
int uad_op_grad_finish(const uad_grad_finish_t* a, int fused, float* scratch, void* stream) {
    if (!a || !scratch) return fail(UAD_ERR_INVALID, "grad_finish: null argument");
    if ((a->slabs && (a->S < 1 || a->L < 1 || !a->dW)) || (a->colpart && (a->T < 1 || a->C < 1 || !a->gamma)) ||
        (a->fin_partial && (a->fin_T < 1 || a->fin_C < 1 || !a->fin_gamma || !a->dwf || !a->dbf || !a->fin_red)))
        return fail(UAD_ERR_INVALID, "grad_finish: a part with an input needs its sizes and outputs");
    hipStream_t st = (hipStream_t)stream;
    if (fused) {
        if (!uad_grad_finish_takes(a->colpart ? a->C : 0, a->fin_partial ? a->fin_C : 0)) return fail(UAD_ERR_UNSUPPORTED, "grad_finish: C <= 512 and fin_C <= 64 in one launch");
        UadGradFinish f;
        memset(&f, 0, sizeof f);
        f.partial = a->slabs; f.S = a->S; f.L = a->L; f.dW = a->dW;
        f.colpart = a->colpart; f.T = a->T; f.C = a->C; f.gamma = a->gamma; f.rstd = a->rstd; f.dgamma = a->dgamma; f.dbeta = a->dbeta; f.dbias = a->dbias;
        f.fin_partial = a->fin_partial; f.fin_T = a->fin_T; f.fin_C = a->fin_C; f.fin_gamma = a->fin_gamma;
        f.dwf = a->dwf; f.dbf = a->dbf; f.fin_dgamma = a->fin_dgamma; f.fin_dbeta = a->fin_dbeta; f.fin_dbias = a->fin_dbias;
        f.scratch = scratch;
        uad_launch_grad_finish(f, st);
    } else {      // the model's order on its side stream
        if (a->fin_partial) {
            uad_launch_reduce_partials(a->fin_partial, a->fin_T, 3 * a->fin_C + 1, 1.0f, a->fin_red, st);
            uad_launch_final_gradfin(a->fin_red, a->fin_C, a->fin_gamma, a->rstd, a->dwf, a->dbf, a->fin_dgamma, a->fin_dbeta, a->fin_dbias, st);
        }
        if (a->slabs) uad_launch_reduce_partials(a->slabs, a->S, a->L, 1.0f, a->dW, st);
        if (a->colpart) uad_launch_bn_grad_finalize(a->colpart, a->T, a->C, a->gamma, a->rstd, a->dgamma, a->dbeta, a->dbias, st, scratch);
    }
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

// ------------------------------------------------------------------------------------------------ the step's small kernels, one launch each
// Each entry checks the domain the kernel itself assumes (read from the kernel: csrc/uad_loss.hip, uad_conv_first.hip, uad_optim.hip, uad_reduce.hip) and launches nothing outside it.
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int uad_op_final_blocks(int H, int W) { return (H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) ? 0 : uad_final_blocks_per_sample(H, W); }
int uad_op_final(const uad_final_t* a, void* stream) {
    if (!a) return fail(UAD_ERR_INVALID, "final: null argument");
    if (a->N < 1 || a->H < 1 || a->W < 1 || a->C < 1) return fail(UAD_ERR_INVALID, "final: sizes must be positive");
    // C / 4 lanes share a pixel and fold their dot product with xor-shuffles (a power of two), the block's 3 C + 2 partials sit in 200 LDS floats
    const int lpp = a->C / 4;
    if (a->C % 4 || (lpp & (lpp - 1)) || 3 * a->C + 2 > 200) return fail(UAD_ERR_UNSUPPORTED, "final: C must be 4, 8, 16, 32 or 64 (got %d)", a->C);
    if (a->N > 65535 || (long long)a->H * a->W > 0x7fffffffLL) return fail(UAD_ERR_UNSUPPORTED, "final: at most 65535 samples of fewer than 2^31 pixels");
    if (!a->c_last || !a->scale || !a->shift || !a->wf || !a->bf || !a->x || !a->x_hat || !a->rec_partial) return fail(UAD_ERR_INVALID, "final: null input or output");
    if (a->d_c && !a->red_partial) return fail(UAD_ERR_INVALID, "final: the backward needs red_partial");
    if (!al16(a->c_last) || !al16(a->scale) || !al16(a->shift) || !al16(a->wf) || !al16(a->d_c)) return fail(UAD_ERR_INVALID, "final: c_last, d_c, scale, shift and wf must be 16-byte aligned");
    UadFinalArgs f;
    f.N = a->N; f.H = a->H; f.W = a->W; f.C = a->C;
    f.c_last = a->c_last; f.scale = a->scale; f.shift = a->shift; f.alpha = a->alpha; f.mult = a->mult;
    f.wf = a->wf; f.bf = a->bf; f.x = a->x; f.x_hat = a->x_hat; f.l1_map = a->l1_map; f.rec_partial = a->rec_partial;
    f.d_c = a->d_c; f.red_partial = a->red_partial; f.inv_batch = a->inv_batch; f.dxhat_in = a->dxhat_in;
    uad_launch_final_fwd_bwd(f, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_op_reparam_fwd(int n, int n_vae, int zdim, const float* mu_raw, const float* ls_raw, const float* mask_mu, const float* mask_ls,
                       const float* mask_mu_ce, const float* eps, float* mu, float* ls, float* sigma, float* z, float* kl, void* stream) {
    if (n < 1 || zdim < 1 || n_vae < 0 || n_vae > n) return fail(UAD_ERR_INVALID, "reparam_fwd: n, zdim >= 1 and 0 <= n_vae <= n");
    if (!mu_raw || (n_vae > 0 && !ls_raw) || !mu || !ls || !sigma || !z || !kl) return fail(UAD_ERR_INVALID, "reparam_fwd: null input or output");
    uad_launch_reparam_fwd(n, n_vae, zdim, mu_raw, ls_raw, mask_mu, mask_ls, mask_mu_ce, eps, mu, ls, sigma, z, kl, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
int uad_op_reparam_bwd(int n, int n_vae, int zdim, const float* dz, const float* mu, const float* sigma, const float* eps, const float* mask_mu,
                       const float* mask_ls, const float* mask_mu_ce, float inv_batch, float* dmu_raw, float* dls_raw, void* stream) {
    if (n < 1 || zdim < 1 || n_vae < 0 || n_vae > n) return fail(UAD_ERR_INVALID, "reparam_bwd: n, zdim >= 1 and 0 <= n_vae <= n");
    if (!dz || (n_vae > 0 && (!mu || !sigma)) || !dmu_raw || !dls_raw) return fail(UAD_ERR_INVALID, "reparam_bwd: null input or output");
    uad_launch_reparam_bwd(n, n_vae, zdim, dz, mu, sigma, eps, mask_mu, mask_ls, mask_mu_ce, inv_batch, dmu_raw, dls_raw, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
int uad_op_loss_finalize(const float* rec_partial, int n, int n_vae, int bps, const float* kl, float inv_batch, float rec_scale, float* rec_per_sample,
                         float* scalars, void* stream) {
    if (n < 1 || bps < 1 || n_vae < 0 || n_vae > n) return fail(UAD_ERR_INVALID, "loss_finalize: n, bps >= 1 and 0 <= n_vae <= n");
    if (!rec_partial || !rec_per_sample || !scalars) return fail(UAD_ERR_INVALID, "loss_finalize: null input or output");
    uad_launch_loss_finalize(rec_partial, n, n_vae, bps, kl, inv_batch, rec_scale, rec_per_sample, scalars, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

// 2 tiled | 1 generic | 0 neither.  The generic kernel indexes a single input channel, reads the gradient as pairs of float4 and stages KS KS CS weights in LDS.
static int first_dgrad_form(const UadConvDesc& d, int form) {
    if (d.N < 1 || d.HB < 1 || d.WB < 1 || d.HS < 1 || d.WS < 1 || d.KS < 1 || d.S < 1 || d.P < 0) return 0;
    if (!form && uad_conv_first_dgrad_tiled(d)) return 2;
    if (d.CB != 1 || d.CS < 8 || d.CS % 8 || (size_t)d.KS * d.KS * d.CS * sizeof(float) > 65536) return 0;
    if (((size_t)d.N * d.HB * d.WB + 255) / 256 > 0x7fffffffull) return 0;
    return 1;
}
int uad_op_conv_first_dgrad_form(const uad_conv_desc_t* d, int form) { return (d && (form == 0 || form == 1)) ? first_dgrad_form(to_desc(d), form) : 0; }
int uad_op_conv_first_dgrad(const uad_conv_desc_t* dd, const float* g, const float* W, const float* x, const float* x_hat, float inv_batch, float* anomaly,
                            float* dx, const float* dxhat, float* x_upd, float restore_lr, int form, void* stream) {
    if (!dd || !g || !W) return fail(UAD_ERR_INVALID, "conv_first_dgrad: null argument");
    if (form != 0 && form != 1) return fail(UAD_ERR_INVALID, "conv_first_dgrad: form is 0 (the launcher's choice) or 1 (generic kernel)");
    const UadConvDesc d = to_desc(dd);
    if (!first_dgrad_form(d, form)) return fail(UAD_ERR_UNSUPPORTED, "conv_first_dgrad: one input channel, Cout a multiple of 8, weights within 64 KiB of LDS");
    if (!al16(g) || !al16(W)) return fail(UAD_ERR_INVALID, "conv_first_dgrad: g and W must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dxhat) {
        if (x || x_hat || anomaly) return fail(UAD_ERR_INVALID, "conv_first_dgrad: the restoration epilogue takes no x, x_hat or anomaly");
        if (!dx && !x_upd) return fail(UAD_ERR_INVALID, "conv_first_dgrad: the restoration epilogue needs dx or x_upd");
        uad_launch_conv_first_dgrad_restore(d, g, W, dxhat, dx, x_upd, restore_lr, st, form == 1);
    } else {
        if (x_upd) return fail(UAD_ERR_INVALID, "conv_first_dgrad: x_upd needs dxhat");
        if (x ? (!x_hat || (!dx && !anomaly)) : (x_hat || anomaly || !dx)) return fail(UAD_ERR_INVALID, "conv_first_dgrad: plain form: dx alone; anomaly form: x, x_hat and dx or anomaly");
        uad_launch_conv_first_dgrad(d, g, W, x, x_hat, inv_batch, anomaly, dx, st, form == 1);
    }
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_op_tv_dxhat(const float* x, const float* xh, int N, int H, int W, float inv_batch, float tv_lambda, float* dxhat, void* stream) {
    if (N < 1 || H < 1 || W < 1 || !x || !xh || !dxhat) return fail(UAD_ERR_INVALID, "tv_dxhat: sizes must be positive and pointers non-null");
    if (((unsigned long long)N * H * W + 255) / 256 > 0x7fffffffull) return fail(UAD_ERR_UNSUPPORTED, "tv_dxhat: too many pixels for one launch");
    uad_launch_tv_dxhat(x, xh, N, H, W, inv_batch, tv_lambda, dxhat, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_op_optim(int kind, float* p, const float* g, float* s1, float* s2, long long n, float lr, float momentum, float decay, float eps, float gscale,
                 const unsigned* fault, void* stream) {
    if (kind < 1 || kind > 3) return fail(UAD_ERR_UNSUPPORTED, "optim: kind is 1 (SGD), 2 (Momentum) or 3 (RMSProp); Adam is uad_op_adam");
    if (n < 1 || !p || !g || (kind >= 2 && !s1) || (kind == 3 && !s2)) return fail(UAD_ERR_INVALID, "optim: n >= 1, p, g and the slots of the kind (2: s1; 3: s1, s2)");
    if ((n + 255) / 256 > 0x7fffffffLL) return fail(UAD_ERR_UNSUPPORTED, "optim: too many elements for one launch");
    uad_launch_optim(kind, p, g, s1, s2, (size_t)n, lr, momentum, decay, eps, gscale, (hipStream_t)stream, fault);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_op_spatial_z_fwd(const float* c, const float* gamma, const float* beta, float rs0, float alpha, const float* mask, int rows, int C, float* z,
                         void* stream) {
    if (rows < 1 || C < 1 || !c || !gamma || !beta || !z) return fail(UAD_ERR_INVALID, "spatial_z_fwd: sizes must be positive and pointers non-null");
    if (C % 4) return fail(UAD_ERR_UNSUPPORTED, "spatial_z_fwd: C must be a multiple of 4 (got %d)", C);
    if (!al16(c) || !al16(gamma) || !al16(beta) || !al16(mask) || !al16(z)) return fail(UAD_ERR_INVALID, "spatial_z_fwd: operands must be 16-byte aligned");
    uad_launch_spatial_z_fwd(c, gamma, beta, rs0, alpha, mask, rows, C, z, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
int uad_op_spatial_z_bwd_blocks(int rows) { return rows < 1 ? 0 : uad_spatial_z_bwd_blocks(rows); }
int uad_op_spatial_z_bwd(const float* dz, const float* c, const float* gamma, const float* beta, float rs0, float alpha, const float* mask, int rows, int C,
                         float* dc, float* colpart, void* stream) {
    if (rows < 1 || C < 1 || !dz || !c || !gamma || !beta || !dc || !colpart) return fail(UAD_ERR_INVALID, "spatial_z_bwd: sizes must be positive and pointers non-null");
    // thread = (row lane, channel quad): the C / 4 quads must tile the 256 threads, or a row lane's LDS slot [rl][C] is summed from the wrong rows (C = 48)
    const int Q = C / 4;
    if (C % 4 || Q > 256 || (Q & (Q - 1))) return fail(UAD_ERR_UNSUPPORTED, "spatial_z_bwd: C / 4 must be a power of two <= 256 (got C = %d)", C);
    if (!al16(dz) || !al16(c) || !al16(gamma) || !al16(beta) || !al16(mask) || !al16(dc)) return fail(UAD_ERR_INVALID, "spatial_z_bwd: operands must be 16-byte aligned");
    uad_launch_spatial_z_bwd(dz, c, gamma, beta, rs0, alpha, mask, rows, C, dc, colpart, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

long long uad_op_colsum_scratch_floats(int rows, int C) { return (rows < 1 || C < 1) ? 0 : (long long)uad_colsum_scratch_floats(rows, C); }
int uad_op_colsum(const float* g, int rows, int C, float* out, float* scratch, void* stream) {
    if (rows < 1 || C < 1 || !g || !out) return fail(UAD_ERR_INVALID, "colsum: sizes must be positive and pointers non-null");
    if ((C + 31) / 32 > 0x7fffffff / 32) return fail(UAD_ERR_UNSUPPORTED, "colsum: too many columns for one launch");
    if (uad_colsum_scratch_floats(rows, C) > (size_t)C && !scratch) return fail(UAD_ERR_INVALID, "colsum: more than one row chunk needs the scratch (uad_op_colsum_scratch_floats)");
    uad_launch_colsum(g, rows, C, out, scratch, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

}  // extern "C"
