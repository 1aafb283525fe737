// uad_gan_ops.inc -- handle-less entries uad_op_gan_* (include/uad_hip.h): ONE launch of a small kernel of uad_gan_kernels.inc on caller-supplied device
// tensors, through the launch helper the phases use (uad_gan.hip: k_*, rowdot<>, avgpool_*, up2_*, z_act_*), asynchronously on `stream`; nothing is
// allocated.  uad_gan.hip includes this file inside its extern "C" block, where the kernels and helpers of its anonymous namespace are visible.  Each
// entry states the kernel's domain as host checks and launches NOTHING outside it (DESIGN section 28 has the table).  Not a translation unit of its own.

static bool gop_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool gop_grid_ok(long long n) { return n > 0 && (n + 255) / 256 <= 0x7fffffffLL; }
// the float4 kernels that give each of C / 4 channel quads 256 / (C / 4) row lanes of a 256-thread workgroup and fold them through 1024 floats of LDS:
// C / 4 must divide 256 (else row lane RL stores past the LDS array) and C <= 1024 (else no row lane exists and the row loop never advances);
// `by_thread`: the kernel writes its column partials with one thread per channel, so C <= 256
static int gop_check_qrl(const char* who, int C, bool by_thread) {
    if (C < 4 || C % 4) return fail(UAD_ERR_UNSUPPORTED, "%s: C = %d is no positive multiple of 4", who, C);
    if (C > 1024 || 256 % (C / 4)) return fail(UAD_ERR_UNSUPPORTED, "%s: C / 4 = %d must divide 256 (C <= 1024)", who, C / 4);
    if (by_thread && C > 256) return fail(UAD_ERR_UNSUPPORTED, "%s: C = %d > 256: the column partials are written by one thread per channel", who, C);
    return UAD_OK;
}
static bool gop_rule_ok(int max_blocks) { return max_blocks == kCoefColsumBlocks || max_blocks == kBnBwdBlocks || max_blocks == kGfinalBlocks; }
static int gop_done() {
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_op_gan_rows_blocks(int rows, int max_blocks) { return (rows < 1 || !gop_rule_ok(max_blocks)) ? 0 : row_split(rows, max_blocks).blocks; }

int uad_op_gan_bn_act_fwd(const float* c, const float* gamma, const float* beta, float rs0, float alpha, long long rows, int C, float* a, void* stream) {
    if (!c || !gamma || !beta || !a || rows < 1) return fail(UAD_ERR_INVALID, "gan_bn_act_fwd: a NULL tensor or rows < 1");
    if (C < 4 || C % 4) return fail(UAD_ERR_UNSUPPORTED, "gan_bn_act_fwd: C = %d is no positive multiple of 4", C);
    if (!gop_al16(c) || !gop_al16(gamma) || !gop_al16(beta) || !gop_al16(a)) return fail(UAD_ERR_INVALID, "gan_bn_act_fwd: operands must be 16-byte aligned");
    if (!gop_grid_ok(rows * (C / 4))) return fail(UAD_ERR_UNSUPPORTED, "gan_bn_act_fwd: too many elements for one grid");
    k_bn_act_fwd(c, gamma, beta, rs0, alpha, (size_t)rows * (C / 4), C, a, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_bn_act_bwd(const float* da, const float* c, const float* gamma, const float* beta, float rs0, float alpha, int rows, int C, int max_blocks,
                          float* dc, float* colpart, void* stream) {
    if (!da || !c || !gamma || !beta || !dc || !colpart || rows < 1) return fail(UAD_ERR_INVALID, "gan_bn_act_bwd: a NULL tensor or rows < 1");
    if (!gop_rule_ok(max_blocks)) return fail(UAD_ERR_INVALID, "gan_bn_act_bwd: max_blocks %d is none of the engine's rules (256, 512, 1024)", max_blocks);
    const int rc = gop_check_qrl("gan_bn_act_bwd", C, true);
    if (rc != UAD_OK) return rc;
    if (!gop_al16(da) || !gop_al16(c) || !gop_al16(gamma) || !gop_al16(beta) || !gop_al16(dc)) return fail(UAD_ERR_INVALID, "gan_bn_act_bwd: operands must be 16-byte aligned");
    k_bn_act_bwd(da, c, gamma, beta, rs0, alpha, rows, C, dc, colpart, max_blocks, (hipStream_t)stream);
    return gop_done();
}

int uad_op_gan_rowdot(int act, const float* feat, const float* w, const float* b, int rows, int C, float* out, void* stream) {
    if (!feat || !w || !b || !out || rows < 1) return fail(UAD_ERR_INVALID, "gan_rowdot: a NULL tensor or rows < 1");
    if (act < 0 || act > 2) return fail(UAD_ERR_INVALID, "gan_rowdot: act %d (0 none, 1 sigmoid, 2 tanh)", act);
    if (C < 4 || C % 4) return fail(UAD_ERR_UNSUPPORTED, "gan_rowdot: C = %d is no positive multiple of 4", C);
    const int lpr = C / 4 > 64 ? 64 : C / 4;
    if (lpr & (lpr - 1)) return fail(UAD_ERR_UNSUPPORTED, "gan_rowdot: min(C / 4, 64) = %d lanes per row is no power of two (the butterfly sum needs one)", lpr);
    if (!gop_al16(feat) || !gop_al16(w)) return fail(UAD_ERR_INVALID, "gan_rowdot: feat and w must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    if (act == 0) rowdot<0>(feat, w, b, rows, C, out, st);
    else if (act == 1) rowdot<1>(feat, w, b, rows, C, out, st);
    else rowdot<2>(feat, w, b, rows, C, out, st);
    return gop_done();
}
static int gop_check_groups(const char* who, long long rows, int rows_per_group) {
    if (rows_per_group < 1) return fail(UAD_ERR_INVALID, "%s: rows_per_group < 1", who);
    if (rows > 4ll * rows_per_group) return fail(UAD_ERR_INVALID, "%s: %lld rows are more than four groups of %d (four coefficients)", who, rows, rows_per_group);
    return UAD_OK;
}
int uad_op_gan_topgrad(const float* w, long long rows, int rows_per_group, int C, const float* coef4, float* out, void* stream) {
    if (!w || !coef4 || !out || rows < 1) return fail(UAD_ERR_INVALID, "gan_topgrad: a NULL argument or rows < 1");
    if (C < 4 || C % 4) return fail(UAD_ERR_UNSUPPORTED, "gan_topgrad: C = %d is no positive multiple of 4", C);
    const int rc = gop_check_groups("gan_topgrad", rows, rows_per_group);
    if (rc != UAD_OK) return rc;
    if (!gop_al16(w) || !gop_al16(out)) return fail(UAD_ERR_INVALID, "gan_topgrad: w and out must be 16-byte aligned");
    if (!gop_grid_ok(rows * (C / 4))) return fail(UAD_ERR_UNSUPPORTED, "gan_topgrad: too many elements for one grid");
    k_topgrad(w, rows_per_group, C, (size_t)rows, Coef4{{coef4[0], coef4[1], coef4[2], coef4[3]}}, out, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_coef_colsum(const float* feat, int rows, int rows_per_group, int C, const float* coef4, int max_blocks, float* partial, void* stream) {
    if (!feat || !coef4 || !partial || rows < 1) return fail(UAD_ERR_INVALID, "gan_coef_colsum: a NULL argument or rows < 1");
    if (!gop_rule_ok(max_blocks)) return fail(UAD_ERR_INVALID, "gan_coef_colsum: max_blocks %d is none of the engine's rules (256, 512, 1024)", max_blocks);
    int rc = gop_check_qrl("gan_coef_colsum", C, false);
    if (rc == UAD_OK) rc = gop_check_groups("gan_coef_colsum", rows, rows_per_group);
    if (rc != UAD_OK) return rc;
    if (!gop_al16(feat)) return fail(UAD_ERR_INVALID, "gan_coef_colsum: feat must be 16-byte aligned");
    k_coef_colsum(feat, rows, rows_per_group, C, Coef4{{coef4[0], coef4[1], coef4[2], coef4[3]}}, partial, max_blocks, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_gfinal_bwd(const float* dx, const float* x, const float* a, const float* wf, int rows, int C, int act, int max_blocks, float* da,
                          float* partial, void* stream) {
    if (!dx || !x || !wf || !da || rows < 1 || (partial && !a)) return fail(UAD_ERR_INVALID, "gan_gfinal_bwd: a NULL tensor (a is needed with partial) or rows < 1");
    if (act < 0 || act > 2) return fail(UAD_ERR_INVALID, "gan_gfinal_bwd: act %d (0 sigmoid, 1 tanh, 2 linear)", act);
    if (!gop_rule_ok(max_blocks)) return fail(UAD_ERR_INVALID, "gan_gfinal_bwd: max_blocks %d is none of the engine's rules (256, 512, 1024)", max_blocks);
    const int rc = gop_check_qrl("gan_gfinal_bwd", C, partial != nullptr);
    if (rc != UAD_OK) return rc;
    if (!gop_al16(wf) || !gop_al16(da) || (partial && !gop_al16(a))) return fail(UAD_ERR_INVALID, "gan_gfinal_bwd: a, wf and da must be 16-byte aligned");
    k_gfinal_bwd(dx, x, a, wf, rows, C, act, da, partial, max_blocks, (hipStream_t)stream);
    return gop_done();
}

int uad_op_gan_interp(const float* xg, const float* x, const float* alpha, int n, int HW, float* din, void* stream) {
    if (!xg || !x || !alpha || !din || n < 1 || HW < 1) return fail(UAD_ERR_INVALID, "gan_interp: a NULL tensor or an extent < 1");
    if (!gop_grid_ok((long long)n * HW)) return fail(UAD_ERR_UNSUPPORTED, "gan_interp: too many elements for one grid");
    k_interp(xg, x, alpha, HW, (size_t)n * HW, din, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_flat(int kind, const float* a, const float* b, const float* c, float coef, long long n, float* out, void* stream) {
    if (kind < UAD_GAN_FLAT_TANH || kind > UAD_GAN_FLAT_LRELU_BWD) return fail(UAD_ERR_INVALID, "gan_flat: unknown kind %d", kind);
    const bool need_a = kind != UAD_GAN_FLAT_ADD_SCALAR;
    const bool need_b = kind == UAD_GAN_FLAT_TANH_BWD || kind == UAD_GAN_FLAT_DIFF_SCALE || kind == UAD_GAN_FLAT_DIFF_SCALE_ACC || kind == UAD_GAN_FLAT_SIGN_SCALE ||
                        kind == UAD_GAN_FLAT_ADD_SCALAR || kind == UAD_GAN_FLAT_LRELU_BWD;
    if (!out || (need_a && !a) || (need_b && !b) || n < 1) return fail(UAD_ERR_INVALID, "gan_flat: kind %d: a NULL tensor that is needed or n < 1", kind);
    const bool f4k = kind == UAD_GAN_FLAT_LRELU_FWD || kind == UAD_GAN_FLAT_LRELU_BWD;
    if (f4k && n % 4) return fail(UAD_ERR_UNSUPPORTED, "gan_flat: the LeakyReLU kernels take a multiple of 4 elements");
    if (f4k && (!gop_al16(a) || !gop_al16(out) || (need_b && !gop_al16(b)))) return fail(UAD_ERR_INVALID, "gan_flat: the LeakyReLU operands must be 16-byte aligned");
    if (!gop_grid_ok(f4k ? n / 4 : n)) return fail(UAD_ERR_UNSUPPORTED, "gan_flat: too many elements for one grid");
    const hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)n;
    switch (kind) {
        case UAD_GAN_FLAT_TANH: k_tanh(a, N, out, st); break;
        case UAD_GAN_FLAT_TANH_BWD: k_tanh_bwd(a, b, c, N, out, st); break;
        case UAD_GAN_FLAT_DIFF_SCALE: k_diff_scale<false>(a, b, coef, N, out, st); break;
        case UAD_GAN_FLAT_DIFF_SCALE_ACC: k_diff_scale<true>(a, b, coef, N, out, st); break;
        case UAD_GAN_FLAT_SIGN_SCALE: k_sign_scale(a, b, coef, N, out, st); break;
        case UAD_GAN_FLAT_ADD: k_add(out, a, N, st); break;
        case UAD_GAN_FLAT_ADD_SCALAR: k_add_scalar(out, b, N, st); break;
        case UAD_GAN_FLAT_LRELU_FWD: z_act_fwd(a, N, out, st, coef); break;
        default: z_act_bwd(a, b, N, out, st, coef); break;
    }
    return gop_done();
}
int uad_op_gan_sum_blocks(void) { return kSumBlocks; }
int uad_op_gan_sum(int mode, const float* a, const float* b, long long n, float* map, float* partial, void* stream) {
    if (mode < 0 || mode > 2) return fail(UAD_ERR_INVALID, "gan_sum: mode %d (0 sum a, 1 sum (a - b)^2, 2 sum |a - b|)", mode);
    if (!a || !partial || n < 1 || (mode != 0 && !b) || (mode != 2 && map)) return fail(UAD_ERR_INVALID, "gan_sum: a NULL tensor that is needed, n < 1, or a map outside mode 2");
    const hipStream_t st = (hipStream_t)stream;
    if (mode == 0) k_sum<0>(a, b, (size_t)n, nullptr, partial, st);
    else if (mode == 1) k_sum<1>(a, b, (size_t)n, nullptr, partial, st);
    else k_sum<2>(a, b, (size_t)n, map, partial, st);
    return gop_done();
}
static bool gop_pen_ok(int n, int H, int W) { return n >= 1 && H >= 1 && W >= 1 && (long long)n * W <= 0x7fffffffLL - 256; }
int uad_op_gan_pen_col_blocks(int n, int W) { return gop_pen_ok(n, 1, W) ? (int)blocks256((size_t)n * W) : 0; }
int uad_op_gan_pen_col(const float* g, int n, int H, int W, float* s, float* partial, void* stream) {
    if (!g || !s || !partial) return fail(UAD_ERR_INVALID, "gan_pen_col: a NULL tensor");
    if (!gop_pen_ok(n, H, W)) return fail(UAD_ERR_INVALID, "gan_pen_col: an extent < 1 or n * W beyond the 32-bit column index");
    k_pen_col(g, n, H, W, s, partial, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_pen_grad(const float* g, const float* s, float coef, int n, int H, int W, float* out, void* stream) {
    if (!g || !s || !out) return fail(UAD_ERR_INVALID, "gan_pen_grad: a NULL tensor");
    if (!gop_pen_ok(n, H, W)) return fail(UAD_ERR_INVALID, "gan_pen_grad: an extent < 1 or n * W beyond the 32-bit column index");
    if (!gop_grid_ok((long long)n * H * W)) return fail(UAD_ERR_UNSUPPORTED, "gan_pen_grad: too many elements for one grid");
    k_pen_grad(g, s, coef, H, W, (size_t)n * H * W, out, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_pool(int kind, const float* in, int N, int H, int C, float* out, void* stream) {
    if (kind < UAD_GAN_POOL_AVG_FWD || kind > UAD_GAN_POOL_UP2_BWD) return fail(UAD_ERR_INVALID, "gan_pool: unknown kind %d", kind);
    if (!in || !out || N < 1 || H < 1) return fail(UAD_ERR_INVALID, "gan_pool: a NULL tensor or an extent < 1");
    if (C < 4 || C % 4) return fail(UAD_ERR_UNSUPPORTED, "gan_pool: C = %d is no positive multiple of 4", C);
    const bool avg = kind == UAD_GAN_POOL_AVG_FWD || kind == UAD_GAN_POOL_AVG_BWD;
    if (avg && H % 2) return fail(UAD_ERR_UNSUPPORTED, "gan_pool: 2 x 2 average pooling needs an even H (got %d)", H);
    if (!gop_al16(in) || !gop_al16(out)) return fail(UAD_ERR_INVALID, "gan_pool: operands must be 16-byte aligned");
    if (!gop_grid_ok((long long)N * H * H * (C / 4) * (kind == UAD_GAN_POOL_UP2_FWD ? 4 : 1))) return fail(UAD_ERR_UNSUPPORTED, "gan_pool: too many elements for one grid");
    const hipStream_t st = (hipStream_t)stream;
    if (kind == UAD_GAN_POOL_AVG_FWD) avgpool_fwd(in, N, H, C, out, st);
    else if (kind == UAD_GAN_POOL_AVG_BWD) avgpool_bwd(in, N, H, C, out, st);
    else if (kind == UAD_GAN_POOL_UP2_FWD) up2_fwd(in, N, H, C, out, st);
    else up2_bwd(in, N, H, C, out, st);
    return gop_done();
}
int uad_op_gan_flip_taps(const float* w, int T, int C, float* out, void* stream) {
    if (!w || !out || T < 1 || C < 1 || w == out) return fail(UAD_ERR_INVALID, "gan_flip_taps: a NULL tensor, an extent < 1, or out aliasing w");
    if ((long long)T * C > 0x7fffffffLL - 256) return fail(UAD_ERR_UNSUPPORTED, "gan_flip_taps: T * C beyond the 32-bit element index");
    k_flip_taps(w, T, C, out, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_combine(int phase, const float* raw, float kappa, float* out, void* stream) {
    if (!raw || !out || phase < 0 || phase > 7) return fail(UAD_ERR_INVALID, "gan_combine: a NULL tensor or a phase outside 0 .. 7");
    k_combine(phase, raw, kappa, out, (hipStream_t)stream);
    return gop_done();
}
int uad_op_gan_critic(const uad_gan_critic_t* c, int n, void* stream) {
    if (!c || n < 1) return fail(UAD_ERR_INVALID, "gan_critic: NULL arguments or n < 1");
    if (c->zd < 1 || c->h1 < 1 || c->h2 < 1) return fail(UAD_ERR_INVALID, "gan_critic: a layer width < 1");
    if (c->zd > kCritMaxZ || c->h1 > kCritMaxH || c->h2 > kCritMaxH)
        return fail(UAD_ERR_UNSUPPORTED, "gan_critic: zd %d / h1 %d / h2 %d beyond the kernel's LDS arrays (%d / %d / %d)", c->zd, c->h1, c->h2, kCritMaxZ, kCritMaxH, kCritMaxH);
    if ((c->mode != 0 && c->mode != 1) || (c->hat_mode != 0 && c->hat_mode != 1)) return fail(UAD_ERR_INVALID, "gan_critic: mode and hat_mode are 0 or 1");
    if (!c->W1 || !c->b1 || !c->W2 || !c->b2 || !c->W3 || !c->b3 || !c->zf || !c->d_fake) return fail(UAD_ERR_INVALID, "gan_critic: a NULL parameter tensor, zf or d_fake");
    if (c->mode == 0 && (!c->zr || !c->eps || !c->d_real || !c->pen || !c->slab)) return fail(UAD_ERR_INVALID, "gan_critic: the critic step needs zr, eps, d_real, pen and slab");
    if (c->mode == 1 && !c->dz_fake) return fail(UAD_ERR_INVALID, "gan_critic: the generator step needs dz_fake");
    CriticArgs a;
    memset(&a, 0, sizeof a);
    a.zd = c->zd; a.h1 = c->h1; a.h2 = c->h2; a.mode = c->mode; a.hat_mode = c->hat_mode;
    a.W1 = c->W1; a.b1 = c->b1; a.W2 = c->W2; a.b2 = c->b2; a.W3 = c->W3; a.b3 = c->b3;
    a.zf = c->zf; a.zr = c->zr; a.eps = c->eps; a.inv_n = c->inv_n; a.scale = c->scale;
    a.d_fake = c->d_fake; a.d_real = c->d_real; a.pen = c->pen; a.slab = c->slab; a.dz_fake = c->dz_fake;
    k_critic(a, n, (hipStream_t)stream);
    return gop_done();
}
