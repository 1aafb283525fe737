// uad_gan_create.inc -- uad_gan_create and the per-variant constructors (parameter tables in TF first-call order, device buffers, workspace
// sizing) of the materialised-graph handle; included by uad_gan.hip inside its extern "C" block.  Not a translation unit of its own.
// Each constructor is gan_new, its parameter table, gan_alloc_flat, then its own activations and scratch.
// What every constructor starts from.  packs: the graph has k5 layers, whose packed copies refresh_packs keeps (stale until the first phase); without
// them nothing is ever packed.
static uad_gan* gan_new(const uad_gan_config_t* cfg, int variant, int npool, bool packs) {
    uad_gan* m = new uad_gan();
    m->cfg = *cfg; m->variant = variant; m->npool = npool; m->exact_from = -1;
    m->nparams = 0; m->math = UAD_MATH_F32; m->packed_valid = !packs; m->pack_all = packs; m->dirty_lo = (1ll << 62); m->dirty_hi = -1;
    m->step[0] = m->step[1] = m->step[2] = 0;
    return m;
}
// ... and, once its parameter table stands, the flat buffers of the core (the packs: a handle gan_new was told has them)
static int gan_alloc_flat(uad_gan* m) {
    const size_t n = (size_t)m->nparams;
    int rc = dev_alloc(m, &m->params, n, "params");
    if (rc == UAD_OK) rc = dev_alloc(m, &m->grads, n, "grads");
    for (float** p : {&m->adam_m, &m->adam_v}) if (rc == UAD_OK) rc = dev_alloc(m, p, n);
    if (m->pack_all) for (float** p : {&m->wpack_f, &m->wpack_d, &m->wpack16_f, &m->wpack16_d}) if (rc == UAD_OK) rc = dev_alloc(m, p, n);
    return rc;
}

// ---- handle of the ResNet variant (models/fanogan_schlegl.py); parameter table in TF first-call order ----
static int create_resnet(const uad_gan_config_t* cfg, uad_gan_t** out) {
    const int H = cfg->height, ir = cfg->inter_res, dim = cfg->dim > 0 ? cfg->dim : 64;
    if (H != 8 * ir) return fail(UAD_ERR_UNSUPPORTED, "ResNet f-AnoGAN: the generator upsamples 8x, height must be 8 * inter_res (fanogan_schlegl.py:28,121-133)");
    if (dim % 32 || dim > 64) return fail(UAD_ERR_UNSUPPORTED, "ResNet f-AnoGAN: dim must be 32 or 64");
    if (ir < 2) return fail(UAD_ERR_UNSUPPORTED, "inter_res >= 2 needed");
    uad_gan* m = gan_new(cfg, 1, 3, true);
    m->dim = dim; m->generic16 = false; m->adam_m2 = m->adam_v2 = nullptr; m->e_sw = m->e_sb = -1;
    char nm[160];
    int cin = 1, res = H;
    for (int i = 0; i < 3; ++i) {
        const int f = (32 << i) < 128 ? (32 << i) : 128;
        Block L;
        L.d = UadConvDesc{1, res, res, cin, res / 2, res / 2, f, 5, 2, 1};
        snprintf(nm, sizeof nm, "Encoder/enc_conv2D_%d/kernel", i); L.w = add_tensor(m, nm, 4, 5, 5, cin, f);
        snprintf(nm, sizeof nm, "Encoder/enc_conv2D_%d/bias", i); L.b = add_tensor(m, nm, 1, f, 1, 1, 1);
        std::string bs = i == 0 ? "Encoder/batch_normalization" : "Encoder/batch_normalization_" + std::to_string(i);
        L.gamma = add_tensor(m, bs + "/gamma", 1, f, 1, 1, 1);
        L.beta = add_tensor(m, bs + "/beta", 1, f, 1, 1, 1);
        L.H = L.W = res / 2; L.C = f;
        m->E.push_back(L);
        cin = f; res /= 2;
    }
    m->cenc = cin; m->cmid = 0; m->flat = ir * ir * cin;
    m->e_cw = m->e_cb = -1;
    m->e_dw = add_tensor(m, "Encoder/dense/kernel", 2, m->flat, cfg->zdim, 1, 1);
    m->e_db = add_tensor(m, "Encoder/dense/bias", 1, cfg->zdim, 1, 1, 1);
    m->grp_off[UAD_GAN_ENCODER] = 0; m->grp_cnt[UAD_GAN_ENCODER] = m->nparams;
    int ln = 0;
    std::map<std::string, int> cnt;
    auto ln_name = [&](const char* scope) { std::string r = std::string(scope) + (ln == 0 ? "layer_normalization" : "layer_normalization_" + std::to_string(ln)); ++ln; return r; };
    auto tf_name = [&](const char* scope, const char* base) {
        const std::string key = std::string(scope) + base;
        const int k = cnt[key]++;
        return k == 0 ? key : key + "_" + std::to_string(k);
    };
    const int flatg = ir * ir * 8 * dim;
    m->g_dw = add_tensor(m, "Generator/dense/kernel", 2, cfg->zdim, flatg, 1, 1);
    m->g_db = add_tensor(m, "Generator/dense/bias", 1, flatg, 1, 1, 1);
    m->g_cw = m->g_cb = m->g_ln0g = m->g_ln0b = -1;
    auto make_block = [&](bool gen, const char* scope, int Hin, int Cin, int Cout, int stride) {
        RB B;
        memset(&B, 0, sizeof B);
        B.gen = gen; B.stride = stride; B.Hin = Hin; B.Cin = Cin; B.Cout = Cout;
        B.Hout = gen ? Hin * stride : Hin / stride;
        std::string s1 = ln_name(scope);
        B.ln1g = add_tensor(m, s1 + "/gamma", 2, Hin, Hin, 1, 1); B.ln1b = add_tensor(m, s1 + "/beta", 2, Hin, Hin, 1, 1);
        std::string c1 = tf_name(scope, "conv2d");
        B.w1 = add_tensor(m, c1 + "/kernel", 4, 3, 3, Cin, Cout); B.b1 = add_tensor(m, c1 + "/bias", 1, Cout, 1, 1, 1);
        std::string s2 = ln_name(scope);
        B.ln2g = add_tensor(m, s2 + "/gamma", 2, Hin, Hin, 1, 1); B.ln2b = add_tensor(m, s2 + "/beta", 2, Hin, Hin, 1, 1);
        std::string c2 = tf_name(scope, gen ? "conv2d_transpose" : "conv2d");
        B.w2 = add_tensor(m, c2 + "/kernel", 4, 3, 3, Cout, Cout); B.b2 = add_tensor(m, c2 + "/bias", 1, Cout, 1, 1, 1);
        B.ws = B.bs = -1;
        if (stride == 2) {
            std::string sh = tf_name(scope, gen ? "conv2d_transpose" : "conv2d");
            if (gen) B.ws = add_tensor(m, sh + "/kernel", 4, 1, 1, Cout, Cin); else B.ws = add_tensor(m, sh + "/kernel", 4, 1, 1, Cin, Cout);
            B.bs = add_tensor(m, sh + "/bias", 1, Cout, 1, 1, 1);
        }
        B.d1 = UadConvDesc{1, Hin, Hin, Cin, Hin, Hin, Cout, 3, 1, 1};
        const int P2 = stride == 1 ? 1 : 0;                       // TF SAME: k3 s1 pads 1 before; k3 s2 on an even size pads 0 before
        if (gen) {
            B.d2 = UadConvDesc{1, B.Hout, B.Hout, Cout, Hin, Hin, Cout, 3, stride, P2};     // big = output of the transposed conv
            B.ds = UadConvDesc{1, B.Hout, B.Hout, Cout, Hin, Hin, Cin, 1, 2, 0};
        } else {
            B.d2 = UadConvDesc{1, Hin, Hin, Cout, B.Hout, B.Hout, Cout, 3, stride, P2};
            B.ds = UadConvDesc{1, Hin, Hin, Cin, Hin, Hin, Cout, 1, 1, 0};
        }
        B.sx = (size_t)Hin * Hin * Cin; B.sc1 = (size_t)Hin * Hin * Cout; B.sout = (size_t)B.Hout * B.Hout * Cout;
        return B;
    };
    {
        const int chans[4] = {8 * dim, 4 * dim, 2 * dim, dim}, strides[4] = {1, 2, 2, 2};
        int c = 8 * dim, r = ir;
        for (int k = 0; k < 4; ++k) { m->GB.push_back(make_block(true, "Generator/", r, c, chans[k], strides[k])); c = chans[k]; r *= strides[k]; }
        const std::string sl = ln_name("Generator/");
        m->s_glg = add_tensor(m, sl + "/gamma", 2, r, r, 1, 1); m->s_glb = add_tensor(m, sl + "/beta", 2, r, r, 1, 1);
        const std::string gf = tf_name("Generator/", "conv2d");
        m->g_fw = add_tensor(m, gf + "/kernel", 4, 1, 1, c, 1); m->g_fb = add_tensor(m, gf + "/bias", 1, 1, 1, 1, 1);
    }
    m->grp_off[UAD_GAN_GENERATOR] = m->grp_cnt[UAD_GAN_ENCODER];
    m->grp_cnt[UAD_GAN_GENERATOR] = m->nparams - m->grp_off[UAD_GAN_GENERATOR];
    {
        const std::string d0 = tf_name("Discriminator/", "conv2d");
        m->s_d0w = add_tensor(m, d0 + "/kernel", 4, 3, 3, 1, dim); m->s_d0b = add_tensor(m, d0 + "/bias", 1, dim, 1, 1, 1);
        m->s_d0 = UadConvDesc{1, H, H, 1, H, H, dim, 3, 1, 1};
        const int chans[4] = {2 * dim, 4 * dim, 8 * dim, 8 * dim}, strides[4] = {2, 2, 2, 1};
        int c = dim, r = H;
        for (int k = 0; k < 4; ++k) { m->DB.push_back(make_block(false, "Discriminator/", r, c, chans[k], strides[k])); c = chans[k]; r /= strides[k]; }
        m->d_hw = add_tensor(m, "Discriminator/dense/kernel", 2, c, 1, 1, 1);
        m->d_hb = add_tensor(m, "Discriminator/dense/bias", 1, 1, 1, 1, 1);
    }
    m->grp_off[UAD_GAN_DISCRIMINATOR] = m->grp_off[UAD_GAN_GENERATOR] + m->grp_cnt[UAD_GAN_GENERATOR];
    m->grp_cnt[UAD_GAN_DISCRIMINATOR] = m->nparams - m->grp_off[UAD_GAN_DISCRIMINATOR];

    // ---- device memory ----
    const size_t NB = (size_t)cfg->max_batch, HW = (size_t)H * H;
    int rc = gan_alloc_flat(m);
#define ALLOC(ptr, n, name) if (rc == UAD_OK) rc = dev_alloc(m, &(ptr), (n), name)
    if (!getenv("UAD_NO_X6")) {       // three-plane packs of the k3 kernels for the bf16x6 exact passes (UAD_NO_X6=1: those passes on the fp32 MFMA kernels)
        ALLOC(m->wpack3_f, (size_t)m->nparams * 2, nullptr); ALLOC(m->wpack3_d, (size_t)m->nparams * 2, nullptr);
    }
    size_t maxact = 3 * NB * HW, max_ta = 0, max_tb = 0, max_sp = 0, max_q = 0, lnp_g = 0;
    m->ec.resize(3); m->ea.resize(4, nullptr);
    for (int i = 0; i < 3; ++i) {
        const size_t sz = NB * asz(m->E[i]);
        snprintf(nm, sizeof nm, "ec%d", i); ALLOC(m->ec[i], sz, nm);
        snprintf(nm, sizeof nm, "ea%d", i + 1); ALLOC(m->ea[i + 1], sz, nm);
        if (sz > maxact) maxact = sz;
    }
    ALLOC(m->zr, NB * cfg->zdim, "zr"); ALLOC(m->z, NB * cfg->zdim, "z"); ALLOC(m->xg, NB * HW, "xg");
    ALLOC(m->s_g0, NB * flatg, "sg_x0"); ALLOC(m->s_dg0, NB * flatg, nullptr);
    auto alloc_block = [&](RB& B, float* X, float* DX, size_t cap_act, size_t cap_fwd, bool critic, const char* tag, int k) {
        B.X = X; B.DX = DX;
        snprintf(nm, sizeof nm, "%s_h1_%d", tag, k); ALLOC(B.H1, cap_act * B.sx, nm);
        snprintf(nm, sizeof nm, "%s_c1_%d", tag, k); ALLOC(B.C1, cap_fwd * B.sc1, nm);
        snprintf(nm, sizeof nm, "%s_h2_%d", tag, k); ALLOC(B.H2, cap_act * B.sc1, nm);
        snprintf(nm, sizeof nm, "%s_out_%d", tag, k); ALLOC(B.OUT, cap_act * B.sout, nm);
        ALLOC(B.ST1, cap_fwd * 2 * B.Cin, nullptr); ALLOC(B.ST2, cap_fwd * 2 * B.Cout, nullptr);
        snprintf(nm, sizeof nm, "%s_dout_%d", tag, k); ALLOC(B.DOUT, cap_act * B.sout, nm);
        snprintf(nm, sizeof nm, "%s_g1_%d", tag, k); ALLOC(B.G1, cap_act * B.sc1, nm);
        if (critic && B.ws >= 0) ALLOC(B.DSC, cap_act * B.sc1, nullptr);
        if (critic) {
            snprintf(nm, sizeof nm, "%s_v1_%d", tag, k); ALLOC(B.V1, NB * B.sx, nm);
            snprintf(nm, sizeof nm, "%s_v2_%d", tag, k); ALLOC(B.V2, NB * B.sc1, nm);
            snprintf(nm, sizeof nm, "%s_injx_%d", tag, k); ALLOC(B.INJX, NB * B.sx, nm);
            snprintf(nm, sizeof nm, "%s_injc1_%d", tag, k); ALLOC(B.INJC1, NB * B.sc1, nm);
        }
        ALLOC(B.LP1, cap_act * (B.Cin / 32) * 2 * B.Hin * B.Hin, nullptr);
        ALLOC(B.LP2, cap_act * (B.Cout / 32) * 2 * B.Hin * B.Hin, nullptr);
        if (cap_fwd * B.sc1 > max_ta) max_ta = cap_fwd * B.sc1;
        if (cap_fwd * B.sx > max_tb) max_tb = cap_fwd * B.sx;
        if (cap_fwd * B.sout > max_sp) max_sp = cap_fwd * B.sout;
        if (NB * B.sc1 > max_q) max_q = NB * B.sc1;
    };
    {
        float* X = m->s_g0; float* DX = m->s_dg0;
        for (size_t k = 0; k < m->GB.size(); ++k) { alloc_block(m->GB[k], X, DX, NB, NB, false, "sg", (int)k); X = m->GB[k].OUT; DX = m->GB[k].DOUT; }
        const RB& L = m->GB.back();
        ALLOC(m->s_hf, NB * L.sout, "sg_hf"); ALLOC(m->s_stf, NB * 2 * L.Cout, nullptr);
        lnp_g = NB * (L.Cout / 32) * 2 * L.Hout * L.Hout;
        if (NB * L.sout > maxact) maxact = NB * L.sout;
    }
    ALLOC(m->lnpart_g, lnp_g, nullptr);
    ALLOC(m->din, 4 * NB * HW, "din");
    ALLOC(m->s_out0, 4 * NB * HW * dim, "sd_out0"); ALLOC(m->s_dout0, 4 * NB * HW * dim, "sd_dout0");
    {
        float* X = m->s_out0; float* DX = m->s_dout0;
        for (size_t k = 0; k < m->DB.size(); ++k) { alloc_block(m->DB[k], X, DX, 4 * NB, 3 * NB, true, "sd", (int)k); X = m->DB[k].OUT; DX = m->DB[k].DOUT; }
    }
    ALLOC(m->s_ta, max_ta, nullptr); ALLOC(m->s_tb, max_tb, nullptr); ALLOC(m->s_sp, max_sp, nullptr); ALLOC(m->s_sct, max_ta, nullptr);
    ALLOC(m->Q, max_q, "Q");
    ALLOC(m->Dd, 3 * NB * ir * ir, "Dd"); ALLOC(m->Gx, NB * HW, "Gx"); ALLOC(m->slopes, NB * H, "slopes");
    ALLOC(m->Ga, maxact, "Ga"); ALLOC(m->Gb, maxact, "Gb");
    ALLOC(m->dxbuf, NB * HW, "dx"); ALLOC(m->dzbuf, NB * cfg->zdim, "dz"); ALLOC(m->dzr, NB * cfg->zdim, nullptr);
    {
        size_t wp = 0, need = (size_t)4 << 20;
        auto wp_need = [&](UadConvDesc d, size_t n) { d.N = (int)n; size_t v = uad_conv_w_partial_floats(d); if (v > wp) wp = v; };
        auto want = [&](UadConvDesc d, size_t n) { d.N = (int)n; for (int f = 0; f < 2; ++f) { size_t v = uad_conv_ws_floats(d, f != 0, false); if (v > need) need = v; } };
        for (size_t i = 1; i < m->E.size(); ++i) { wp_need(m->E[i].d, NB); UadConvDesc d = m->E[i].d; d.N = (int)NB; for (int f = 0; f < 2; ++f) { size_t v = uad_conv_ws_floats(d, f != 0, true); if (v > need) need = v; } }
        for (auto& B : m->GB) { wp_need(B.d1, NB); wp_need(B.d2, NB); want(B.d1, NB); want(B.d2, NB); if (B.ws >= 0) { wp_need(B.ds, NB); want(B.ds, NB); } }
        for (auto& B : m->DB) { wp_need(B.d1, 4 * NB); wp_need(B.d2, 4 * NB); want(B.d1, 3 * NB); want(B.d2, 3 * NB); want(B.d1, NB); want(B.d2, NB);
                                if (B.ws >= 0) { wp_need(B.ds, 4 * NB); want(B.ds, 3 * NB); want(B.ds, NB); } }
        wp_need(dense_desc(1, m->flat, cfg->zdim), NB); wp_need(dense_desc(1, cfg->zdim, flatg), NB);
        want(dense_desc(1, m->flat, cfg->zdim), NB); want(dense_desc(1, cfg->zdim, flatg), NB);
        { UadConvDesc d0 = m->s_d0; d0.N = (int)(4 * NB); size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        { UadConvDesc d0 = m->E[0].d; d0.N = (int)NB; size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        ALLOC(m->wpartial, wp, nullptr);
        m->ws.floats = need; m->ws.ptr = nullptr; m->ws.counters = nullptr; m->ws.ncounters = 0;      // no in-kernel split-K reduction on this handle
        ALLOC(m->ws.ptr, need, nullptr);
    }
    ALLOC(m->colscratch, kUadColsumScratchFloats, nullptr); ALLOC(m->colpart, (size_t)kBnBwdBlocks * 2 * 128, nullptr);
    ALLOC(m->redpart, 1024, nullptr); ALLOC(m->raw, 16, "raw"); ALLOC(m->scalars_own, 16, nullptr);
    ALLOC(m->finpart, (size_t)1024 * 520, nullptr);
#undef ALLOC
    if (rc != UAD_OK) { uad_gan_destroy(m); return rc; }
    *out = m;
    return UAD_OK;
}

// ---- handle of the AAE family (ConstrainedAE / AAE / ConstrainedAAE); parameter table in TF first-call order ----

static int create_zimmerer(const uad_gan_config_t* cfg, uad_gan_t** out) {
    const int H = cfg->height, zd = cfg->zdim;
    if (H < 32 || H % 16) return fail(UAD_ERR_UNSUPPORTED, "Zimmerer VAE: height must be a power of two >= 32");
    if (cfg->inter_res != H / 16) return fail(UAD_ERR_INVALID, "Zimmerer VAE: intermediateResolutions must be height / 16 (four stride-2 stages)");
    uad_gan* m = gan_new(cfg, UAD_GAN_AAE, 4, false);
    const bool ce = cfg->aae_kind == 5;
    const std::string se = ce ? "Encoder/" : "", sb = ce ? "Bottleneck/" : "", sdc = ce ? "Decoder/" : "";
    m->aae_kind = cfg->aae_kind; m->zim = true; m->zim_ce = ce; m->gmv = false; m->a_constrained = m->a_critic = false;
    m->dim = 0; m->generic16 = false; m->adam_m2 = m->adam_v2 = nullptr; m->e_sw = m->e_sb = -1; m->a_zw = m->a_zb = -1;
    static const int ef[4] = {16, 64, 256, 1024}, gf[4] = {1024, 256, 64, 16};
    char nm[160];
    int cin = 1, res = H;
    for (int i = 0; i < 4; ++i) {
        Block L;
        L.d = UadConvDesc{1, res, res, cin, res / 2, res / 2, ef[i], 4, 2, 1};
        snprintf(nm, sizeof nm, "enc_conv2D_%d/kernel", i + 1); L.w = add_tensor(m, se + nm, 4, 4, 4, cin, ef[i]);
        snprintf(nm, sizeof nm, "enc_conv2D_%d/bias", i + 1); L.b = add_tensor(m, se + nm, 1, ef[i], 1, 1, 1);
        L.gamma = L.beta = -1; L.H = L.W = res / 2; L.C = ef[i];
        m->E.push_back(L);
        cin = ef[i]; res /= 2;
    }
    const int r = res;
    m->cenc = 1024; m->cmid = 1024; m->flat = r * r * 1024;
    m->z_muw = add_tensor(m, sb + "dense/kernel", 2, m->flat, zd, 1, 1); m->z_mub = add_tensor(m, sb + "dense/bias", 1, zd, 1, 1, 1);
    m->z_lsw = add_tensor(m, sb + "dense_1/kernel", 2, m->flat, zd, 1, 1); m->z_lsb = add_tensor(m, sb + "dense_1/bias", 1, zd, 1, 1, 1);
    m->z_dw = add_tensor(m, sb + "dense_2/kernel", 2, zd, m->flat, 1, 1); m->z_db = add_tensor(m, sb + "dense_2/bias", 1, m->flat, 1, 1, 1);
    cin = 1024;
    for (int i = 0; i < 4; ++i) {
        Block L;
        L.d = UadConvDesc{1, res * 2, res * 2, gf[i], res, res, cin, 4, 2, 1};
        snprintf(nm, sizeof nm, "dec_Conv2DT_%d/kernel", i + 1); L.w = add_tensor(m, sdc + nm, 4, 4, 4, gf[i], cin);
        snprintf(nm, sizeof nm, "dec_Conv2DT_%d/bias", i + 1); L.b = add_tensor(m, sdc + nm, 1, gf[i], 1, 1, 1);
        res *= 2;
        L.gamma = L.beta = -1; L.H = L.W = res; L.C = gf[i];
        m->G.push_back(L);
        cin = gf[i];
    }
    m->z_fw = add_tensor(m, sdc + "dec_Conv2D_final/kernel", 4, 4, 4, 16, 1); m->z_fb = add_tensor(m, sdc + "dec_Conv2D_final/bias", 1, 1, 1, 1, 1);
    m->z_fd = UadConvDesc{1, H, H, 1, H, H, 16, 4, 1, 2};
    m->g_fw = m->z_fw; m->g_fb = m->z_fb;
    for (int k = 0; k < 3; ++k) { m->grp_off[k] = 0; m->grp_cnt[k] = m->nparams; }      // one optimizer over every variable

    const size_t NB = (size_t)cfg->max_batch * (ce ? 2 : 1), HW = (size_t)H * H;      // ceVAE: both branches in one pass
    int rc = gan_alloc_flat(m);
#define ALLOC(ptr, n, name) if (rc == UAD_OK) rc = dev_alloc(m, &(ptr), (n), name)
    m->wpack_f = m->wpack_d = m->wpack16_f = m->wpack16_d = nullptr;
    m->a_xcat = m->z_l1 = nullptr;
    if (ce) { ALLOC(m->a_xcat, NB * HW, nullptr); ALLOC(m->z_l1, NB * HW, nullptr); }
    size_t maxact = NB * HW * 16;
    m->ec.resize(4); m->ea.resize(5, nullptr);
    for (int i = 0; i < 4; ++i) {
        const size_t sz = NB * asz(m->E[i]);
        snprintf(nm, sizeof nm, "ec%d", i); ALLOC(m->ec[i], sz, nm);
        snprintf(nm, sizeof nm, "ea%d", i + 1); ALLOC(m->ea[i + 1], sz, nm);
        if (sz > maxact) maxact = sz;
    }
    m->gc.resize(5, nullptr); m->ga.resize(5, nullptr);
    ALLOC(m->ga[0], NB * m->flat, "ga0");
    for (int i = 0; i < 4; ++i) {
        const size_t sz = NB * asz(m->G[i]);
        snprintf(nm, sizeof nm, "gc%d", i + 1); ALLOC(m->gc[i + 1], sz, nm);
        snprintf(nm, sizeof nm, "ga%d", i + 1); ALLOC(m->ga[i + 1], sz, nm);
        if (sz > maxact) maxact = sz;
    }
    ALLOC(m->Ga, maxact, "Ga"); ALLOC(m->Gb, maxact, "Gb");
    ALLOC(m->xg, NB * HW, "xg"); ALLOC(m->dxbuf, NB * HW, "dx"); ALLOC(m->z, NB * zd, "z"); ALLOC(m->dzbuf, NB * zd, "dz");
    ALLOC(m->v_mu_raw, NB * zd, nullptr); ALLOC(m->v_ls_raw, NB * zd, nullptr); ALLOC(m->v_mu, NB * zd, "mu"); ALLOC(m->v_ls, NB * zd, "ls");
    ALLOC(m->v_sigma, NB * zd, "sigma"); ALLOC(m->v_kl, NB, nullptr); ALLOC(m->v_dmu, NB * zd, nullptr); ALLOC(m->v_dls, NB * zd, nullptr);
    ALLOC(m->z_wflip, 256, nullptr); ALLOC(m->z_dwflip, 256, nullptr);
    {
        size_t wp = 0, need = (size_t)4 << 20;
        auto wp_need = [&](UadConvDesc d, size_t n) { d.N = (int)n; size_t v = uad_conv_w_partial_floats(d); if (v > wp) wp = v; };
        auto want = [&](UadConvDesc d, size_t n) { d.N = (int)n; for (int f = 0; f < 2; ++f) { size_t v = uad_conv_ws_floats(d, f != 0, false); if (v > need) need = v; } };
        for (size_t i = 1; i < m->E.size(); ++i) { wp_need(m->E[i].d, NB); want(m->E[i].d, NB); }
        for (auto& L : m->G) { wp_need(L.d, NB); want(L.d, NB); }
        wp_need(dense_desc(1, m->flat, zd), NB); wp_need(dense_desc(1, zd, m->flat), NB);
        want(dense_desc(1, m->flat, zd), NB); want(dense_desc(1, zd, m->flat), NB);
        { UadConvDesc d0 = m->E[0].d; d0.N = (int)NB; size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        { UadConvDesc d0 = m->z_fd; d0.N = (int)NB; size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        ALLOC(m->wpartial, wp, nullptr);
        m->ws.floats = need; m->ws.ptr = nullptr; m->ws.counters = nullptr; m->ws.ncounters = 0;      // no in-kernel split-K reduction on this handle
        ALLOC(m->ws.ptr, need, nullptr);
    }
    size_t cs = kUadColsumScratchFloats;
    { const size_t v = uad_colsum_scratch_floats((int)NB, m->flat); if (v > cs) cs = v; }
    ALLOC(m->colscratch, cs, nullptr);
    ALLOC(m->redpart, 1024, nullptr); ALLOC(m->raw, 16, "raw"); ALLOC(m->scalars_own, 16, nullptr);
#undef ALLOC
    if (rc != UAD_OK) { uad_gan_destroy(m); return rc; }
    *out = m;
    return UAD_OK;
}


static int create_you(const uad_gan_config_t* cfg, uad_gan_t** out) {
    const int H = cfg->height, Z = cfg->zdim, W = cfg->dim_w, C = cfg->dim;
    if (H < 16 || H % 16) return fail(UAD_ERR_UNSUPPORTED, "GMVAE (You): height must be a power of two >= 16");
    if (cfg->inter_res != H / 4) return fail(UAD_ERR_INVALID, "GMVAE (You): the latent map is height / 4 (two stride-2 convolutions): set intermediateResolutions accordingly");
    // the first decoder convolution contracts over dim_z channels: 1 (image-side kernel) or a multiple of 8 (generic kernels' K step)
    if (!(Z == 1 || Z % 8 == 0) || Z > 64 || W < 1 || W > 64 || C < 1 || C > 64 || (long long)Z * C > 1024)
        return fail(UAD_ERR_UNSUPPORTED, "GMVAE (You): dim_z 1 or a multiple of 8 (<= 64), dim_w <= 64, dim_c <= 64, dim_z * dim_c <= 1024");
    uad_gan* m = gan_new(cfg, UAD_GAN_AAE, 2, false);
    m->aae_kind = 6; m->you = true; m->zim = m->zim_ce = m->gmv = false; m->a_constrained = m->a_critic = false;
    m->gm_W = W; m->gm_Z = Z; m->gm_C = C;
    m->dim = C; m->generic16 = false; m->adam_m2 = m->adam_v2 = nullptr; m->e_sw = m->e_sb = -1; m->a_zw = m->a_zb = -1;
    auto conv_op = [&](const std::string& name, int kind, int hin, int cin, int cout, int stride, bool relu) {
        YOp o;
        o.kind = kind; o.relu = relu; o.c = o.a = nullptr;
        const int hout = hin / stride;
        if (kind == 0) {
            o.L.d = UadConvDesc{1, hin, hin, cin, hout, hout, cout, 3, stride, stride == 2 ? 0 : 1};
            o.L.w = add_tensor(m, name + "/kernel", 4, 3, 3, cin, cout);
        } else {
            o.L.d = UadConvDesc{1, hout, hout, cout, hin, hin, cin, 3, 1, 1};
            o.L.w = add_tensor(m, name + "/kernel", 4, 3, 3, cout, cin);
        }
        o.L.b = add_tensor(m, name + "/bias", 1, cout, 1, 1, 1);
        o.L.gamma = o.L.beta = -1; o.L.H = o.L.W = hout; o.L.C = cout;
        o.Hout = hout; o.Cout = cout;
        return o;
    };
    static const char* en[6] = {"q_wz_x/3x3convlayer", "q_wz_x/3x3convlayer1", "q_wz_x/3x3convlayer2", "q_wz_x/3x3convlayer3", "q_wz_x/3x3convlayer4",
                                "q_wz_x/3x3convlayer5"};
    static const int es[6] = {2, 1, 1, 2, 1, 1};
    int h = H, cin = 1;
    for (int i = 0; i < 6; ++i) { m->y_enc.push_back(conv_op(en[i], 0, h, cin, 64, es[i], true)); h /= es[i]; cin = 64; }
    const int r = h, Q = Z * C;
    {
        int k = 0;
        const char* hn[4] = {"q_wz_x/w_mu", "q_wz_x/w_log_sigma", "q_wz_x/z_mu", "q_wz_x/z_log_sigma"};
        const int hd[4] = {W, W, Z, Z};
        for (int j = 0; j < 4; ++j) {
            m->y_off[k++] = add_tensor(m, std::string(hn[j]) + "/kernel", 4, 1, 1, 64, hd[j]);
            m->y_off[k++] = add_tensor(m, std::string(hn[j]) + "/bias", 1, hd[j], 1, 1, 1);
        }
        m->y_off[k++] = add_tensor(m, "p_z_wc/1x1convlayer/kernel", 4, 1, 1, W, 64); m->y_off[k++] = add_tensor(m, "p_z_wc/1x1convlayer/bias", 1, 64, 1, 1, 1);
        m->y_off[k++] = add_tensor(m, "p_z_wc/z_wc_mu/kernel", 4, 1, 1, 64, Q); m->y_off[k++] = add_tensor(m, "p_z_wc/z_wc_mu/bias", 1, Q, 1, 1, 1);
        m->y_off[k++] = add_tensor(m, "p_z_wc/z_wc_log_sigma/kernel", 4, 1, 1, 64, Q); m->y_off[k++] = add_tensor(m, "p_z_wc/z_wc_log_sigma/bias", 1, Q, 1, 1, 1);
        m->y_off[k++] = add_tensor(m, "Variable", 1, Q, 1, 1, 1);
        m->y_total = m->nparams - m->y_off[0];
    }
    auto up_op = [&](int hin, int c) { YOp o; o.kind = 2; o.relu = false; o.c = o.a = nullptr; o.Hout = 2 * hin; o.Cout = c; o.L.w = o.L.b = o.L.gamma = o.L.beta = -1; return o; };
    h = r;
    m->y_dec.push_back(conv_op("p_x_z/3x3convlayer1", 0, h, Z, 64, 1, true));
    m->y_dec.push_back(conv_op("p_x_z/3x3upconvlayer1", 1, h, 64, 64, 1, true));
    m->y_dec.push_back(conv_op("p_x_z/3x3upconvlayer2", 1, h, 64, 64, 1, true));
    m->y_dec.push_back(up_op(h, 64)); h *= 2;
    m->y_dec.push_back(conv_op("p_x_z/3x3convlayer2", 0, h, 64, 64, 1, true));
    m->y_dec.push_back(conv_op("p_x_z/3x3upconvlayer3", 1, h, 64, 64, 1, true));
    m->y_dec.push_back(conv_op("p_x_z/3x3upconvlayer4", 1, h, 64, 64, 1, true));
    m->y_dec.push_back(up_op(h, 64)); h *= 2;
    m->y_dec.push_back(conv_op("p_x_z/3x3convlayer3", 0, h, 64, 64, 1, false));
    m->y_dec.push_back(conv_op("p_x_z/y_mu", 0, h, 64, 1, 1, false));
    m->y_fd = UadConvDesc{1, H, H, 1, H, H, 64, 3, 1, 1};
    m->g_fw = m->y_dec.back().L.w; m->g_fb = m->y_dec.back().L.b;
    for (int k = 0; k < 3; ++k) { m->grp_off[k] = 0; m->grp_cnt[k] = m->nparams; }
    m->flat = r * r * Z; m->cenc = 64; m->cmid = 64;

    const size_t NB = (size_t)cfg->max_batch, HW = (size_t)H * H, Lm = NB * r * r;
    int rc = gan_alloc_flat(m);
    char nm[64];
#define ALLOC(ptr, n, name) if (rc == UAD_OK) rc = dev_alloc(m, &(ptr), (n), name)
    m->wpack_f = m->wpack_d = m->wpack16_f = m->wpack16_d = nullptr;
    size_t maxact = NB * HW * 64;
    for (size_t i = 0; i < m->y_enc.size(); ++i) {
        YOp& o = m->y_enc[i];
        snprintf(nm, sizeof nm, "yec%d", (int)i); ALLOC(o.c, NB * yop_out(o), nm);
        if (i + 1 < m->y_enc.size()) { ALLOC(o.a, NB * yop_out(o), nullptr); }
    }
    for (size_t i = 0; i + 1 < m->y_dec.size(); ++i) {
        YOp& o = m->y_dec[i];
        if (o.kind != 2) { snprintf(nm, sizeof nm, "ydc%d", (int)i); ALLOC(o.c, NB * yop_out(o), nm); }
        if (o.kind == 2 || o.relu) { ALLOC(o.a, NB * yop_out(o), nullptr); } else o.a = o.c;
    }
    ALLOC(m->Ga, maxact, "Ga"); ALLOC(m->Gb, maxact, "Gb");
    ALLOC(m->xg, NB * HW, "xg"); ALLOC(m->dxbuf, NB * HW, "dx"); ALLOC(m->gm_dxhat, NB * HW, nullptr);
    ALLOC(m->a_zm, Lm * Z, "z_s"); ALLOC(m->y_dzdec, Lm * Z, nullptr); ALLOC(m->y_h, Lm * 64, "h");
    ALLOC(m->y_ones, 64, nullptr); ALLOC(m->y_zeros, 64, nullptr);
    ALLOC(m->y_loc, Lm * 3, "loc"); ALLOC(m->y_colpart, Lm * 2 * 64, nullptr);
    ALLOC(m->y_dheads, Lm * (2 * W + 2 * Z), nullptr); ALLOC(m->y_da7, Lm * 64, nullptr); ALLOC(m->y_dM, Lm * Q, nullptr); ALLOC(m->y_dLq, Lm * Q, nullptr);
    ALLOC(m->y_ws, Lm * W, nullptr); ALLOC(m->y_mid, Lm * 64, nullptr);
    ALLOC(m->y_partial, (size_t)uad_gm_wgrad_chunks((int)Lm) * (size_t)m->y_total, nullptr);
    ALLOC(m->z_wflip, 1024, nullptr); ALLOC(m->z_dwflip, 1024, nullptr);
    if (rc == UAD_OK) {
        std::vector<float> ones(64, 1.0f);
        HIP_TRY(hipMemcpy(m->y_ones, ones.data(), 64 * sizeof(float), hipMemcpyHostToDevice));
    }
    {
        size_t wp = 0, need = (size_t)4 << 20;
        auto wp_need = [&](UadConvDesc d) { d.N = (int)NB; size_t v = uad_conv_w_partial_floats(d); if (v > wp) wp = v; };
        auto want = [&](UadConvDesc d) { d.N = (int)NB; for (int f = 0; f < 2; ++f) { size_t v = uad_conv_ws_floats(d, f != 0, false); if (v > need) need = v; } };
        auto first = [&](UadConvDesc d) { d.N = (int)NB; size_t v = uad_conv_first_wgrad_partial_floats(d); if (v > wp) wp = v; };
        for (auto& o : m->y_enc) { if (o.L.d.CB % 4) first(o.L.d); else { wp_need(o.L.d); want(o.L.d); } }
        for (size_t i = 0; i + 1 < m->y_dec.size(); ++i) {
            auto& o = m->y_dec[i];
            if (o.kind == 2) continue;
            if (o.L.d.CB % 4) first(o.L.d); else { wp_need(o.L.d); want(o.L.d); }
        }
        first(m->y_fd);
        ALLOC(m->wpartial, wp, nullptr);
        m->ws.floats = need; m->ws.ptr = nullptr; m->ws.counters = nullptr; m->ws.ncounters = 0;      // no in-kernel split-K reduction on this handle
        ALLOC(m->ws.ptr, need, nullptr);
    }
    ALLOC(m->colscratch, kUadColsumScratchFloats, nullptr);
    ALLOC(m->redpart, 1024, nullptr); ALLOC(m->raw, 16, "raw"); ALLOC(m->scalars_own, 16, nullptr);
#undef ALLOC
    if (rc != UAD_OK) { uad_gan_destroy(m); return rc; }
    *out = m;
    return UAD_OK;
}


static int create_chen(const uad_gan_config_t* cfg, uad_gan_t** out) {
    const int H = cfg->height, ir = cfg->inter_res, dim = cfg->dim > 0 ? cfg->dim : 64, zd = cfg->zdim;
    if (H != 8 * ir) return fail(UAD_ERR_UNSUPPORTED, "constrained AAE (Chen): three stride-2 blocks, height must be 8 * inter_res");
    if (dim % 32 || dim > 64) return fail(UAD_ERR_UNSUPPORTED, "constrained AAE (Chen): dim must be 32 or 64");
    if (ir < 2) return fail(UAD_ERR_UNSUPPORTED, "inter_res >= 2 needed");
    if (zd > kCritMaxZ) return fail(UAD_ERR_UNSUPPORTED, "zDim <= %d", kCritMaxZ);
    uad_gan* m = gan_new(cfg, UAD_GAN_AAE, 3, false);
    m->aae_kind = 7; m->chen = true; m->dim = dim; m->generic16 = false; m->e_sw = m->e_sb = -1;
    m->a_constrained = true; m->a_critic = true; m->a_h1 = 400; m->a_h2 = 200;
    char nm[160];
    int ln = 0;
    std::map<std::string, int> cnt;
    auto ln_name = [&](const char* scope) { std::string r = std::string(scope) + (ln == 0 ? "layer_normalization" : "layer_normalization_" + std::to_string(ln)); ++ln; return r; };
    auto tf_name = [&](const char* scope, const char* base) {
        const std::string key = std::string(scope) + base;
        const int k = cnt[key]++;
        return k == 0 ? key : key + "_" + std::to_string(k);
    };
    auto make_block = [&](bool gen, const char* scope, int Hin, int Cin, int Cout, int stride) {
        RB B;
        memset(&B, 0, sizeof B);
        B.gen = gen; B.stride = stride; B.Hin = Hin; B.Cin = Cin; B.Cout = Cout;
        B.Hout = gen ? Hin * stride : Hin / stride;
        std::string s1 = ln_name(scope);
        B.ln1g = add_tensor(m, s1 + "/gamma", 2, Hin, Hin, 1, 1); B.ln1b = add_tensor(m, s1 + "/beta", 2, Hin, Hin, 1, 1);
        std::string c1 = tf_name(scope, "conv2d");
        B.w1 = add_tensor(m, c1 + "/kernel", 4, 3, 3, Cin, Cout); B.b1 = add_tensor(m, c1 + "/bias", 1, Cout, 1, 1, 1);
        std::string s2 = ln_name(scope);
        B.ln2g = add_tensor(m, s2 + "/gamma", 2, Hin, Hin, 1, 1); B.ln2b = add_tensor(m, s2 + "/beta", 2, Hin, Hin, 1, 1);
        std::string c2 = tf_name(scope, gen ? "conv2d_transpose" : "conv2d");
        B.w2 = add_tensor(m, c2 + "/kernel", 4, 3, 3, Cout, Cout); B.b2 = add_tensor(m, c2 + "/bias", 1, Cout, 1, 1, 1);
        B.ws = B.bs = -1;
        if (stride == 2) {
            std::string sh = tf_name(scope, gen ? "conv2d_transpose" : "conv2d");
            if (gen) B.ws = add_tensor(m, sh + "/kernel", 4, 1, 1, Cout, Cin); else B.ws = add_tensor(m, sh + "/kernel", 4, 1, 1, Cin, Cout);
            B.bs = add_tensor(m, sh + "/bias", 1, Cout, 1, 1, 1);
        }
        B.d1 = UadConvDesc{1, Hin, Hin, Cin, Hin, Hin, Cout, 3, 1, 1};
        const int P2 = stride == 1 ? 1 : 0;
        if (gen) {
            B.d2 = UadConvDesc{1, B.Hout, B.Hout, Cout, Hin, Hin, Cout, 3, stride, P2};
            B.ds = UadConvDesc{1, B.Hout, B.Hout, Cout, Hin, Hin, Cin, 1, 2, 0};
        } else {
            B.d2 = UadConvDesc{1, Hin, Hin, Cout, B.Hout, B.Hout, Cout, 3, stride, P2};
            B.ds = UadConvDesc{1, Hin, Hin, Cin, Hin, Hin, Cout, 1, 1, 0};
        }
        B.sx = (size_t)Hin * Hin * Cin; B.sc1 = (size_t)Hin * Hin * Cout; B.sout = (size_t)B.Hout * B.Hout * Cout;
        return B;
    };
    // Encoder (:15-47, evaluate_encoder :128-151): conv2d, four blocks, dense
    {
        const std::string e0 = tf_name("Encoder/", "conv2d");
        m->s_d0w = add_tensor(m, e0 + "/kernel", 4, 3, 3, 1, dim); m->s_d0b = add_tensor(m, e0 + "/bias", 1, dim, 1, 1, 1);
        m->s_d0 = UadConvDesc{1, H, H, 1, H, H, dim, 3, 1, 1};
        const int chans[4] = {2 * dim, 4 * dim, 8 * dim, 8 * dim}, strides[4] = {2, 2, 2, 1};
        int c = dim, r = H;
        for (int k = 0; k < 4; ++k) { m->DB.push_back(make_block(false, "Encoder/", r, c, chans[k], strides[k])); c = chans[k]; r /= strides[k]; }
    }
    const int flatg = ir * ir * 8 * dim;
    m->flat = flatg; m->cenc = 8 * dim; m->cmid = 0;
    m->e_cw = m->e_cb = -1;
    m->e_dw = add_tensor(m, "Encoder/dense/kernel", 2, flatg, zd, 1, 1); m->e_db = add_tensor(m, "Encoder/dense/bias", 1, zd, 1, 1, 1);
    const long long enc_end = m->nparams;
    // Decoder (:49-83, evaluate_decoder :154-170)
    m->g_dw = add_tensor(m, "Decoder/dense/kernel", 2, zd, flatg, 1, 1); m->g_db = add_tensor(m, "Decoder/dense/bias", 1, flatg, 1, 1, 1);
    m->g_cw = m->g_cb = m->g_ln0g = m->g_ln0b = -1;
    {
        const int chans[4] = {8 * dim, 4 * dim, 2 * dim, dim}, strides[4] = {1, 2, 2, 2};
        int c = 8 * dim, r = ir;
        for (int k = 0; k < 4; ++k) { m->GB.push_back(make_block(true, "Decoder/", r, c, chans[k], strides[k])); c = chans[k]; r *= strides[k]; }
        const std::string sl = ln_name("Decoder/");
        m->s_glg = add_tensor(m, sl + "/gamma", 2, r, r, 1, 1); m->s_glb = add_tensor(m, sl + "/beta", 2, r, r, 1, 1);
        const std::string gf = tf_name("Decoder/", "conv2d");
        m->g_fw = add_tensor(m, gf + "/kernel", 4, 1, 1, c, 1); m->g_fb = add_tensor(m, gf + "/bias", 1, 1, 1, 1, 1);
    }
    const long long ae_end = m->nparams;
    m->a_w1 = add_tensor(m, "Discriminator/dense/kernel", 2, zd, m->a_h1, 1, 1); m->a_b1 = add_tensor(m, "Discriminator/dense/bias", 1, m->a_h1, 1, 1, 1);
    m->a_w2 = add_tensor(m, "Discriminator/dense_1/kernel", 2, m->a_h1, m->a_h2, 1, 1); m->a_b2 = add_tensor(m, "Discriminator/dense_1/bias", 1, m->a_h2, 1, 1, 1);
    m->a_w3 = add_tensor(m, "Discriminator/dense_2/kernel", 2, m->a_h2, 1, 1, 1); m->a_b3 = add_tensor(m, "Discriminator/dense_2/bias", 1, 1, 1, 1, 1);
    m->a_nd = m->nparams - ae_end;
    m->grp_off[0] = 0; m->grp_cnt[0] = enc_end;          // optim_gen: 'Encoder' in var.name
    m->grp_off[1] = 0; m->grp_cnt[1] = ae_end;           // optim_ae
    m->grp_off[2] = ae_end; m->grp_cnt[2] = m->nparams - ae_end;

    const size_t NB = (size_t)cfg->max_batch, E2 = 2 * NB, HW = (size_t)H * H;
    int rc = gan_alloc_flat(m);
#define ALLOC(ptr, n, name) if (rc == UAD_OK) rc = dev_alloc(m, &(ptr), (n), name)
    ALLOC(m->adam_m2, (size_t)m->nparams, nullptr); ALLOC(m->adam_v2, (size_t)m->nparams, nullptr);
    m->wpack_f = m->wpack_d = m->wpack16_f = m->wpack16_d = nullptr;
    size_t maxact = NB * HW * dim, max_ta = 0, max_tb = 0, max_sp = 0;
    auto alloc_block = [&](RB& B, float* X, float* DX, size_t cap, const char* tag, int k) {
        B.X = X; B.DX = DX;
        snprintf(nm, sizeof nm, "%s_h1_%d", tag, k); ALLOC(B.H1, cap * B.sx, nm);
        snprintf(nm, sizeof nm, "%s_c1_%d", tag, k); ALLOC(B.C1, cap * B.sc1, nm);
        snprintf(nm, sizeof nm, "%s_h2_%d", tag, k); ALLOC(B.H2, cap * B.sc1, nm);
        snprintf(nm, sizeof nm, "%s_out_%d", tag, k); ALLOC(B.OUT, cap * B.sout, nm);
        ALLOC(B.ST1, cap * 2 * B.Cin, nullptr); ALLOC(B.ST2, cap * 2 * B.Cout, nullptr);
        ALLOC(B.DOUT, cap * B.sout, nullptr); ALLOC(B.G1, cap * B.sc1, nullptr);
        if (!B.gen && B.ws >= 0) ALLOC(B.DSC, cap * B.sc1, nullptr);
        ALLOC(B.LP1, cap * (B.Cin / 32) * 2 * B.Hin * B.Hin, nullptr);
        ALLOC(B.LP2, cap * (B.Cout / 32) * 2 * B.Hin * B.Hin, nullptr);
        if (NB * B.sc1 > max_ta) max_ta = NB * B.sc1;
        if (NB * B.sx > max_tb) max_tb = NB * B.sx;
        if (NB * B.sout > max_sp) max_sp = NB * B.sout;
    };
    ALLOC(m->din, E2 * HW, "din");
    ALLOC(m->s_out0, E2 * HW * dim, "sd_out0"); ALLOC(m->s_dout0, E2 * HW * dim, nullptr);
    {
        float* X = m->s_out0; float* DX = m->s_dout0;
        for (size_t k = 0; k < m->DB.size(); ++k) { alloc_block(m->DB[k], X, DX, E2, "sd", (int)k); X = m->DB[k].OUT; DX = m->DB[k].DOUT; }
    }
    ALLOC(m->s_g0, NB * flatg, "sg_x0"); ALLOC(m->s_dg0, NB * flatg, nullptr);
    size_t lnp_g = 0;
    {
        float* X = m->s_g0; float* DX = m->s_dg0;
        for (size_t k = 0; k < m->GB.size(); ++k) { alloc_block(m->GB[k], X, DX, NB, "sg", (int)k); X = m->GB[k].OUT; DX = m->GB[k].DOUT; }
        const RB& L = m->GB.back();
        ALLOC(m->s_hf, NB * L.sout, "sg_hf"); ALLOC(m->s_stf, NB * 2 * L.Cout, nullptr);
        lnp_g = NB * (L.Cout / 32) * 2 * L.Hout * L.Hout;
        if (NB * L.sout > maxact) maxact = NB * L.sout;
    }
    ALLOC(m->lnpart_g, lnp_g, nullptr);
    ALLOC(m->s_ta, max_ta, nullptr); ALLOC(m->s_tb, max_tb, nullptr); ALLOC(m->s_sp, max_sp, nullptr); ALLOC(m->s_sct, max_ta, nullptr);
    ALLOC(m->Ga, maxact, "Ga"); ALLOC(m->Gb, maxact, "Gb");
    ALLOC(m->xg, NB * HW, "xg"); ALLOC(m->dxbuf, NB * HW, "dx"); ALLOC(m->Gx, NB * HW, "Gx"); ALLOC(m->a_xcat, E2 * HW, nullptr);
    ALLOC(m->a_zm, E2 * zd, "z"); ALLOC(m->a_dzm, E2 * zd, nullptr); ALLOC(m->dzbuf, NB * zd, "dz"); ALLOC(m->dzr, NB * zd, nullptr);
    ALLOC(m->a_slab, NB * (size_t)m->a_nd, nullptr); for (int k = 0; k < 3; ++k) ALLOC(m->a_crit[k], NB, nullptr);
    {
        size_t wp = 0, need = (size_t)4 << 20;
        auto wp_need = [&](UadConvDesc d, size_t n) { d.N = (int)n; size_t v = uad_conv_w_partial_floats(d); if (v > wp) wp = v; };
        auto want = [&](UadConvDesc d, size_t n) { d.N = (int)n; for (int f = 0; f < 2; ++f) { size_t v = uad_conv_ws_floats(d, f != 0, false); if (v > need) need = v; } };
        for (auto& B : m->GB) { wp_need(B.d1, NB); wp_need(B.d2, NB); want(B.d1, NB); want(B.d2, NB); if (B.ws >= 0) { wp_need(B.ds, NB); want(B.ds, NB); } }
        for (auto& B : m->DB) { wp_need(B.d1, E2); wp_need(B.d2, E2); want(B.d1, NB); want(B.d2, NB); if (B.ws >= 0) { wp_need(B.ds, E2); want(B.ds, NB); } }
        wp_need(dense_desc(1, flatg, zd), E2); wp_need(dense_desc(1, zd, flatg), NB);
        want(dense_desc(1, flatg, zd), NB); want(dense_desc(1, zd, flatg), NB);
        { UadConvDesc d0 = m->s_d0; d0.N = (int)E2; size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        ALLOC(m->wpartial, wp, nullptr);
        m->ws.floats = need; m->ws.ptr = nullptr; m->ws.counters = nullptr; m->ws.ncounters = 0;      // no in-kernel split-K reduction on this handle
        ALLOC(m->ws.ptr, need, nullptr);
    }
    ALLOC(m->colscratch, kUadColsumScratchFloats, nullptr); ALLOC(m->colpart, (size_t)kBnBwdBlocks * 2 * 128, nullptr);
    ALLOC(m->redpart, 1024, nullptr); ALLOC(m->raw, 16, "raw"); ALLOC(m->scalars_own, 16, nullptr);
    ALLOC(m->finpart, (size_t)1024 * 520, nullptr);
#undef ALLOC
    if (rc != UAD_OK) { uad_gan_destroy(m); return rc; }
    *out = m;
    return UAD_OK;
}

static int create_aae(const uad_gan_config_t* cfg, uad_gan_t** out) {
    const int H = cfg->height, ir = cfg->inter_res;
    if (cfg->aae_kind == 4 || cfg->aae_kind == 5) return create_zimmerer(cfg, out);
    if (cfg->aae_kind == 6) return create_you(cfg, out);
    if (cfg->aae_kind == 7) return create_chen(cfg, out);
    if (cfg->aae_kind < 0 || cfg->aae_kind > 7) return fail(UAD_ERR_INVALID, "bad aae_kind");
    const bool gmv = cfg->aae_kind == 3;
    if (gmv) {
        const long long q = (long long)cfg->zdim * cfg->dim;
        if (cfg->dim_w < 1 || cfg->dim_w > 1024 || cfg->zdim < 1 || cfg->zdim > 1024 || cfg->dim < 1 || cfg->dim > 64 || q > 4096)
            return fail(UAD_ERR_UNSUPPORTED, "dense GMVAE: 1 <= dim_w, dim_z <= 1024, 1 <= dim_c <= 64, dim_z * dim_c <= 4096");
    }
    const int npool = ilog2i(H) - ilog2i(ir);
    if (npool < 2 || npool > 5) return fail(UAD_ERR_UNSUPPORTED, "log2(height/inter_res) = %d: 2..5 blocks supported", npool);
    if (!gmv && cfg->zdim > kCritMaxZ) return fail(UAD_ERR_UNSUPPORTED, "zDim <= %d", kCritMaxZ);
    uad_gan* m = gan_new(cfg, UAD_GAN_AAE, npool, true);
    m->gmv = gmv; m->gm_W = cfg->dim_w; m->gm_Z = cfg->zdim; m->gm_C = cfg->dim; m->gm_J = 2 * cfg->dim_w + 2 * cfg->zdim;
    m->dim = 0; m->generic16 = false; m->adam_m2 = m->adam_v2 = nullptr; m->e_sw = m->e_sb = -1;
    m->aae_kind = cfg->aae_kind; m->a_constrained = cfg->aae_kind == 0 || cfg->aae_kind == 2; m->a_critic = cfg->aae_kind == 1 || cfg->aae_kind == 2;
    m->a_h1 = cfg->aae_kind == 2 ? 100 : 50; m->a_h2 = 50;
    char nm[160];
    int cin = 1, res = H;
    for (int i = 0; i < npool; ++i) {
        const int f = (32 << i) < 128 ? (32 << i) : 128;
        Block L;
        L.d = UadConvDesc{1, res, res, cin, res / 2, res / 2, f, 5, 2, 1};
        snprintf(nm, sizeof nm, "Encoder/enc_conv2D_%d/kernel", i); L.w = add_tensor(m, nm, 4, 5, 5, cin, f);
        snprintf(nm, sizeof nm, "Encoder/enc_conv2D_%d/bias", i); L.b = add_tensor(m, nm, 1, f, 1, 1, 1);
        std::string bs = i == 0 ? "Encoder/batch_normalization" : "Encoder/batch_normalization_" + std::to_string(i);
        L.gamma = add_tensor(m, bs + "/gamma", 1, f, 1, 1, 1);
        L.beta = add_tensor(m, bs + "/beta", 1, f, 1, 1, 1);
        L.H = L.W = res / 2; L.C = f;
        m->E.push_back(L);
        cin = f; res /= 2;
    }
    m->cenc = cin; m->cmid = cin / 8; m->flat = ir * ir * m->cmid;
    if (m->cmid % 8 || m->flat % 8) { delete m; return fail(UAD_ERR_UNSUPPORTED, "bottleneck channels must be a multiple of 8"); }
    const bool caae = cfg->aae_kind == 2;       // constrained_adversarial_autoencoder.py: conv2d / dense live in 'Encoder', dense (dec) / conv2d_1 in 'Decoder'
    const std::string n_conv = caae ? "Encoder/conv2d" : "Bottleneck/conv2d", n_z = caae ? "Encoder/dense" : "Bottleneck/dense";
    const std::string n_dec = caae ? "Decoder/dense" : "Bottleneck/dense_1", n_rev = caae ? "Decoder/conv2d_1" : "Bottleneck/conv2d_1";
    m->a_cw = add_tensor(m, n_conv + "/kernel", 4, 1, 1, m->cenc, m->cmid); m->a_cb = add_tensor(m, n_conv + "/bias", 1, m->cmid, 1, 1, 1);
    m->a_zw = m->a_zb = -1;
    if (gmv) {
        // layers take their scope name at first call (model :22-45): conv2d, dense .. dense_3 (w_mu, w_log_sigma, z_mu, z_log_sigma), dense_4 (dec_dense),
        // conv2d_1; then, outside any scope, dense / dense_1 (p(z|w,c)) and the 0.1 Variable (:48-53)
        const int hd[4] = {cfg->dim_w, cfg->dim_w, cfg->zdim, cfg->zdim};
        int ofs = 0;
        for (int h = 0; h < 4; ++h) {
            const std::string nmh = h == 0 ? "Bottleneck/dense" : "Bottleneck/dense_" + std::to_string(h);
            m->gm_hw[h] = add_tensor(m, nmh + "/kernel", 2, m->flat, hd[h], 1, 1); m->gm_hb[h] = add_tensor(m, nmh + "/bias", 1, hd[h], 1, 1, 1);
            m->gm_hd[h] = hd[h]; m->gm_ho[h] = ofs; ofs += hd[h];
        }
    } else {
        m->a_zw = add_tensor(m, n_z + "/kernel", 2, m->flat, cfg->zdim, 1, 1); m->a_zb = add_tensor(m, n_z + "/bias", 1, cfg->zdim, 1, 1, 1);
    }
    const long long gen_end_caae = m->nparams;        // 'Encoder' in name: blocks + conv2d + dense
    long long gen_end = caae ? gen_end_caae : m->a_cw;  // AAE: the encoder blocks only (the bottleneck lives in 'Bottleneck')
    const std::string n_dec2 = gmv ? "Bottleneck/dense_4" : n_dec;
    m->a_dw = add_tensor(m, n_dec2 + "/kernel", 2, cfg->zdim, m->flat, 1, 1); m->a_db = add_tensor(m, n_dec2 + "/bias", 1, m->flat, 1, 1, 1);
    m->a_rw = add_tensor(m, n_rev + "/kernel", 4, 1, 1, m->cmid, m->cenc); m->a_rb = add_tensor(m, n_rev + "/bias", 1, m->cenc, 1, 1, 1);
    if (gmv) {
        const int q = cfg->zdim * cfg->dim;
        m->gm_mw = add_tensor(m, "dense/kernel", 2, cfg->dim_w, q, 1, 1); m->gm_mb = add_tensor(m, "dense/bias", 1, q, 1, 1, 1);
        m->gm_lw = add_tensor(m, "dense_1/kernel", 2, cfg->dim_w, q, 1, 1); m->gm_lb = add_tensor(m, "dense_1/bias", 1, q, 1, 1, 1);
        m->gm_var = add_tensor(m, "Variable", 1, q, 1, 1, 1);
    }
    m->a_dbng = add_tensor(m, "Decoder/batch_normalization/gamma", 1, m->cenc, 1, 1, 1);
    m->a_dbnb = add_tensor(m, "Decoder/batch_normalization/beta", 1, m->cenc, 1, 1, 1);
    cin = m->cenc; res = ir;
    for (int i = 0; i < npool; ++i) {
        const int f = (128 >> i) > 32 ? (128 >> i) : 32;
        Block L;
        L.d = UadConvDesc{1, res * 2, res * 2, f, res, res, cin, 5, 2, 1};
        snprintf(nm, sizeof nm, "Decoder/dec_Conv2DT_%d/kernel", i); L.w = add_tensor(m, nm, 4, 5, 5, f, cin);
        snprintf(nm, sizeof nm, "Decoder/dec_Conv2DT_%d/bias", i); L.b = add_tensor(m, nm, 1, f, 1, 1, 1);
        res *= 2;
        const std::string bs = "Decoder/batch_normalization_" + std::to_string(i + 1);
        L.gamma = add_tensor(m, bs + "/gamma", 1, f, 1, 1, 1);
        L.beta = add_tensor(m, bs + "/beta", 1, f, 1, 1, 1);
        L.H = L.W = res; L.C = f;
        m->G.push_back(L);
        cin = f;
    }
    m->g_fw = add_tensor(m, "Decoder/dec_Conv2D_final/kernel", 4, 1, 1, cin, 1);
    m->g_fb = add_tensor(m, "Decoder/dec_Conv2D_final/bias", 1, 1, 1, 1, 1);
    const long long ae_end = m->nparams;
    m->a_w1 = m->a_b1 = m->a_w2 = m->a_b2 = m->a_w3 = m->a_b3 = -1; m->a_nd = 0;
    if (m->a_critic) {
        m->a_w1 = add_tensor(m, "Discriminator/dense/kernel", 2, cfg->zdim, m->a_h1, 1, 1); m->a_b1 = add_tensor(m, "Discriminator/dense/bias", 1, m->a_h1, 1, 1, 1);
        m->a_w2 = add_tensor(m, "Discriminator/dense_1/kernel", 2, m->a_h1, m->a_h2, 1, 1); m->a_b2 = add_tensor(m, "Discriminator/dense_1/bias", 1, m->a_h2, 1, 1, 1);
        m->a_w3 = add_tensor(m, "Discriminator/dense_2/kernel", 2, m->a_h2, 1, 1, 1); m->a_b3 = add_tensor(m, "Discriminator/dense_2/bias", 1, 1, 1, 1, 1);
        m->a_nd = m->nparams - ae_end;
    }
    // groups: 0 = optim_gen ('Encoder' variables, a prefix), 1 = optim_ae (every autoencoder variable), 2 = optim_dis
    m->grp_off[0] = 0; m->grp_cnt[0] = gen_end;
    m->grp_off[1] = 0; m->grp_cnt[1] = ae_end;
    m->grp_off[2] = ae_end; m->grp_cnt[2] = m->nparams - ae_end;

    const size_t NB = (size_t)cfg->max_batch, HW = (size_t)H * H, E2 = m->a_constrained ? 2 * NB : NB;
    int rc = gan_alloc_flat(m);
#define ALLOC(ptr, n, name) if (rc == UAD_OK) rc = dev_alloc(m, &(ptr), (n), name)
    ALLOC(m->adam_m2, (size_t)m->nparams, nullptr); ALLOC(m->adam_v2, (size_t)m->nparams, nullptr);
    size_t maxact = NB * HW;
    m->ec.resize(npool); m->ea.resize(npool + 1, nullptr); m->a_eg.resize(npool); m->a_cp.resize(npool);
    for (int i = 0; i < npool; ++i) {
        const size_t sz = E2 * asz(m->E[i]);
        snprintf(nm, sizeof nm, "ec%d", i); ALLOC(m->ec[i], sz, nm);
        snprintf(nm, sizeof nm, "ea%d", i + 1); ALLOC(m->ea[i + 1], sz, nm);
        ALLOC(m->a_eg[i], sz, nullptr);
        ALLOC(m->a_cp[i], (size_t)2 * kBnBwdBlocks * 2 * m->E[i].C, nullptr);
        if (NB * asz(m->E[i]) > maxact) maxact = NB * asz(m->E[i]);
    }
    ALLOC(m->et, E2 * m->flat, "et"); ALLOC(m->a_zm, E2 * cfg->zdim, "z"); ALLOC(m->a_dzm, E2 * cfg->zdim, nullptr);
    ALLOC(m->a_dflat, E2 * m->flat, nullptr); ALLOC(m->a_xcat, E2 * HW, nullptr);
    ALLOC(m->gdv, NB * m->flat, "gdv"); ALLOC(m->xg, NB * HW, "xg"); ALLOC(m->ddv, NB * m->flat, nullptr);
    m->gc.resize(npool + 1); m->ga.resize(npool + 1);
    for (int i = 0; i <= npool; ++i) {
        const size_t per = i == 0 ? (size_t)ir * ir * m->cenc : asz(m->G[i - 1]);
        snprintf(nm, sizeof nm, "gc%d", i); ALLOC(m->gc[i], NB * per, nm);
        snprintf(nm, sizeof nm, "ga%d", i); ALLOC(m->ga[i], NB * per, nm);
        if (NB * per > maxact) maxact = NB * per;
    }
    ALLOC(m->Ga, maxact, "Ga"); ALLOC(m->Gb, maxact, "Gb");
    ALLOC(m->dxbuf, NB * HW, "dx"); ALLOC(m->Gx, NB * HW, "Gx"); ALLOC(m->dzbuf, NB * cfg->zdim, "dz"); ALLOC(m->dzr, NB * cfg->zdim, nullptr);
    m->a_slab = nullptr; m->a_crit[0] = m->a_crit[1] = m->a_crit[2] = nullptr;
    if (m->a_critic) { ALLOC(m->a_slab, NB * (size_t)m->a_nd, nullptr); for (int k = 0; k < 3; ++k) ALLOC(m->a_crit[k], NB, nullptr); }
    m->gm_hv = m->gm_hvm = m->gm_ws = m->gm_M = m->gm_Lq = m->gm_pc = m->gm_loss3 = m->gm_dhv = m->gm_dM = m->gm_dLq = m->gm_dxhat = nullptr;
    if (gmv) {
        const size_t q = (size_t)cfg->zdim * cfg->dim;
        ALLOC(m->gm_hv, NB * m->gm_J, "hv"); ALLOC(m->gm_hvm, NB * m->gm_J, "hvm"); ALLOC(m->gm_ws, NB * cfg->dim_w, "w_s");
        ALLOC(m->gm_M, NB * q, "M"); ALLOC(m->gm_Lq, NB * q, "Lq"); ALLOC(m->gm_pc, NB * cfg->dim, "pc"); ALLOC(m->gm_loss3, 3 * NB, nullptr);
        ALLOC(m->gm_dhv, NB * m->gm_J, "dhv"); ALLOC(m->gm_dM, NB * q, nullptr); ALLOC(m->gm_dLq, NB * q, nullptr); ALLOC(m->gm_dxhat, NB * HW, nullptr);
    }
    {
        size_t wp = 0, need = (size_t)4 << 20;
        auto wp_need = [&](UadConvDesc d, size_t n) { d.N = (int)n; size_t v = uad_conv_w_partial_floats(d); if (v > wp) wp = v; };
        auto want = [&](UadConvDesc d, size_t n, bool pack) { d.N = (int)n; for (int f = 0; f < 2; ++f) { size_t v = uad_conv_ws_floats(d, f != 0, pack); if (v > need) need = v; } };
        for (size_t i = 1; i < m->E.size(); ++i) { wp_need(m->E[i].d, E2); want(m->E[i].d, NB, true); }
        for (auto& L : m->G) { wp_need(L.d, NB); want(L.d, NB, true); }
        wp_need(conv1x1_desc(1, ir, ir, m->cenc, m->cmid), E2); wp_need(conv1x1_desc(1, ir, ir, m->cmid, m->cenc), NB);
        want(conv1x1_desc(1, ir, ir, m->cenc, m->cmid), NB, false); want(conv1x1_desc(1, ir, ir, m->cmid, m->cenc), NB, false);
        if (!gmv) {
            wp_need(dense_desc(1, m->flat, cfg->zdim), E2); wp_need(dense_desc(1, cfg->zdim, m->flat), NB);
            want(dense_desc(1, m->flat, cfg->zdim), NB, false); want(dense_desc(1, cfg->zdim, m->flat), NB, false);
        }
        { UadConvDesc d0 = m->E[0].d; d0.N = (int)E2; size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        ALLOC(m->wpartial, wp, nullptr);
        m->ws.floats = need; m->ws.ptr = nullptr; m->ws.counters = nullptr; m->ws.ncounters = 0;      // no in-kernel split-K reduction on this handle
        ALLOC(m->ws.ptr, need, nullptr);
    }
    ALLOC(m->colscratch, kUadColsumScratchFloats, nullptr); ALLOC(m->colpart, (size_t)kBnBwdBlocks * 2 * 128, nullptr);
    ALLOC(m->redpart, 1024, nullptr); ALLOC(m->raw, 16, "raw"); ALLOC(m->scalars_own, 16, nullptr);
    ALLOC(m->finpart, (size_t)1024 * 65, nullptr);
#undef ALLOC
    if (rc != UAD_OK) { uad_gan_destroy(m); return rc; }
    *out = m;
    return UAD_OK;
}

int uad_gan_create(const uad_gan_config_t* cfg, uad_gan_t** out) {
    if (!cfg || !out) return fail(UAD_ERR_INVALID, "null argument");
    const int H = cfg->height;
    if (H != cfg->width || H <= 0 || (H & (H - 1))) return fail(UAD_ERR_INVALID, "height/width must be equal powers of two");
    if (cfg->inter_res <= 0 || (cfg->inter_res & (cfg->inter_res - 1)) || cfg->inter_res >= H)
        return fail(UAD_ERR_INVALID, "inter_res must be a power of two smaller than height");
    if (cfg->channels != 1) return fail(UAD_ERR_UNSUPPORTED, "numChannels=%d: only 1 is supported", cfg->channels);
    const bool dense_gmvae = cfg->variant == UAD_GAN_AAE && (cfg->aae_kind == 3 || cfg->aae_kind == 6);      // its latent widths are free (skinny-dense kernels)
    if (!dense_gmvae && (cfg->zdim <= 0 || cfg->zdim % 8)) return fail(UAD_ERR_UNSUPPORTED, "zDim must be a positive multiple of 8");
    if (cfg->max_batch <= 0) return fail(UAD_ERR_INVALID, "max_batch must be positive");
    if (cfg->variant != UAD_GAN_UNIFIED && cfg->variant != UAD_GAN_RESNET && cfg->variant != UAD_GAN_ANOVAEGAN && cfg->variant != UAD_GAN_AAE)
        return fail(UAD_ERR_INVALID, "bad variant");
    if (cfg->variant == UAD_GAN_AAE) return create_aae(cfg, out);
    if (cfg->variant == UAD_GAN_RESNET) return create_resnet(cfg, out);
    const int npool = ilog2i(H) - ilog2i(cfg->inter_res);
    if (npool < 2 || npool > 5) return fail(UAD_ERR_UNSUPPORTED, "log2(height/inter_res) = %d: 2..5 blocks supported", npool);
    if (H < 32) return fail(UAD_ERR_UNSUPPORTED, "height >= 32 needed");

    uad_gan* m = gan_new(cfg, cfg->variant, npool, true);
    m->dim = 0; m->generic16 = false;
    const bool av = cfg->variant == UAD_GAN_ANOVAEGAN;
    const int ir = cfg->inter_res;
    char nm[160];
    // ---- parameter table, TF variable-creation order (fanogan.py:15-58) ----
    int cin = 1, res = H;
    for (int i = 0; i < npool; ++i) {
        const int f = (32 << i) < 128 ? (32 << i) : 128;
        Block L;
        L.d = UadConvDesc{1, res, res, cin, res / 2, res / 2, f, 5, 2, 1};
        snprintf(nm, sizeof nm, "Encoder/enc_conv2D_%d/kernel", i); L.w = add_tensor(m, nm, 4, 5, 5, cin, f);
        snprintf(nm, sizeof nm, "Encoder/enc_conv2D_%d/bias", i); L.b = add_tensor(m, nm, 1, f, 1, 1, 1);
        std::string bs = i == 0 ? "Encoder/batch_normalization" : "Encoder/batch_normalization_" + std::to_string(i);
        L.gamma = add_tensor(m, bs + "/gamma", 1, f, 1, 1, 1);
        L.beta = add_tensor(m, bs + "/beta", 1, f, 1, 1, 1);
        L.H = L.W = res / 2; L.C = f;
        m->E.push_back(L);
        cin = f; res /= 2;
    }
    m->cenc = cin; m->cmid = cin / 8; m->flat = ir * ir * m->cmid;
    m->e_cw = add_tensor(m, "Encoder/conv2d/kernel", 4, 1, 1, m->cenc, m->cmid);
    m->e_cb = add_tensor(m, "Encoder/conv2d/bias", 1, m->cmid, 1, 1, 1);
    m->e_dw = add_tensor(m, "Encoder/dense/kernel", 2, m->flat, cfg->zdim, 1, 1);
    m->e_db = add_tensor(m, "Encoder/dense/bias", 1, cfg->zdim, 1, 1, 1);
    m->e_sw = m->e_sb = -1;
    if (av) {
        m->e_sw = add_tensor(m, "Encoder/dense_1/kernel", 2, m->flat, cfg->zdim, 1, 1);
        m->e_sb = add_tensor(m, "Encoder/dense_1/bias", 1, cfg->zdim, 1, 1, 1);
    }
    m->grp_off[UAD_GAN_ENCODER] = 0; m->grp_cnt[UAD_GAN_ENCODER] = m->nparams;
    m->g_dw = add_tensor(m, "Generator/dense/kernel", 2, cfg->zdim, m->flat, 1, 1);
    m->g_db = add_tensor(m, "Generator/dense/bias", 1, m->flat, 1, 1, 1);
    m->g_cw = add_tensor(m, "Generator/conv2d_1/kernel", 4, 1, 1, m->cmid, m->cenc);
    m->g_cb = add_tensor(m, "Generator/conv2d_1/bias", 1, m->cenc, 1, 1, 1);
    int ln = 0;
    auto ln_name = [&](const char* scope) { std::string r = std::string(scope) + (ln == 0 ? "layer_normalization" : "layer_normalization_" + std::to_string(ln)); ++ln; return r; };
    { const std::string s = ln_name("Generator/"); m->g_ln0g = add_tensor(m, s + "/gamma", 2, ir, ir, 1, 1); m->g_ln0b = add_tensor(m, s + "/beta", 2, ir, ir, 1, 1); }
    cin = m->cenc; res = ir;
    for (int i = 0; i < npool; ++i) {
        const int f = (128 >> i) > 32 ? (128 >> i) : 32;
        Block L;
        L.d = UadConvDesc{1, res * 2, res * 2, f, res, res, cin, 5, 2, 1};
        snprintf(nm, sizeof nm, "Generator/dec_Conv2DT_%d/kernel", i); L.w = add_tensor(m, nm, 4, 5, 5, f, cin);
        snprintf(nm, sizeof nm, "Generator/dec_Conv2DT_%d/bias", i); L.b = add_tensor(m, nm, 1, f, 1, 1, 1);
        res *= 2;
        const std::string s = ln_name("Generator/");
        L.gamma = add_tensor(m, s + "/gamma", 2, res, res, 1, 1);
        L.beta = add_tensor(m, s + "/beta", 2, res, res, 1, 1);
        L.H = L.W = res; L.C = f;
        m->G.push_back(L);
        cin = f;
    }
    m->g_fw = add_tensor(m, "Generator/dec_Conv2D_final/kernel", 4, 1, 1, cin, 1);
    m->g_fb = add_tensor(m, "Generator/dec_Conv2D_final/bias", 1, 1, 1, 1, 1);
    m->grp_off[UAD_GAN_GENERATOR] = m->grp_cnt[UAD_GAN_ENCODER];
    m->grp_cnt[UAD_GAN_GENERATOR] = m->nparams - m->grp_off[UAD_GAN_GENERATOR];
    cin = 1; res = H;
    for (int i = 0; i < npool; ++i) {
        const int f = (32 << i) < 128 ? (32 << i) : 128;
        Block L;
        L.d = UadConvDesc{1, res, res, cin, res / 2, res / 2, f, 5, 2, 1};
        snprintf(nm, sizeof nm, "Discriminator/enc_conv2D_%d/kernel", i); L.w = add_tensor(m, nm, 4, 5, 5, cin, f);
        snprintf(nm, sizeof nm, "Discriminator/enc_conv2D_%d/bias", i); L.b = add_tensor(m, nm, 1, f, 1, 1, 1);
        res /= 2;
        const std::string s = ln_name("Discriminator/");
        L.gamma = add_tensor(m, s + "/gamma", 2, res, res, 1, 1);
        L.beta = add_tensor(m, s + "/beta", 2, res, res, 1, 1);
        L.H = L.W = res; L.C = f;
        m->D.push_back(L);
        cin = f;
    }
    m->d_hw = add_tensor(m, "Discriminator/dense/kernel", 2, cin, 1, 1, 1);
    m->d_hb = add_tensor(m, "Discriminator/dense/bias", 1, 1, 1, 1, 1);
    m->grp_off[UAD_GAN_DISCRIMINATOR] = m->grp_off[UAD_GAN_GENERATOR] + m->grp_cnt[UAD_GAN_GENERATOR];
    m->grp_cnt[UAD_GAN_DISCRIMINATOR] = m->nparams - m->grp_off[UAD_GAN_DISCRIMINATOR];
    if (m->cmid % 8 || m->flat % 8) { delete m; return fail(UAD_ERR_UNSUPPORTED, "bottleneck channels must be a multiple of 8"); }

    // ---- device memory ----
    const size_t NB = (size_t)cfg->max_batch, HW = (size_t)H * H;
    int rc = gan_alloc_flat(m);
#define ALLOC(ptr, n, name) if (rc == UAD_OK) rc = dev_alloc(m, &(ptr), (n), name)
    size_t maxact = 3 * NB * HW;
    m->ec.resize(npool); m->ea.resize(npool + 1, nullptr);
    for (int i = 0; i < npool; ++i) {
        const size_t s = NB * asz(m->E[i]);
        snprintf(nm, sizeof nm, "ec%d", i); ALLOC(m->ec[i], s, nm);
        snprintf(nm, sizeof nm, "ea%d", i + 1); ALLOC(m->ea[i + 1], s, nm);
        if (s > maxact) maxact = s;
    }
    ALLOC(m->et, NB * m->flat, "et"); ALLOC(m->zr, NB * cfg->zdim, "zr"); ALLOC(m->z, NB * cfg->zdim, "z");
    ALLOC(m->gdv, NB * m->flat, "gdv"); ALLOC(m->xg, NB * HW, "xg");
    m->adam_m2 = m->adam_v2 = nullptr;
    if (av) {
        const size_t nz = NB * cfg->zdim;
        ALLOC(m->adam_m2, (size_t)m->nparams, nullptr); ALLOC(m->adam_v2, (size_t)m->nparams, nullptr);
        ALLOC(m->v_mu_raw, nz, nullptr); ALLOC(m->v_ls_raw, nz, nullptr); ALLOC(m->v_mu, nz, "v_mu"); ALLOC(m->v_ls, nz, nullptr);
        ALLOC(m->v_sigma, nz, "v_sigma"); ALLOC(m->v_kl, NB, nullptr); ALLOC(m->v_dmu, nz, nullptr); ALLOC(m->v_dls, nz, nullptr);
        ALLOC(m->v_dflat2, NB * m->flat, nullptr);
    }
    m->gc.resize(npool + 1); m->ga.resize(npool + 1); m->gstat.resize(npool + 1);
    size_t lnp_g = 0;
    for (int i = 0; i <= npool; ++i) {
        const size_t per = i == 0 ? (size_t)ir * ir * m->cenc : asz(m->G[i - 1]);
        const int C = i == 0 ? m->cenc : m->G[i - 1].C;
        snprintf(nm, sizeof nm, "gc%d", i); ALLOC(m->gc[i], NB * per, nm);
        snprintf(nm, sizeof nm, "ga%d", i); ALLOC(m->ga[i], NB * per, nm);
        ALLOC(m->gstat[i], NB * 2 * C, nullptr);
        if (NB * per > maxact) maxact = NB * per;
        const size_t lp = NB * (C / 32) * 2 * (per / C);
        if (lp > lnp_g) lnp_g = lp;
    }
    ALLOC(m->lnpart_g, lnp_g, nullptr);
    ALLOC(m->din, 4 * NB * HW, "din");
    m->Dc.resize(npool); m->Dstat.resize(npool); m->Da.resize(npool + 1, nullptr); m->Dg.resize(npool); m->V.resize(npool);
    m->inj.resize(npool); m->lnpart.resize(npool);
    size_t maxc = 0;
    for (int i = 0; i < npool; ++i) {
        const Block& L = m->D[i];
        const size_t per = asz(L);
        snprintf(nm, sizeof nm, "Dc%d", i); ALLOC(m->Dc[i], 3 * NB * per, nm);
        ALLOC(m->Dstat[i], 3 * NB * 2 * L.C, nullptr);
        snprintf(nm, sizeof nm, "Da%d", i + 1); ALLOC(m->Da[i + 1], 4 * NB * per, nm);
        snprintf(nm, sizeof nm, "Dg%d", i); ALLOC(m->Dg[i], 4 * NB * per, nm);
        snprintf(nm, sizeof nm, "V%d", i); ALLOC(m->V[i], NB * per, nm);
        snprintf(nm, sizeof nm, "inj%d", i); ALLOC(m->inj[i], NB * per, nm);
        ALLOC(m->lnpart[i], 4 * NB * (L.C / 32) * 2 * L.H * L.W, nullptr);
        if (3 * NB * per > maxact) maxact = 3 * NB * per;
        if (per > maxc) maxc = per;
    }
    ALLOC(m->Q, NB * maxc, "Q");
    ALLOC(m->Dd, 3 * NB * ir * ir, "Dd"); ALLOC(m->Gx, NB * HW, "Gx"); ALLOC(m->slopes, NB * H, "slopes");
    ALLOC(m->Ga, maxact, "Ga"); ALLOC(m->Gb, maxact, "Gb");
    ALLOC(m->dxbuf, NB * HW, "dx"); ALLOC(m->dzbuf, NB * cfg->zdim, "dz"); ALLOC(m->dzr, NB * cfg->zdim, nullptr);
    ALLOC(m->dflat, NB * m->flat, nullptr); ALLOC(m->ddv, NB * m->flat, nullptr);
    {
        size_t wp = 0;
        auto wp_need = [&](UadConvDesc d, size_t n) { d.N = (int)n; size_t v = uad_conv_w_partial_floats(d); if (v > wp) wp = v; };
        for (size_t i = 1; i < m->E.size(); ++i) wp_need(m->E[i].d, NB);
        for (auto& L : m->G) wp_need(L.d, NB);
        for (size_t i = 1; i < m->D.size(); ++i) wp_need(m->D[i].d, 4 * NB);
        wp_need(conv1x1_desc(1, ir, ir, m->cenc, m->cmid), NB); wp_need(conv1x1_desc(1, ir, ir, m->cmid, m->cenc), NB);
        wp_need(dense_desc(1, m->flat, cfg->zdim), NB); wp_need(dense_desc(1, cfg->zdim, m->flat), NB);
        { UadConvDesc d0 = m->D[0].d; d0.N = (int)(4 * NB); size_t v = uad_conv_first_wgrad_partial_floats(d0); if (v > wp) wp = v; }
        ALLOC(m->wpartial, wp, nullptr);
        size_t need = (size_t)4 << 20;
        auto want = [&](UadConvDesc d, size_t n, bool f, bool pack) { d.N = (int)n; size_t v = uad_conv_ws_floats(d, f, pack); if (v > need) need = v; };
        for (size_t i = 1; i < m->E.size(); ++i) { want(m->E[i].d, NB, true, true); want(m->E[i].d, NB, false, true); }
        for (auto& L : m->G) { want(L.d, NB, true, true); want(L.d, NB, false, true); }
        for (size_t i = 1; i < m->D.size(); ++i) { want(m->D[i].d, 3 * NB, true, true); want(m->D[i].d, 3 * NB, false, true); want(m->D[i].d, NB, true, true); want(m->D[i].d, NB, false, true); }
        for (int f = 0; f < 2; ++f) {
            want(conv1x1_desc(1, ir, ir, m->cenc, m->cmid), NB, f, false); want(conv1x1_desc(1, ir, ir, m->cmid, m->cenc), NB, f, false);
            want(dense_desc(1, m->flat, cfg->zdim), NB, f, false); want(dense_desc(1, cfg->zdim, m->flat), NB, f, false);
        }
        m->ws.floats = need; m->ws.ptr = nullptr; m->ws.counters = nullptr; m->ws.ncounters = 0;      // no in-kernel split-K reduction on this handle
        ALLOC(m->ws.ptr, need, nullptr);
    }
    ALLOC(m->colscratch, kUadColsumScratchFloats, nullptr); ALLOC(m->colpart, (size_t)kBnBwdBlocks * 2 * 128, nullptr);
    ALLOC(m->redpart, 1024, nullptr); ALLOC(m->raw, 16, "raw"); ALLOC(m->scalars_own, 16, nullptr);
    ALLOC(m->finpart, (size_t)1024 * 65, nullptr);
#undef ALLOC
    if (rc != UAD_OK) { uad_gan_destroy(m); return rc; }
    *out = m;
    return UAD_OK;
}

