"""Plain numpy statements of the train / restore step's small kernels (csrc/uad_loss.hip, uad_conv_first.hip, uad_optim.hip, uad_reduce.hip; tv_dxhat_kernel of csrc/uad_gmvae.hip) and the case tables of
tests/test_gpu_step_kernels.py.  tests/test_step_kernel_refs.py pins every statement here against oracle/nn.py and oracle/vae.py without a GPU.

Every ref_* function computes in the precision `dt` it is given (float64: the reference; float32: the same expressions in fp32 arithmetic, dot products
summed sequentially, from which the pointwise bounds of the GPU tests are measured -- pointwise_bound()).  Formulas: the kernels' own comments,
oracle/vae.py (Model.forward / losses / backward, CeVAE.ce_losses) and oracle/nn.py (bn_frozen_*, leaky_relu_*, *_tf_step).

Ties and kinks are BUILT INTO the inputs (nothing is filtered after the fact): pre-activations of every LeakyReLU site are moved at least KINK away from
zero, sign sites get operands that are either bit-equal (the zero-sign result is then required) or at least KINK apart."""
import numpy as np


def as_f32(v):
    """a scalar argument as the kernel receives it: rounded to fp32 (the fp64 reference takes the SAME number)"""
    return float(np.float32(v))


ALPHA = as_f32(0.3)                           # keras LeakyReLU default (oracle/vae.py: LRELU_ALPHA)
BN_MULT = float(np.float32(1.0) / np.sqrt(np.float32(1.0) + np.float32(1e-3)))      # frozen BN: 1 / sqrt(1 + eps), as the engines pass it
KINK = 1e-3                                   # least distance of a pre-activation / sign operand from its kink
SUM_TOL, LONG_SUM_TOL = 1e-4, 3e-4            # reduced quantities against fp64: the project's bars (tests/gpu_util.py REL_TOL; S1 / S2 in tests/test_gpu_ops.py)
POINTWISE_CAP = 1e-4


def _c(dt, *arrs):
    return [None if a is None else np.asarray(a, dtype=dt) for a in arrs]


def _seq_dot(a, w):
    """sum_c a[..., c] * w[c] added channel after channel in a's precision (the order-free worst case of an fp32 dot product)"""
    acc = a[..., 0] * w[0]
    for k in range(1, a.shape[-1]):
        acc = acc + a[..., k] * w[k]
    return acc


def away_from_kink(pre, kink=KINK):
    """pre-activations with every |value| < kink moved out to +-1.001 kink (zero goes to +)"""
    s = np.where(pre >= 0, 1.0, -1.0)
    return np.where(np.abs(pre) < kink, s * 1.001 * kink, pre)


# ------------------------------------------------------------------------------------------------ final 1x1 conv + L1 (final_kernel<false|true>)
def ref_final(c, scale, shift, mult, alpha, wf, bf, x, inv_batch, dxhat_in=None, zero_sign=None, backward=True, dt=np.float64):
    """c [N,H,W,C], x [N,H,W].  zero_sign: boolean [N,H,W] of pixels whose x was set to the caller's own x_hat bit for bit (s = 0 there).
    Returns a dict: x_hat, l1, rec [N], and with backward d_c, red [3C+1] = {dw, S1, S2, dbf}, s."""
    c, scale, shift, wf, x, dxhat_in = _c(dt, c, scale, shift, wf, x, dxhat_in)
    t = c.dtype.type
    sc = scale * t(mult)
    bn = c * sc + shift
    a = np.where(bn > 0, bn, bn * t(alpha))
    xh = _seq_dot(a, wf) + t(bf)
    diff = xh - x
    out = {'x_hat': xh, 'l1': np.abs(diff), 'rec': np.abs(diff).reshape(x.shape[0], -1).sum(axis=1), 'bn': bn}
    if not backward:
        return out
    if dxhat_in is not None:
        s = dxhat_in
    else:
        s = np.sign(diff) * t(inv_batch)
        if zero_sign is not None:
            s = np.where(zero_sign, t(0), s)
    da = s[..., None] * wf
    dbn = np.where(bn > 0, da, da * t(alpha))
    C = c.shape[-1]
    red = np.concatenate([(s[..., None] * a).reshape(-1, C).sum(0), dbn.reshape(-1, C).sum(0), (dbn * c).reshape(-1, C).sum(0), [s.sum()]])
    out.update(d_c=dbn * sc, red=red, s=s)
    return out


def final_blocks(H, W):
    """uad_final_blocks_per_sample restated (the GPU test holds it to uad_op_final_blocks)"""
    return max(1, (H * W) // 512)


def final_pass_pixels(C):
    """pixels one pass of a final_kernel workgroup covers: ppp * UNR = (256 / (C / 4)) * 4"""
    return (256 // (C // 4)) * 4


def final_last_block_pixels(H, W):
    hw, b = H * W, final_blocks(H, W)
    return hw - (b - 1) * -(-hw // b)


def short_last_block_shape(limit=64):
    """smallest image (in pixels, H >= 64) with more than one block per sample whose LAST block has fewer than `limit` pixels: shorter than one pass for
    every C the kernel takes up to 64 (final_pass_pixels(64) = 64).  With B = hw // 512 blocks of ceil(hw / B) pixels that needs B >= 450 or so."""
    hw = 512 * 2
    while True:
        if final_blocks(1, hw) > 1 and 0 < final_last_block_pixels(1, hw) < limit:
            for H in range(64, int(hw ** 0.5) + 1):
                if hw % H == 0:
                    return H, hw // H
        hw += 1


FINAL_C = (16, 32, 64)
FINAL_SHAPES = ((1, 8, 8), (3, 16, 16), (2, 20, 12), (2, 64, 64))
FINAL_MODES = ('fwd', 'sign', 'dxhat')


def final_inputs(N, H, W, C, seed):
    """c with no BN output within KINK of zero, BN / final-conv parameters, x_hat of the fp64 reference and an x at least KINK away from it everywhere"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.8, 1.2, C).astype(np.float32)
    shift = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    wf = (rng.standard_normal(C) / np.sqrt(C)).astype(np.float32)
    bf = np.float32(0.05)
    c = rng.standard_normal((N, H, W, C))
    sc = scale.astype(np.float64) * BN_MULT
    c = ((away_from_kink(c * sc + shift) - shift) / sc).astype(np.float32)
    bn = c.astype(np.float64) * sc + shift
    assert np.abs(bn).min() >= KINK, 'a LeakyReLU pre-activation is left within KINK of zero'
    xh = ref_final(c, scale, shift, BN_MULT, ALPHA, wf, bf, np.zeros((N, H, W)), 1.0, backward=False)['x_hat']
    x = (xh + rng.choice([-1.0, 1.0], xh.shape) * rng.uniform(2 * KINK, 0.5, xh.shape)).astype(np.float32)
    assert np.abs(x.astype(np.float64) - xh).min() >= KINK
    dxhat = (rng.standard_normal((N, H, W)) / N).astype(np.float32)
    return dict(c=c, scale=scale, shift=shift, wf=wf, bf=bf, x=x, dxhat=dxhat, inv_batch=as_f32(1.0 / N))


def tie_pixels(shape):
    """the fixed set of pixels whose two sign operands are made bit-equal: every 7th, the first and the last"""
    m = np.zeros(int(np.prod(shape)), bool)
    m[::7] = True
    m[0] = m[-1] = True
    return m.reshape(shape)


# ------------------------------------------------------------------------------------------------ reparameterisation + KL
def ref_reparam_fwd(mu_raw, ls_raw, n_vae, mask_mu=None, mask_ls=None, mask_mu_ce=None, eps=None, dt=np.float64):
    """[n, zdim] tensors; mask_mu_ce is [n - n_vae, zdim] (indexed from the first context sample).  Returns mu, ls, sigma, z, kl [n]."""
    mu_raw, ls_raw, mask_mu, mask_ls, mask_mu_ce, eps = _c(dt, mu_raw, ls_raw, mask_mu, mask_ls, mask_mu_ce, eps)
    t = mu_raw.dtype.type
    n = mu_raw.shape[0]
    m = mu_raw * mask_mu if mask_mu is not None else mu_raw.copy()
    l = ls_raw * mask_ls if mask_ls is not None else ls_raw.copy()
    s = np.exp(l)
    z = m + (eps * s if eps is not None else t(0) * s)
    kl = t(0.5) * (m * m + s * s - t(2) * l - t(1)).sum(axis=1)
    if n_vae < n:      # context branch: z = masked mu, no sampling, no KL
        mc = mu_raw[n_vae:] * mask_mu_ce if mask_mu_ce is not None else mu_raw[n_vae:]
        m[n_vae:], l[n_vae:], s[n_vae:], z[n_vae:], kl[n_vae:] = mc, 0, 1, mc, 0
    return m, l, s, z, kl


def ref_reparam_bwd(dz, mu, sigma, n_vae, inv_batch, eps=None, mask_mu=None, mask_ls=None, mask_mu_ce=None, dt=np.float64):
    dz, mu, sigma, eps, mask_mu, mask_ls, mask_mu_ce = _c(dt, dz, mu, sigma, eps, mask_mu, mask_ls, mask_mu_ce)
    t = dz.dtype.type
    n = dz.shape[0]
    dm = dz + mu * t(inv_batch)
    dl = (dz * eps * sigma if eps is not None else t(0) * dz) + (sigma * sigma - t(1)) * t(inv_batch)
    if mask_mu is not None:
        dm = dm * mask_mu
    if mask_ls is not None:
        dl = dl * mask_ls
    if n_vae < n:
        dm[n_vae:] = dz[n_vae:] * mask_mu_ce if mask_mu_ce is not None else dz[n_vae:]
        dl[n_vae:] = 0
    return dm, dl


REPARAM_ZDIM = (1, 16, 63, 64, 65, 128, 200)
REPARAM_N = (1, 3)


def reparam_inputs(n, zdim, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)      # noqa: E731
    keep = lambda: f((rng.random((n, zdim)) >= 0.2) / 0.8)      # noqa: E731
    return dict(mu_raw=f(rng.standard_normal((n, zdim))), ls_raw=f(0.5 * rng.standard_normal((n, zdim))), eps=f(rng.standard_normal((n, zdim))),
                mask_mu=keep(), mask_ls=keep(), mask_mu_ce=keep(), dz=f(rng.standard_normal((n, zdim)) / n))


# ------------------------------------------------------------------------------------------------ loss finalize
def ref_loss_finalize(rec_partial, n_vae, kl, inv_batch, rec_scale, dt=np.float64):
    """rec_partial [n, bps] -> (rec_per_sample [n], scalars [8]) -- trainers/ceVAE.py:45-50 via the kernel's comment"""
    rp, kl = _c(dt, rec_partial, kl)
    t = rp.dtype.type
    rec = rp.sum(axis=1)
    tr, tc = rec[:n_vae].sum(), rec[n_vae:].sum()
    tk = kl[:n_vae].sum() if kl is not None else t(0)
    ib = t(inv_batch)
    return rec, np.array([t(rec_scale) * (tr + tc) * ib, tk * ib, (tr + tk + tc) * ib, 0, tr * ib, tc * ib, (tr + tk) * ib, 0], dtype=dt)


LOSS_N = (1, 5, 255, 256, 257, 600)
LOSS_BPS = (1, 3, 16)


# ------------------------------------------------------------------------------------------------ first-layer data gradient
def ref_first_dgrad(g, W, HB, WB, S, P, dt=np.float64):
    """g [N,HS,WS,CS], W [KS,KS,1,CS] -> acc [N,HB,WB]: every small pixel (i, j) adds g . W[ky, kx] to big pixel (S i - P + ky, S j - P + kx)"""
    g, W = _c(dt, g, W)
    N, HS, WS, CS = g.shape
    KS = W.shape[0]
    pad = np.zeros((N, S * (HS - 1) + KS + HB, S * (WS - 1) + KS + WB), dtype=dt)      # big pixel y sits at row y + P
    for ky in range(KS):
        for kx in range(KS):
            pad[:, ky:ky + S * (HS - 1) + 1:S, kx:kx + S * (WS - 1) + 1:S] += _seq_dot(g, W[ky, kx, 0])
    return pad[:, P:P + HB, P:P + WB].copy()


def ref_dgrad_epilogue(acc, kind, x=None, x_hat=None, inv_batch=0.0, dxhat=None, x_upd=None, lr=0.0, dt=np.float64):
    """kind 'plain' -> {dx}; 'anomaly' -> {dx, anomaly}; 'restore' -> {dx, x_upd}"""
    acc, x, x_hat, dxhat, x_upd = _c(dt, acc, x, x_hat, dxhat, x_upd)
    t = acc.dtype.type
    if kind == 'plain':
        return {'dx': acc}
    if kind == 'anomaly':
        diff = x - x_hat
        gx = acc + np.sign(diff) * t(inv_batch)
        return {'dx': gx, 'anomaly': np.abs(diff) * np.abs(gx)}
    gx = acc - dxhat
    return {'dx': gx, 'x_upd': x_upd - t(lr) * gx}


# (N, HB, WB, CS): k5 s2 SAME (P = 1), one input channel.  The first two are shapes the tiled kernel takes, the others only the generic one
# (24 is no multiple of 16; CS = 64 and H = 10: the first-layer forward case of tests/test_gpu_ops.py)
DGRAD_SHAPES = ((2, 16, 16, 32), (1, 32, 48, 32), (2, 24, 24, 32), (1, 10, 10, 64))
DGRAD_TILED = (True, True, False, False)
DGRAD_EPILOGUES = ('plain', 'anomaly', 'restore')


def dgrad_inputs(N, HB, WB, CS, seed):
    rng = np.random.default_rng(seed)
    HS, WS = (HB + 1) // 2, (WB + 1) // 2
    g = (rng.standard_normal((N, HS, WS, CS)) / 8).astype(np.float32)
    W = (rng.standard_normal((5, 5, 1, CS)) / 5).astype(np.float32)
    x_hat = rng.uniform(0, 1, (N, HB, WB)).astype(np.float32)
    x = (x_hat + rng.choice([-1.0, 1.0], x_hat.shape) * rng.uniform(2 * KINK, 0.5, x_hat.shape)).astype(np.float32)
    ties = tie_pixels(x.shape)
    x[ties] = x_hat[ties]      # bit-equal operands: sign(0) = 0 is required there
    assert (np.abs(x.astype(np.float64) - x_hat)[~ties] >= KINK).all()
    return dict(g=g, W=W, x=x, x_hat=x_hat, ties=ties, dxhat=(rng.standard_normal((N, HB, WB)) / N).astype(np.float32),
                x_upd=rng.uniform(0, 1, (N, HB, WB)).astype(np.float32), inv_batch=as_f32(1.0 / N), lr=as_f32(1e-3),
                desc=(N, HB, WB, 1, HS, WS, CS, 5, 2, 1))


# ------------------------------------------------------------------------------------------------ TV term of the restoration objective
TV_SHAPES = ((1, 1, 1), (1, 1, 7), (2, 5, 3), (3, 16, 16), (1, 17, 31))
# both exactly representable with few bits: tv_lambda * (integer in -4 .. 4) is exact in fp32, so the kernel's result is ONE rounding of the exact value
# whether or not the compiler fuses the last multiply-add
TV_LAMBDA, TV_INV_BATCH = 1.8125, 0.375


def ref_tv_dxhat(x, xh, inv_batch, tv_lambda, dt=np.float64):
    """dxhat = -sign(r) inv_batch - tv_lambda dTV/dr, r = x - xh, TV = sum |r[i+1,j] - r[i,j]| + |r[i,j+1] - r[i,j]| per image; sign(0) = 0"""
    x, xh = _c(dt, x, xh)
    t = x.dtype.type
    r = x - xh
    tv = np.zeros_like(r)
    dv, dh = np.sign(r[:, 1:] - r[:, :-1]), np.sign(r[:, :, 1:] - r[:, :, :-1])
    tv[:, 1:] += dv
    tv[:, :-1] -= dv
    tv[:, :, 1:] += dh
    tv[:, :, :-1] -= dh
    return -np.sign(r) * t(inv_batch) - t(tv_lambda) * tv


def tv_objective(x, xh, inv_batch, tv_lambda):
    """inv_batch sum |xh - x| + tv_lambda TV(x - xh): ref_tv_dxhat is its gradient in xh (trainers/GMVAE_spatial.py:57-58, 90-92)"""
    r = x - xh
    return inv_batch * np.abs(r).sum() + tv_lambda * (np.abs(r[:, 1:] - r[:, :-1]).sum() + np.abs(r[:, :, 1:] - r[:, :, :-1]).sum())


def tv_inputs(N, H, W, seed):
    """multiples of 2^-10 in [0, 1] (every fp32 subtraction of the kernel is exact); a known share of equal neighbouring residuals and of r == 0"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1025, (N, H, W)) / 1024.0
    r = rng.integers(-3, 4, (N, H, W)) / 1024.0          # 7 levels: neighbours tie often, r == 0 for one pixel in seven
    xh = np.clip(x - r, 0.0, 1.0)
    return x.astype(np.float32), xh.astype(np.float32)


# ------------------------------------------------------------------------------------------------ SGD / Momentum / RMSProp
def ref_optim(kind, p, g, s1, s2, lr, momentum, decay, eps, gscale, dt=np.float64):
    """one step; returns (p, s1, s2) (slots a kind does not use come back unchanged) -- oracle/nn.py: sgd / momentum / rmsprop_tf_step on g * gscale"""
    p, g, s1, s2 = _c(dt, p, g, s1, s2)
    t = p.dtype.type
    gi = g * t(gscale)
    if kind == 1:
        return p - t(lr) * gi, s1, s2
    if kind == 2:
        a = t(momentum) * s1 + gi
        return p - t(lr) * a, a, s2
    ms = t(decay) * s2 + (t(1) - t(decay)) * gi * gi
    mom = t(momentum) * s1 + t(lr) * gi / np.sqrt(ms + t(eps))
    return p - mom, mom, ms


OPTIM_N = (1, 255, 256, 257, 100003)
OPTIM_HYPER = dict(lr=as_f32(0.01), momentum=as_f32(0.9), decay=as_f32(0.9), eps=as_f32(1e-10), gscale=0.5)


def optim_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return ((0.1 * rng.standard_normal(n)).astype(np.float32), [rng.standard_normal(n).astype(np.float32) for _ in range(3)])


# ------------------------------------------------------------------------------------------------ spatial latent
def ref_spatial_z_fwd(c, gamma, beta, rs0, alpha, mask=None, dt=np.float64):
    c, gamma, beta, mask = _c(dt, c, gamma, beta, mask)
    t = c.dtype.type
    y = c * (gamma * t(rs0)) + beta
    y = np.where(y > 0, y, t(alpha) * y)
    return y * mask if mask is not None else y


def ref_spatial_z_bwd(dz, c, gamma, beta, rs0, alpha, mask=None, dt=np.float64):
    """-> dc [rows, C], S1 [C] = sum d bn, S2 [C] = sum d bn * c"""
    dz, c, gamma, beta, mask = _c(dt, dz, c, gamma, beta, mask)
    t = c.dtype.type
    g = gamma * t(rs0)
    d = dz * mask if mask is not None else dz
    dn = np.where(c * g + beta > 0, d, t(alpha) * d)
    return dn * g, dn.sum(axis=0), (dn * c).sum(axis=0)


SPATIAL_ROWS = (1, 7, 511, 512, 513, 1300)
SPATIAL_C = (16, 64, 128)


def spatial_inputs(rows, C, seed):
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.8, 1.2, C).astype(np.float32)
    beta = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    g = gamma.astype(np.float64) * BN_MULT
    c = ((away_from_kink(rng.standard_normal((rows, C)) * g + beta) - beta) / g).astype(np.float32)
    assert np.abs(c.astype(np.float64) * g + beta).min() >= KINK, 'a LeakyReLU pre-activation is left within KINK of zero'
    return dict(c=c, gamma=gamma, beta=beta, dz=rng.standard_normal((rows, C)).astype(np.float32),
                mask=((rng.random((rows, C)) >= 0.2) / 0.8).astype(np.float32))


# ------------------------------------------------------------------------------------------------ column sums
COLSUM_ROWS = (1, 31, 1000, 5000)
COLSUM_C = (20, 32, 33, 128)


# ------------------------------------------------------------------------------------------------ pointwise bounds
def _rel(a32, a64):
    return float(np.abs(np.asarray(a32, np.float64) - a64).max() / max(np.abs(a64).max(), 1e-30))


def _measure_final():
    worst = {'x_hat': 0.0, 'd_c': 0.0}
    shapes = FINAL_SHAPES + ((1,) + short_last_block_shape(),)
    for C in FINAL_C:
        for k, (N, H, W) in enumerate(shapes):
            if k == len(FINAL_SHAPES) and C != FINAL_C[0]:
                continue      # (the large shape once: more pixels of the same distribution add nothing to a maximum over 10^5 of them)
            i = final_inputs(N, H, W, C, seed=1000 * C + k)
            a = [i['c'], i['scale'], i['shift'], BN_MULT, ALPHA, i['wf'], i['bf'], i['x'], i['inv_batch']]
            for dx in (None, i['dxhat']):
                r64, r32 = ref_final(*a, dxhat_in=dx), ref_final(*a, dxhat_in=dx, dt=np.float32)
                for key in worst:
                    worst[key] = max(worst[key], _rel(r32[key], r64[key]))
    return worst


def _measure_reparam():
    worst = dict.fromkeys(('mu', 'ls', 'sigma', 'z', 'dmu_raw', 'dls_raw'), 0.0)
    for zdim in REPARAM_ZDIM:
        for n in REPARAM_N:
            i = reparam_inputs(n, zdim, seed=100 * zdim + n)
            for n_vae in sorted({n, n - 1, 0}):
                kw = dict(mask_mu=i['mask_mu'], mask_ls=i['mask_ls'], mask_mu_ce=i['mask_mu_ce'][:n - n_vae], eps=i['eps'])
                f64, f32 = ref_reparam_fwd(i['mu_raw'], i['ls_raw'], n_vae, **kw), ref_reparam_fwd(i['mu_raw'], i['ls_raw'], n_vae, dt=np.float32, **kw)
                for key, a, b in zip(('mu', 'ls', 'sigma', 'z'), f32, f64):
                    worst[key] = max(worst[key], _rel(a, b))
                mu, sg = f64[0].astype(np.float32), f64[2].astype(np.float32)
                b64 = ref_reparam_bwd(i['dz'], mu, sg, n_vae, as_f32(1.0 / max(n_vae, 1)), **kw)
                b32 = ref_reparam_bwd(i['dz'], mu, sg, n_vae, as_f32(1.0 / max(n_vae, 1)), dt=np.float32, **kw)
                for key, a, b in zip(('dmu_raw', 'dls_raw'), b32, b64):
                    worst[key] = max(worst[key], _rel(a, b))
    return worst


def _measure_dgrad():
    worst = dict.fromkeys(('dx', 'anomaly', 'x_upd'), 0.0)
    for k, s in enumerate(DGRAD_SHAPES):
        i = dgrad_inputs(*s, seed=40 + k)
        a64, a32 = (ref_first_dgrad(i['g'], i['W'], s[1], s[2], 2, 1, dt=d) for d in (np.float64, np.float32))
        for kind in DGRAD_EPILOGUES:
            kw = dict(x=i['x'], x_hat=i['x_hat'], inv_batch=i['inv_batch'], dxhat=i['dxhat'], x_upd=i['x_upd'], lr=i['lr'])
            r64, r32 = ref_dgrad_epilogue(a64, kind, **kw), ref_dgrad_epilogue(a32, kind, dt=np.float32, **kw)
            for key in r64:
                worst[key] = max(worst[key], _rel(r32[key], r64[key]))
    return worst


def _measure_optim():
    worst = dict.fromkeys(('update', 's1', 's2'), 0.0)
    for kind in (1, 2, 3):
        for n in OPTIM_N:
            p, gs = optim_inputs(n, seed=10 * kind + n % 7)
            s1, s2 = np.zeros(n, np.float32), np.ones(n, np.float32)
            for g in gs:
                r64, r32 = ref_optim(kind, p, g, s1, s2, **OPTIM_HYPER), ref_optim(kind, p, g, s1, s2, dt=np.float32, **OPTIM_HYPER)
                worst['update'] = max(worst['update'], _rel(r32[0].astype(np.float64) - p, r64[0] - p))
                if kind >= 2:
                    worst['s1'] = max(worst['s1'], _rel(r32[1], r64[1]))
                if kind == 3:
                    worst['s2'] = max(worst['s2'], _rel(r32[2], r64[2]))
                p, s1, s2 = r32      # the chain continues from fp32 state, as on the device
    return worst


def _measure_spatial():
    worst = {'z': 0.0, 'dc': 0.0}
    for rows in SPATIAL_ROWS:
        for C in SPATIAL_C:
            i = spatial_inputs(rows, C, seed=rows + C)
            for mask in (None, i['mask']):
                a = (i['gamma'], i['beta'], BN_MULT, ALPHA, mask)
                worst['z'] = max(worst['z'], _rel(ref_spatial_z_fwd(i['c'], *a, dt=np.float32), ref_spatial_z_fwd(i['c'], *a)))
                worst['dc'] = max(worst['dc'], _rel(ref_spatial_z_bwd(i['dz'], i['c'], *a, dt=np.float32)[0], ref_spatial_z_bwd(i['dz'], i['c'], *a)[0]))
    return worst


_MEASURE = {'final': _measure_final, 'reparam': _measure_reparam, 'dgrad': _measure_dgrad, 'optim': _measure_optim, 'spatial': _measure_spatial}
_MEASURED = {}


def measured(family):
    """{output: largest relative max-norm error of the fp32 evaluation against fp64 over the family's own test inputs}"""
    if family not in _MEASURED:
        _MEASURED[family] = _MEASURE[family]()
    return _MEASURED[family]


def pointwise_bound(family, output):
    """four times the largest fp32-evaluation error seen, capped at POINTWISE_CAP"""
    return min(4.0 * measured(family)[output], POINTWISE_CAP)
