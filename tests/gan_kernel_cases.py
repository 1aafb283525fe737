"""Plain numpy statements of the small kernels of the materialised-graph engine (csrc/uad_gan_kernels.inc, every kernel but the LayerNorm ones) and the case
tables of tests/test_gpu_gan_kernels.py.  tests/test_gan_kernel_refs.py pins every statement here against oracle/ without a GPU.

Every ref_* function computes in the precision `dt` it is given: float64 is the reference; float32 is the same expression in fp32 arithmetic, from which the
pointwise bounds of the GPU tests are measured (pointwise_bound(), four times the largest fp32-against-fp64 error over this module's own inputs, capped at
1e-4).  The bit-exact statements (pooling, upsampling, combine, gathers, selections) are written in np.float32 with the kernel's association order.

Ties and kinks are BUILT INTO the inputs: sign / |a - b| sites get bit-equal operands at tie_mask() positions, LeakyReLU sites get pre-activations that are
exactly +0.0 and -0.0 at zero_mask() positions, the critic gets one hidden unit whose pre-activation is exactly zero.  Every other pre-activation is at
least 10 times farther from zero than its fp32 evaluation can move it (kink_margin(); asserted on the CPU for every case), so no device / reference
branch disagreement can occur.  Nothing from the package is imported here."""
import numpy as np

from oracle import nn as onn


def as_f32(v):
    """a scalar argument as the kernel receives it: rounded to fp32 (the fp64 reference takes the SAME number)"""
    return float(np.float32(v))


F = np.float32
ALPHA = as_f32(0.3)                           # keras LeakyReLU default (oracle: LRELU)
CRITIC_ALPHA = float(F(0.2))                  # tf.nn.leaky_relu default as critic_kernel holds it: the fp32 number 0.2f
BN_RS0 = float(F(1.0) / np.sqrt(F(1.0) + F(1e-3)))      # frozen BN: 1 / sqrt(1 + eps), as the engine passes it
KINK = 1e-3                                   # construction distance of a LeakyReLU pre-activation from zero
MARGIN = 10.0                                 # required: min |pre-activation| >= MARGIN * max |fp32-evaluated - fp64| pre-activation
SUM_TOL = 1e-4                                # reduced quantities against fp64: tests/gpu_util.py REL_TOL
POINTWISE_CAP = 1e-4
RULE_COEF, RULE_BN, RULE_GFINAL = 256, 512, 1024      # the engine's row-split rules (uad_gan.hip: kCoefColsumBlocks, kBnBwdBlocks, kGfinalBlocks)
SUM_BLOCKS = 256


def _c(dt, *arrs):
    return [None if a is None else np.asarray(a, dtype=dt) for a in arrs]


def away_from_kink(pre, kink=KINK):
    s = np.where(pre >= 0, 1.0, -1.0)
    return np.where(np.abs(pre) < kink, s * 1.001 * kink, pre)


def tie_mask(shape):
    """positions whose two operands are bit-equal: every 7th, the first and the last"""
    m = np.zeros(int(np.prod(shape)), bool)
    m[::7] = True
    m[0] = m[-1] = True
    return m.reshape(shape)


def row_split(rows, max_blocks):
    """uad_gan.hip row_split restated: (rows per workgroup, workgroups); the GPU test holds the count to uad_op_gan_rows_blocks"""
    rpb = -(-rows // max_blocks)
    return rpb, -(-rows // rpb)


def block_sums(v, rows, max_blocks):
    """v [rows, ...] -> [blocks, ...]: sums over each workgroup's consecutive rows"""
    rpb, blocks = row_split(rows, max_blocks)
    return np.stack([v[b * rpb:min(rows, (b + 1) * rpb)].sum(axis=0) for b in range(blocks)])


def kink_margin(pre64, pre32, exact_zero=None):
    """(smallest |pre-activation| outside the built-in zeros, largest |fp32 - fp64| pre-activation error)"""
    a = np.abs(np.asarray(pre64, np.float64))
    if exact_zero is not None:
        assert not np.asarray(pre64)[exact_zero].any() and not np.asarray(pre32)[exact_zero].any(), 'a built-in zero is not exactly zero'
        a = a[~exact_zero]
    return (float(a.min()) if a.size else np.inf), float(np.abs(np.asarray(pre32, np.float64) - pre64).max())


def margin_ok(pre64, pre32, exact_zero=None):
    lo, err = kink_margin(pre64, pre32, exact_zero)
    return lo >= MARGIN * err and lo > 0


# ------------------------------------------------------------------------------------------------ frozen-stats BN
def bn_pre(c, gamma, beta, rs0, dt=np.float64):
    c, gamma, beta = _c(dt, c, gamma, beta)
    return c * (gamma * c.dtype.type(rs0)) + beta


def ref_bn_act_fwd(c, gamma, beta, rs0, alpha, dt=np.float64):
    y = bn_pre(c, gamma, beta, rs0, dt)
    return np.where(y > 0, y, y.dtype.type(alpha) * y)


def ref_bn_act_bwd(da, c, gamma, beta, rs0, alpha, dt=np.float64):
    """-> dc [rows, C], dn [rows, C] (its column sums are S1, those of dn * c are S2)"""
    y = bn_pre(c, gamma, beta, rs0, dt)
    da, gamma = _c(dt, da, gamma)
    t = y.dtype.type
    dn = np.where(y > 0, da, t(alpha) * da)
    return dn * (gamma * t(rs0)), dn


QRL_C = (4, 32, 128, 256)                     # C / 4 divides 256; 4: 256 row lanes, most idle; 256: 4 row lanes, the one-thread-per-channel limit
QRL_C_WIDE = (512, 1024)                      # coef_colsum only (its partial write strides over C)
QRL_ROWS = (1, 7, 513, 1030)                  # 512 rule: 513 -> 2 rows per workgroup, the last has one; 1030 -> 3, the last has one
GFINAL_ROWS = QRL_ROWS + (1025,)              # 1024 rule: 2 rows per workgroup, the last has one
COEF_ROWS = QRL_ROWS + (257,)                 # 256 rule: 2 rows per workgroup, the last has one
FLAT_COUNTS = (1, 255, 256, 257, 1000)        # elements (float4s for the float4 kernels): both sides of one workgroup, and four workgroups


BN_FWD_CASES = tuple((t4 * 4 // C, C) for t4 in FLAT_COUNTS for C in (4, 32) if (t4 * 4) % C == 0)      # (rows, C): the flat counts as [t4, 4] and [t4 / 8, 32]


def zero_mask(shape):
    """where a LeakyReLU pre-activation is built to be exactly zero: channel 0 of every 3rd row (+0.0 and -0.0 alternate)"""
    m = np.zeros(shape, bool)
    m[::3, 0] = True
    return m


def bn_inputs(rows, C, seed):
    """c with every pre-activation at least KINK from zero, except zero_mask(): there c = +-0.0 and beta[0] = -0.0, so the pre-activation is +0.0 / -0.0 in
    every precision, fused or not ((+0) g + (-0) = +0, (-0) g + (-0) = -0)"""
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.8, 1.2, C).astype(F)
    beta = rng.uniform(-0.1, 0.1, C).astype(F)
    beta[0] = F(-0.0)
    g = gamma.astype(np.float64) * BN_RS0
    c = ((away_from_kink(rng.standard_normal((rows, C)) * g + beta) - beta) / g).astype(F)
    z = zero_mask((rows, C))
    c[z] = np.where(np.arange(int(z.sum())) % 2 == 0, F(0.0), F(-0.0))
    return dict(c=c, gamma=gamma, beta=beta, da=rng.standard_normal((rows, C)).astype(F), zeros=z)


# ------------------------------------------------------------------------------------------------ heads
def ref_rowdot(feat, w, b, act, dt=np.float64):
    feat, w, b = _c(dt, feat, w, b)
    s = feat @ w + b[0]
    return s if act == 0 else (1.0 / (1.0 + np.exp(-s)) if act == 1 else np.tanh(s))


ROWDOT_C = (4, 8, 64, 256, 512)               # 1 lane per row, 2 (a partial wave), 16, 64, 64 with a second strided pass
ROWDOT_ROWS = (1, 3, 5, 257)


def group_coef(rows, rpg, coef4, dt=np.float64):
    return np.asarray(coef4, dt)[np.arange(rows) // rpg]


def ref_topgrad(w, rows, rpg, coef4, dt=np.float64):
    return group_coef(rows, rpg, coef4, dt)[:, None] * np.asarray(w, dt)[None, :]


def ref_coef_colsum_terms(feat, rpg, coef4, dt=np.float64):
    feat = np.asarray(feat, dt)
    return feat * group_coef(feat.shape[0], rpg, coef4, dt)[:, None]


COEF4 = (as_f32(0.37), as_f32(-0.37), 0.0, 1.0)      # pass D's pattern: +k fake, -k real, 0 interpolates, 1 adjoint rows


def topgrad_rows(t4, C):
    assert (t4 * 4) % C == 0
    return t4 * 4 // C


TOPGRAD_CASES = tuple((t4, C) for (t4, C) in ((1, 4), (255, 4), (255, 20), (256, 4), (257, 4), (1000, 4), (1000, 20), (1280, 128)))
# rows_per_group = ceil(rows / 4): all four coefficients are used once rows >= 4; C = 4 puts 256 rows in a workgroup, so group boundaries (rows / 4) fall inside one


def ref_gfinal(dx, x, a, wf, act, dt=np.float64):
    """-> da [rows, C], dv [rows] (partials: sums of dv * a and of dv)"""
    dx, x, wf = _c(dt, dx, x, wf)
    t = dx.dtype.type
    dv = dx * (x * (t(1) - x) if act == 0 else ((t(1) - x * x) if act == 1 else t(1)))
    return dv[:, None] * wf[None, :], dv


def gfinal_inputs(rows, C, seed):
    rng = np.random.default_rng(seed)
    return dict(dx=rng.standard_normal(rows).astype(F), x=rng.uniform(0.05, 0.95, rows).astype(F), a=rng.standard_normal((rows, C)).astype(F),
                wf=(rng.standard_normal(C) / np.sqrt(C)).astype(F))


# ------------------------------------------------------------------------------------------------ elementwise
def ref_interp(xg, x, alpha, dt=np.float64):
    xg, x, alpha = _c(dt, xg, x, alpha)
    return np.stack([xg, x, x + alpha[:, None] * (xg - x)])


INTERP_CASES = tuple((n, hw) for n in (1, 3) for hw in (1, 7, 256)) + ((1, 255), (1, 257), (3, 300))


def ref_flat(kind, a, b, c, coef, out0, dt=np.float64):
    """the nine uad_op_gan_flat kinds (include/uad_hip.h: UAD_GAN_FLAT_*); out0 = the output's previous content for the in-place kinds"""
    a, b, c, out0 = _c(dt, a, b, c, out0)
    t = (a if a is not None else b).dtype.type
    if kind == 0:
        return np.tanh(a)
    if kind == 1:
        return a * (t(1) - b * b) * (c if c is not None else t(1))
    if kind == 2:
        return t(coef) * (a - b)
    if kind == 3:
        return out0 + t(coef) * (a - b)
    if kind == 4:
        return t(coef) * np.sign(a - b)
    if kind == 5:
        return out0 + a
    if kind == 6:
        return out0 + b[0]
    if kind == 7:
        return np.where(a > 0, a, t(coef) * a)
    return np.where(b > 0, a, t(coef) * a)


FLAT_KINDS = {'tanh': 0, 'tanh_bwd': 1, 'tanh_bwd_mask': 1, 'diff_scale': 2, 'diff_scale_acc': 3, 'sign_scale': 4, 'add': 5, 'add_scalar': 6, 'lrelu_fwd': 7,
              'lrelu_bwd': 8}
FLAT_COEF = as_f32(0.2)                       # lrelu: tf.nn.leaky_relu default; the scale kernels: any fp32 number


def flat_inputs(name, n, seed):
    """n floats per operand.  sign_scale: a == b bit for bit at tie_mask(); lrelu: the pre-activation is +0.0 / -0.0 at every 5th / every 5th + 1 element"""
    rng = np.random.default_rng(seed)
    f = lambda: rng.standard_normal(n).astype(F)      # noqa: E731
    a, b, out0 = f(), f(), f()
    c = ((rng.random(n) >= 0.2) / 0.8).astype(F) if name == 'tanh_bwd_mask' else None
    if name.startswith('tanh_bwd'):
        b = np.tanh(b)
    if name == 'sign_scale':
        b[tie_mask(n)] = a[tie_mask(n)]
    pre = a if name == 'lrelu_fwd' else b
    if name.startswith('lrelu'):
        pre[::5] = F(0.0)
        pre[1::5] = F(-0.0)
    return dict(a=a, b=b, c=c, out0=out0)


def ref_sum_terms(mode, a, b, dt=np.float64):
    a, b = _c(dt, a, b)
    return a if mode == 0 else ((a - b) ** 2 if mode == 1 else np.abs(a - b))


def sum_partials(terms):
    """the fixed 256 x 256 grid, grid-stride: element i belongs to workgroup (i // 256) % 256"""
    n = terms.size
    pad = np.zeros(-(-n // 65536) * 65536, terms.dtype)
    pad[:n] = terms
    return pad.reshape(-1, SUM_BLOCKS, 256).sum(axis=(0, 2))


SUM_N = (1, 65535, 65536, 65537, 200000)      # idle workgroups, the exact grid, a one-element second pass, a ragged second pass


def sum_inputs(n, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 1.5, n).astype(F), rng.uniform(-1.0, 1.0, n).astype(F)
    ties = tie_mask(n)
    b[ties] = a[ties]
    return a, b, ties


# ------------------------------------------------------------------------------------------------ slope penalty (trainers/fAnoGAN.py:56-57)
def ref_pen_col(g, dt=np.float64):
    """g [n, H, W] -> slopes [n, W], (slope - 1)^2 [n, W]"""
    g = np.asarray(g, dt)
    s = np.sqrt((g * g).sum(axis=1))
    return s, (s - g.dtype.type(1)) ** 2


def ref_pen_grad(g, s, coef, dt=np.float64):
    g, s = _c(dt, g, s)
    t = g.dtype.type
    return (t(coef) * (s - t(1)) / s)[:, None, :] * g


PEN_SHAPES = ((1, 1, 1), (2, 5, 3), (3, 16, 100), (1, 8, 257))
PEN_GRAD_SHAPES = ((1, 1, 1), (1, 5, 51), (1, 16, 16), (1, 1, 257), (2, 5, 100))      # 1, 255, 256, 257, 1000 elements
PEN_COEF = as_f32(10.0 * 2.0 / 300.0)
MIN_SLOPE = 0.05


def pen_inputs(n, H, W, seed):
    """|g| >= MIN_SLOPE everywhere (so every slope is); with H > 1, column 1 of sample 0 is a unit vector: slope exactly 1 in every precision"""
    rng = np.random.default_rng(seed)
    g = (rng.choice([-1.0, 1.0], (n, H, W)) * rng.uniform(MIN_SLOPE, 1.5, (n, H, W))).astype(F)
    if H > 1 and W > 1:
        g[0, :, 1] = 0
        g[0, H // 2, 1] = -1
    return g


# ------------------------------------------------------------------------------------------------ pooling, upsampling, tap flip: bit-exact fp32
def ref_avgpool_fwd(x):
    x = np.asarray(x, F)
    return ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * F(0.25)


def ref_avgpool_bwd(g):
    return np.repeat(np.repeat(np.asarray(g, F) * F(0.25), 2, axis=1), 2, axis=2)


def ref_up2_fwd(x):
    return np.repeat(np.repeat(np.asarray(x, F), 2, axis=1), 2, axis=2)


def ref_up2_bwd(g):
    g = np.asarray(g, F)
    return (g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + (g[:, 1::2, 0::2] + g[:, 1::2, 1::2])


POOL_H, POOL_C, POOL_N = (2, 4, 6), (4, 8, 36), (1, 3)
FLIP_T, FLIP_C = (1, 9, 25), (1, 3, 64)


def ref_flip_taps(w):
    return np.asarray(w, F)[::-1].copy()


# ------------------------------------------------------------------------------------------------ combine (bit-exact fp32, the kernel's association)
S = dict(GEN_LOSS=0, DISC_FAKE=1, DISC_REAL=2, PENALTY=3, DISC_LOSS=4, LOSS_IMG=5, LOSS_FTS=6, ENC_LOSS=7, REC_LOSS=8, KL=9, GM_LOSS=10, GM_CON=11, GM_W=12,
         GM_C=13)      # include/uad_hip.h: UAD_GAN_S_*
COMBINE_PHASES = (0, 1, 2, 3, 4, 5, 6, 7)      # 0: the f-AnoGAN encoder phase (the kernel's last branch)
# four distinct values with at most 9 significant bits and a 3-bit kappa: every product kappa * raw[k] is exact in fp32, so each sum is ONE rounding of the
# exact value whether or not the compiler fuses the multiply-add -- the fp32 statement below has one bit pattern
COMBINE_RAW = tuple(F(v) for v in (187 / 256, -362 / 256, 81 / 256, 87 / 32))
COMBINE_KAPPA = 0.625


def ref_combine(phase, raw, kappa):
    """{scalar index: fp32 value} -- exactly the slots the branch writes"""
    r = [F(v) for v in raw]
    k = F(kappa)
    if phase == 1:
        return {S['DISC_FAKE']: r[0], S['GEN_LOSS']: -r[0]}
    if phase == 2:
        return {S['DISC_FAKE']: r[0], S['DISC_REAL']: r[1], S['PENALTY']: r[2], S['DISC_LOSS']: F(F(r[0] - r[1]) + r[2]), S['GEN_LOSS']: -r[0]}
    if phase == 7:
        return {S['REC_LOSS']: r[0], S['GM_CON']: F(r[1] * k), S['GM_W']: F(r[2] * k), S['GM_C']: F(r[3] * k),
                S['GM_LOSS']: F(F(F(r[0] + F(r[1] * k)) + F(r[2] * k)) + F(r[3] * k))}
    if phase == 6:
        return {S['LOSS_IMG']: r[0], S['LOSS_FTS']: r[1], S['KL']: r[2], S['REC_LOSS']: F(F(0.5) * F(r[0] + r[1])), S['ENC_LOSS']: F(F(r[0] + r[2]) + r[1]),
                S['GM_LOSS']: F(r[0] + r[2])}
    if phase == 5:
        return {S['REC_LOSS']: r[0], S['GM_CON']: r[1], S['GM_W']: r[2], S['GM_C']: r[3], S['GM_LOSS']: F(F(F(r[0] + r[1]) + r[2]) + r[3])}
    if phase == 3:
        return {S['REC_LOSS']: r[0], S['KL']: r[1], S['ENC_LOSS']: F(r[0] + F(k * r[1]))}
    return {S['LOSS_IMG']: r[0], S['LOSS_FTS']: r[1], S['ENC_LOSS']: F(r[0] + F(k * r[1])), S['REC_LOSS']: r[2]}      # 4 (AAE) and 0 (encoder)


# ------------------------------------------------------------------------------------------------ latent critic
CRITIC_ZD = (1, 127, 128, 129, 512)
CRITIC_H = ((1, 1), (127, 129), (400, 400))
CRITIC_N = (1, 3)
CRITIC_SCALE = 10.0


def critic_size(zd, h1, h2):
    return zd * h1 + h1 + h1 * h2 + h2 + h2 + 1


def critic_segments(zd, h1, h2):
    """[(name, slice)] of a sample's slab: dW1 | db1 | dW2 | db2 | dW3 | db3"""
    out, o = [], 0
    for name, k in (('dW1', zd * h1), ('db1', h1), ('dW2', h1 * h2), ('db2', h2), ('dW3', h2), ('db3', 1)):
        out.append((name, slice(o, o + k)))
        o += k
    return out


def _lrelu(a, alpha):
    return onn.leaky_relu_fwd(a, alpha)


def critic_fwd(P, v, dt=np.float64, alpha=CRITIC_ALPHA):
    W1, b1, W2, b2, W3, b3, v = _c(dt, P['W1'], P['b1'], P['W2'], P['b2'], P['W3'], P['b3'], v)
    al = v.dtype.type(alpha)
    a1 = v @ W1 + b1
    h1 = _lrelu(a1, al)
    a2 = h1 @ W2 + b2
    h2 = _lrelu(a2, al)
    return dict(d=h2 @ W3 + b3[0], a1=a1, a2=a2, h1=h1, h2=h2, m1=np.where(a1 > 0, v.dtype.type(1), al), m2=np.where(a2 > 0, v.dtype.type(1), al), v=v)


def z_hat(zf, zr, eps, hat_mode, dt=np.float64):
    zf, zr, eps = _c(dt, zf, zr, eps)
    return (zf if hat_mode else zr) + eps[:, None] * (zr - zf)


def ref_critic(P, zf, zr, eps, inv_n, scale, mode, hat_mode, dt=np.float64, alpha=CRITIC_ALPHA):
    """mode 0 -> d_fake, d_real, pen [n], slab [n, nD], slopes [n]; mode 1 -> d_fake, dz_fake [n, zd]"""
    W1, W2, W3 = _c(dt, P['W1'], P['W2'], P['W3'])
    t = W1.dtype.type
    f = critic_fwd(P, zf, dt, alpha)

    def input_grad(c):
        u2 = c['m2'] * W3
        u1 = c['m1'] * (u2 @ W2.T)
        return u2, u1, u1 @ W1.T
    if mode == 1:
        return dict(d_fake=f['d'], dz_fake=-t(inv_n) * input_grad(f)[2])
    r, h = critic_fwd(P, zr, dt, alpha), critic_fwd(P, z_hat(zf, zr, eps, hat_mode, dt), dt, alpha)
    u2, u1, gz = input_grad(h)
    s = np.sqrt((gz * gz).sum(axis=1))
    pen = t(scale) * t(inv_n) * (s - t(1)) ** 2
    coef = t(scale) * t(2) * (s - t(1)) / s * t(inv_n)
    da2 = [t(inv_n) * W3 * f['m2'], -t(inv_n) * W3 * r['m2']]
    da1 = [(da2[0] @ W2.T) * f['m1'], (da2[1] @ W2.T) * r['m1']]
    gbar = coef[:, None] * gz
    tb1 = (gbar @ W1) * h['m1']
    ub2 = tb1 @ W2
    n = f['v'].shape[0]
    dW1 = f['v'][:, :, None] * da1[0][:, None, :] + r['v'][:, :, None] * da1[1][:, None, :] + gbar[:, :, None] * u1[:, None, :]
    dW2 = f['h1'][:, :, None] * da2[0][:, None, :] + r['h1'][:, :, None] * da2[1][:, None, :] + tb1[:, :, None] * u2[:, None, :]
    dW3 = t(inv_n) * (f['h2'] - r['h2']) + ub2 * h['m2']
    slab = np.concatenate([dW1.reshape(n, -1), da1[0] + da1[1], dW2.reshape(n, -1), da2[0] + da2[1], dW3, np.zeros((n, 1), dt)], axis=1)
    return dict(d_fake=f['d'], d_real=r['d'], pen=pen, slab=slab, slopes=s, pre=(f, r, h))


def critic_zero_unit(h1, h2):
    """(layer, unit) whose pre-activation is built to be exactly zero (zero weight column, zero bias), or None for the 1 x 1 critic, whose only path it would
    cut (slope 0: (s - 1) / s undefined)"""
    return (1, 0) if h1 > 1 else ((2, 0) if h2 > 1 else None)


def critic_inputs(zd, h1, h2, n, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(F)      # noqa: E731
    P = dict(W1=f(rng.standard_normal((zd, h1)) / np.sqrt(zd)), b1=f(0.1 * rng.standard_normal(h1)), W2=f(rng.standard_normal((h1, h2)) / np.sqrt(h1)),
             b2=f(0.1 * rng.standard_normal(h2)), W3=f(rng.standard_normal(h2) / np.sqrt(h2)), b3=f(0.1 * rng.standard_normal(1)))
    zu = critic_zero_unit(h1, h2)
    if zu is not None:
        P['W%d' % zu[0]][:, zu[1]] = 0
        P['b%d' % zu[0]][zu[1]] = 0
    return dict(P=P, zf=f(rng.standard_normal((n, zd))), zr=f(rng.standard_normal((n, zd))), eps=f(rng.uniform(0.05, 0.95, n)))


def critic_margins(i, hat_mode, zu):
    """[(min |pre|, max fp32 error)] over the six pre-activation tensors of a critic-step case, the built-in zero unit left out"""
    r64, r32 = (ref_critic(i['P'], i['zf'], i['zr'], i['eps'], 1.0, CRITIC_SCALE, 0, hat_mode, dt=d) for d in (np.float64, np.float32))
    out = []
    for c64, c32 in zip(r64['pre'], r32['pre']):
        for layer, key in ((1, 'a1'), (2, 'a2')):
            z = np.zeros(c64[key].shape, bool)
            if zu is not None and zu[0] == layer:
                z[:, zu[1]] = True
            out.append(kink_margin(c64[key], c32[key], z))
    return out, float(r64['slopes'].min()), float(np.abs(r64['slopes'] - 1.0).min())


# (zd, h1, h2, n) -> seed of critic_inputs.  Fixed data: each is the first seed from 7000 + 13 zd + 3 h1 + h2 + n on at which critic_conditions_hold()
# (find_critic_seed() reproduces the table); tests/test_gan_kernel_refs.py asserts the conditions for every entry.
CRITIC_SEEDS = {
    (1, 1, 1, 1): 7018, (1, 1, 1, 3): 7024, (1, 127, 129, 1): 7527, (1, 127, 129, 3): 7528, (1, 400, 400, 1): 8614, (1, 400, 400, 3): 8617,
    (127, 1, 1, 1): 8656, (127, 1, 1, 3): 8658, (127, 127, 129, 1): 9162, (127, 127, 129, 3): 9164, (127, 400, 400, 1): 10252, (127, 400, 400, 3): 10254,
    (128, 1, 1, 1): 8669, (128, 1, 1, 3): 8672, (128, 127, 129, 1): 9175, (128, 127, 129, 3): 9177, (128, 400, 400, 1): 10265, (128, 400, 400, 3): 10267,
    (129, 1, 1, 1): 8682, (129, 1, 1, 3): 8685, (129, 127, 129, 1): 9188, (129, 127, 129, 3): 9190, (129, 400, 400, 1): 10278, (129, 400, 400, 3): 10280,
    (512, 1, 1, 1): 13663, (512, 1, 1, 3): 13663, (512, 127, 129, 1): 14167, (512, 127, 129, 3): 14169, (512, 400, 400, 1): 15257, (512, 400, 400, 3): 15259,
    (5, 7, 3, 4): 7093,
}


def critic_conditions_hold(i, h1, h2):
    """the REFERENCE alone has every pre-activation MARGIN times its fp32 error away from zero, for both hat modes, every slope >= MIN_SLOPE (where
    (s - 1) / s is undefined) and |slope - 1| >= MIN_SLOPE (where the penalty (s - 1)^2 of a sample loses all relative precision in any arithmetic)"""
    for hat in (0, 1):
        ms, smin, sdist = critic_margins(i, hat, critic_zero_unit(h1, h2))
        if not (smin >= MIN_SLOPE and sdist >= MIN_SLOPE and all(lo >= MARGIN * err and lo > 0 for lo, err in ms)):
            return False
    return True


def find_critic_seed(zd, h1, h2, n, tries=200):
    """how CRITIC_SEEDS was made (CPU only, never called by a GPU test): the first of `tries` seeds from the fixed start that meets the conditions"""
    start = 7000 + 13 * zd + 3 * h1 + h2 + n
    for seed in range(start, start + tries):
        if critic_conditions_hold(critic_inputs(zd, h1, h2, n, seed), h1, h2):
            return seed
    raise AssertionError(f'no seed within {tries} of {start} meets the critic input conditions for {(zd, h1, h2, n)}')


def critic_case(zd, h1, h2, n):
    """inputs of one critic case, from the committed seed table"""
    return critic_inputs(zd, h1, h2, n, CRITIC_SEEDS[(zd, h1, h2, n)])


# ------------------------------------------------------------------------------------------------ pointwise bounds
def _rel(a32, a64):
    return float(np.abs(np.asarray(a32, np.float64) - a64).max() / max(np.abs(a64).max(), 1e-30))


def _measure_bn():
    worst = {'fwd': 0.0, 'dc': 0.0}
    for C in QRL_C:
        for rows in QRL_ROWS:
            i = bn_inputs(rows, C, seed=rows + C)
            a = (i['c'], i['gamma'], i['beta'], BN_RS0, ALPHA)
            worst['fwd'] = max(worst['fwd'], _rel(ref_bn_act_fwd(*a, dt=F), ref_bn_act_fwd(*a)))
            worst['dc'] = max(worst['dc'], _rel(ref_bn_act_bwd(i['da'], *a, dt=F)[0], ref_bn_act_bwd(i['da'], *a)[0]))
    for rows, C in BN_FWD_CASES:
        i = bn_inputs(rows, C, seed=rows + C)
        a = (i['c'], i['gamma'], i['beta'], BN_RS0, ALPHA)
        worst['fwd'] = max(worst['fwd'], _rel(ref_bn_act_fwd(*a, dt=F), ref_bn_act_fwd(*a)))
    return worst


def _measure_heads():
    worst = {'topgrad': 0.0, 'gfinal_da': 0.0}
    for t4, C in TOPGRAD_CASES:
        rows = topgrad_rows(t4, C)
        w = np.random.default_rng(t4 + C).standard_normal(C).astype(F)
        rpg = -(-rows // 4)
        worst['topgrad'] = max(worst['topgrad'], _rel(ref_topgrad(w, rows, rpg, COEF4, F), ref_topgrad(w, rows, rpg, COEF4)))
    for C in QRL_C:
        for rows in GFINAL_ROWS:
            i = gfinal_inputs(rows, C, seed=rows + C)
            for act in (0, 1, 2):
                worst['gfinal_da'] = max(worst['gfinal_da'], _rel(ref_gfinal(i['dx'], i['x'], i['a'], i['wf'], act, F)[0],
                                                                  ref_gfinal(i['dx'], i['x'], i['a'], i['wf'], act)[0]))
    return worst


def _measure_flat():
    worst = dict.fromkeys(FLAT_KINDS, 0.0)
    for name, kind in FLAT_KINDS.items():
        for n in FLAT_COUNTS:
            m = n * 4 if name.startswith('lrelu') else n
            i = flat_inputs(name, m, seed=kind * 10007 + n)
            a = (kind, i['a'], i['b'], i['c'], FLAT_COEF, i['out0'])
            worst[name] = max(worst[name], _rel(ref_flat(*a, dt=F), ref_flat(*a)))
    worst['interp'] = 0.0
    for n, hw in INTERP_CASES:
        xg, x, al = interp_inputs(n, hw)
        worst['interp'] = max(worst['interp'], _rel(ref_interp(xg, x, al, F)[2], ref_interp(xg, x, al)[2]))
    worst['sum_map'] = 0.0
    for n in SUM_N:
        a, b, _ = sum_inputs(n, seed=n)
        worst['sum_map'] = max(worst['sum_map'], _rel(ref_sum_terms(2, a, b, F), ref_sum_terms(2, a, b)))
    worst['pen_grad'] = 0.0
    for k, (n, H, W) in enumerate(PEN_GRAD_SHAPES):
        g = pen_inputs(n, H, W, seed=50 + k)
        s = ref_pen_col(g)[0].astype(F)
        worst['pen_grad'] = max(worst['pen_grad'], _rel(ref_pen_grad(g, s, PEN_COEF, F), ref_pen_grad(g, s, PEN_COEF)))
    return worst


def interp_inputs(n, hw):
    rng = np.random.default_rng(100 * n + hw)
    return rng.uniform(0, 1, (n, hw)).astype(F), rng.uniform(0, 1, (n, hw)).astype(F), rng.uniform(0, 1, n).astype(F)


_MEASURE = {'bn': _measure_bn, 'heads': _measure_heads, 'flat': _measure_flat}
_MEASURED = {}


def measured(family):
    """{output: largest relative max-norm error of the fp32 evaluation against fp64 over the family's own test inputs}"""
    if family not in _MEASURED:
        _MEASURED[family] = _MEASURE[family]()
    return _MEASURED[family]


def pointwise_bound(family, output):
    """four times the largest fp32-evaluation error seen, capped at POINTWISE_CAP"""
    return min(4.0 * measured(family)[output], POINTWISE_CAP)
