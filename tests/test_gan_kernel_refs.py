"""CPU: the fp64 statements of tests/gan_kernel_cases.py (what tests/test_gpu_gan_kernels.py holds the device kernels to) pinned to the oracle -- oracle.nn
(bn_frozen_*, leaky_relu_*, dense_*), the latent critic of oracle.aae / oracle.caae_chen (critic, critic_backward, critic_penalty and _z_hat through whole
disc_phase / gen_phase calls, whose loss dictionaries also pin combine's critic and generator branches; the other branches against the oracles' loss
formulas), the slope penalty of oracle.fanogan -- and the conditions the case tables promise: every LeakyReLU pre-activation outside the built-in zeros
is at least 10 times its fp32 evaluation error away from zero, every slope is away from 0."""
import types

import numpy as np
import pytest

from oracle import aae as oaae, caae_chen as ochen, fanogan as ofan, nn as onn
from tests import gan_kernel_cases as K

RTOL = 1e-12      # two fp64 evaluations of one formula in different association orders


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ BN, LeakyReLU
@pytest.mark.parametrize('rows,C', [(7, 4), (513, 32), (32, 32)])
def test_bn_statements_are_the_oracles(rows, C):
    """oracle.nn's rstd is 1 / sqrt(1 + 1e-3) in fp64, the kernels get its fp32 rounding K.BN_RS0: the statements are compared at the oracle's number"""
    i = K.bn_inputs(rows, C, seed=rows + C)
    c, g, b, da = (i[k].astype(np.float64) for k in ('c', 'gamma', 'beta', 'da'))
    rs0 = 1.0 / np.sqrt(1.0 + onn.BN_EPS)
    assert abs(K.BN_RS0 - rs0) <= 2.0 ** -24 * rs0
    y = onn.bn_frozen_fwd(c, g, b)
    close(K.bn_pre(c, g, b, rs0), y)
    close(K.ref_bn_act_fwd(c, g, b, rs0, K.ALPHA), onn.leaky_relu_fwd(y, K.ALPHA))
    dc, dn = K.ref_bn_act_bwd(da, c, g, b, rs0, K.ALPHA)
    odc, odg, odb = onn.bn_frozen_bwd(c, g, onn.leaky_relu_bwd(y, da, K.ALPHA))
    close(dc, odc)
    close(dn.sum(axis=0), odb)                       # S1 = d beta
    close((dn * c).sum(axis=0) * rs0, odg)           # S2 * rstd = d gamma
    for rule in (K.RULE_BN, K.RULE_GFINAL):           # the per-workgroup partials add up to the column sums
        close(K.block_sums(dn, rows, rule).sum(axis=0), dn.sum(axis=0))
        assert K.block_sums(dn, rows, rule).shape[0] == K.row_split(rows, rule)[1]


def test_lrelu_statements_are_the_oracles_at_signed_zeros_too():
    i = K.flat_inputs('lrelu_fwd', 40, seed=1)
    a = i['a'].astype(np.float64)
    assert (a[::5] == 0).all() and not np.signbit(a[::5]).any() and np.signbit(a[1::5]).all()
    got, ref = K.ref_flat(7, a, None, None, K.FLAT_COEF, None), onn.leaky_relu_fwd(a, K.FLAT_COEF)
    assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    i = K.flat_inputs('lrelu_bwd', 40, seed=2)
    assert np.array_equal(K.ref_flat(8, i['a'].astype(np.float64), i['b'].astype(np.float64), None, K.FLAT_COEF, None),
                          onn.leaky_relu_bwd(i['b'].astype(np.float64), i['a'].astype(np.float64), K.FLAT_COEF))


def test_bn_pre_activations_keep_their_margin():
    """every case of the BN tables: min |pre-activation| >= 10 x max |fp32 - fp64| outside the built-in +-0.0, which are exact in both precisions"""
    cases = {(rows, C) for C in K.QRL_C for rows in K.QRL_ROWS} | set(K.BN_FWD_CASES)
    for rows, C in sorted(cases):
        i = K.bn_inputs(rows, C, seed=rows + C)
        a = (i['c'], i['gamma'], i['beta'], K.BN_RS0)
        p64, p32 = K.bn_pre(*a), K.bn_pre(*a, dt=np.float32)
        assert K.margin_ok(p64, p32, i['zeros']), (rows, C, K.kink_margin(p64, p32, i['zeros']))
        z32 = p32[i['zeros']]
        assert np.signbit(z32).any() and not np.signbit(z32).all() if z32.size > 1 else True      # both signed zeros occur


# ------------------------------------------------------------------------------------------------ heads
def test_head_statements_are_dense_layers():
    rng = np.random.default_rng(0)
    rows, C, rpg = 11, 8, 3
    feat, w, b = rng.standard_normal((rows, C)), rng.standard_normal(C), rng.standard_normal(1)
    close(K.ref_rowdot(feat, w, b, 0), onn.dense_fwd(feat, w[:, None], b)[:, 0])
    close(K.ref_rowdot(feat, w, b, 1), 1.0 / (1.0 + np.exp(-onn.dense_fwd(feat, w[:, None], b)[:, 0])))
    close(K.ref_rowdot(feat, w, b, 2), np.tanh(onn.dense_fwd(feat, w[:, None], b)[:, 0]))
    # topgrad / coef_colsum: Dense(1) backward with d loss / d out[row] = coef[row / rows_per_group]
    g = K.group_coef(rows, rpg, K.COEF4)[:, None]
    dx, dw, _ = onn.dense_bwd(feat, w[:, None], g)
    close(K.ref_topgrad(w, rows, rpg, K.COEF4), dx)
    close(K.ref_coef_colsum_terms(feat, rpg, K.COEF4).sum(axis=0), dw[:, 0])
    # gfinal: activation derivative from the activation's OUTPUT, then the Dense(1) backward
    i = K.gfinal_inputs(rows, C, seed=3)
    dxo, x, a, wf = (i[k].astype(np.float64) for k in ('dx', 'x', 'a', 'wf'))
    for act, dact in ((0, x * (1 - x)), (1, 1 - x * x), (2, np.ones(rows))):
        da, dv = K.ref_gfinal(dxo, x, a, wf, act)
        oda, odw, odb = onn.dense_bwd(a, wf[:, None], (dxo * dact)[:, None])
        close(da, oda)
        close((dv[:, None] * a).sum(axis=0), odw[:, 0])
        close(dv.sum(), odb[0])
    s = rng.standard_normal(5)
    close(1 / (1 + np.exp(-s)) * (1 - 1 / (1 + np.exp(-s))), np.gradient(1 / (1 + np.exp(-(s[:, None] + np.array([-1e-6, 0, 1e-6])))), 1e-6, axis=1)[:, 1], 1e-6)
    close(1 - np.tanh(s) ** 2, np.gradient(np.tanh(s[:, None] + np.array([-1e-6, 0, 1e-6])), 1e-6, axis=1)[:, 1], 1e-6)


# ------------------------------------------------------------------------------------------------ slope penalty
@pytest.mark.parametrize('k', range(len(K.PEN_SHAPES)))
def test_pen_statements_are_the_fanogan_penalty(k):
    n, H, W = K.PEN_SHAPES[k]
    g = K.pen_inputs(n, H, W, seed=30 + k).astype(np.float64)
    scale = 10.0
    pen, grad = ofan.FAnoGAN.gradient_penalty(types.SimpleNamespace(scale=scale), g[..., None])
    s, t = K.ref_pen_col(g)
    close(scale * t.sum() / (n * W), pen)
    close(K.ref_pen_grad(g, s, scale * 2.0 / (n * W)), grad[..., 0])
    assert s.min() >= K.MIN_SLOPE
    if H > 1 and W > 1:
        assert s[0, 1] == 1.0 and K.ref_pen_col(g, np.float32)[0][0, 1] == 1.0


def test_pen_grad_slopes_are_away_from_zero():
    for k, (n, H, W) in enumerate(K.PEN_GRAD_SHAPES):
        assert K.ref_pen_col(K.pen_inputs(n, H, W, seed=50 + k))[0].min() >= K.MIN_SLOPE


# ------------------------------------------------------------------------------------------------ latent critic
def oracle_params(P):
    return {'Discriminator/dense/kernel': P['W1'], 'Discriminator/dense/bias': P['b1'], 'Discriminator/dense_1/kernel': P['W2'],
            'Discriminator/dense_1/bias': P['b2'], 'Discriminator/dense_2/kernel': P['W3'][:, None], 'Discriminator/dense_2/bias': P['b3']}


def slab_of(g, zd, h1, h2):
    return np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for k in
                           ('Discriminator/dense/kernel', 'Discriminator/dense/bias', 'Discriminator/dense_1/kernel', 'Discriminator/dense_1/bias',
                            'Discriminator/dense_2/kernel', 'Discriminator/dense_2/bias')])


@pytest.mark.parametrize('hat', (0, 1))
@pytest.mark.parametrize('zd,h1,h2,n', [(1, 1, 1, 3), (127, 127, 129, 3), (129, 400, 400, 1), (5, 7, 3, 4)])
def test_critic_statement_is_the_oracles_disc_and_gen_phase(zd, h1, h2, n, hat):
    """the oracle's own disc_phase / gen_phase with the encoder replaced by the case's z_: d_fake, d_real, the penalty, the gradient of every critic tensor
    (= the statement's slab summed over the samples), z_hat of both trainers, and combine's critic / generator branches against the loss dictionaries"""
    i = K.critic_case(zd, h1, h2, n)
    P64 = {k: v.astype(np.float64) for k, v in i['P'].items()}
    zf, zr, eps = (i[k].astype(np.float64) for k in ('zf', 'zr', 'eps'))
    assert K.CRITIC_ALPHA == float(np.float32(oaae.CRITIC_ALPHA))      # the kernel's 0.2f; the statements are compared at the oracle's double 0.2
    m = oaae.AAE.__new__(ochen.CAAEChen if hat else oaae.AAE)
    m.scale, m.zdim = K.CRITIC_SCALE, zd
    m.encode = lambda p, x, mask_z=None: (zf, {})
    m.encode_backward = lambda p, cache, dz, g: g.update({'Encoder/dz': dz})
    ref = K.ref_critic(P64, zf, zr, eps, 1.0 / n, K.CRITIC_SCALE, 0, hat, alpha=oaae.CRITIC_ALPHA)
    ref1 = K.ref_critic(P64, zf, zr, eps, 1.0 / n, K.CRITIC_SCALE, 1, hat, alpha=oaae.CRITIC_ALPHA)
    zh = K.z_hat(zf, zr, eps, hat)
    close(zh, m._z_hat(zr, zf, eps[:, None]))
    p = oracle_params(P64)
    losses, g = oaae.AAE.disc_phase(m, p, np.zeros((n, 1)), zr, eps)
    close(ref['d_fake'].mean(), losses['disc_fake'])
    close(ref['d_real'].mean(), losses['disc_real'])
    close(ref['pen'].sum(), losses['penalty'], 1e-11)
    close(ref['slab'].sum(axis=0), slab_of(g, zd, h1, h2), 1e-10)
    assert not ref['slab'][:, -1].any()
    d, _ = oaae.AAE.critic(m, p, zf)
    close(ref['d_fake'], d[:, 0])
    gl, gg = oaae.AAE.gen_phase(m, p, np.zeros((n, 1)))
    close(ref1['d_fake'], d[:, 0])
    close(ref1['dz_fake'], gg['Encoder/dz'])
    # combine: critic step raw = {mean d_fake, mean d_real, penalty}, generator step raw = {mean d_fake}
    raw = [losses['disc_fake'], losses['disc_real'], losses['penalty'], 0.0]
    c2, c1 = K.ref_combine(2, raw, 0.0), K.ref_combine(1, raw, 0.0)
    close(c2[K.S['DISC_LOSS']], losses['disc_loss'], 1e-6)
    close(c2[K.S['GEN_LOSS']], -losses['disc_fake'], 1e-6)
    close(c1[K.S['GEN_LOSS']], gl['gen_loss'], 1e-6)
    assert set(c1) == {K.S['DISC_FAKE'], K.S['GEN_LOSS']}


def test_critic_cases_keep_their_margins():
    """every case of the GPU table, both hat modes: pre-activations 10 x their fp32 error from zero (the built-in zero unit aside, which is exactly zero in
    both precisions), slopes away from 0 and from 1"""
    for zd in K.CRITIC_ZD:
        for h1, h2 in K.CRITIC_H:
            for n in K.CRITIC_N:
                i = K.critic_case(zd, h1, h2, n)
                assert K.find_critic_seed(zd, h1, h2, n) == K.CRITIC_SEEDS[(zd, h1, h2, n)] and K.critic_conditions_hold(i, h1, h2)
                zu = K.critic_zero_unit(h1, h2)
                assert (zu is None) == (h1 == 1 and h2 == 1)
                for hat in (0, 1):
                    ms, smin, sdist = K.critic_margins(i, hat, zu)
                    assert smin >= K.MIN_SLOPE and sdist >= K.MIN_SLOPE
                    for lo, err in ms:
                        assert lo > 0 and lo >= K.MARGIN * err, (zd, h1, h2, n, hat, lo, err)


# ------------------------------------------------------------------------------------------------ combine
def test_combine_statement_against_the_oracles_loss_algebra():
    """the branches whose phases are not run above, against the formulas of the oracles' loss dictionaries (oracle/aae.py ae_phase: loss = mean(L2 + rho Rec_z);
    oracle/vae.py, gmvae*.py, zimmerer.py: sums of the raw terms), in fp64 at fp32 tolerance; and: exactly the scalars a branch defines"""
    r = [float(v) for v in K.COMBINE_RAW]
    k = K.COMBINE_KAPPA
    rng = np.random.default_rng(5)
    l2, rz = rng.uniform(0, 1, 6), rng.uniform(0, 1, 6)
    c = K.ref_combine(4, [l2.mean(), rz.mean(), 0.3, 0.0], k)
    close(c[K.S['ENC_LOSS']], (l2 + k * rz).mean(), 1e-6)
    want = {0: r[0] + k * r[1], 3: r[0] + k * r[1], 4: r[0] + k * r[1]}
    for ph, v in want.items():
        close(K.ref_combine(ph, r, k)[K.S['ENC_LOSS']], v, 1e-6)
    close(K.ref_combine(5, r, k)[K.S['GM_LOSS']], sum(r), 1e-6)
    close(K.ref_combine(7, r, k)[K.S['GM_LOSS']], r[0] + k * (r[1] + r[2] + r[3]), 1e-6)
    c6 = K.ref_combine(6, r, k)
    close(c6[K.S['ENC_LOSS']], r[0] + r[2] + r[1], 1e-6)
    close(c6[K.S['REC_LOSS']], 0.5 * (r[0] + r[1]), 1e-6)
    close(c6[K.S['GM_LOSS']], r[0] + r[2], 1e-6)
    assert len(set(K.COMBINE_RAW)) == 4
    for j in range(4):      # every product with kappa is exact in fp32: the statement has one bit pattern, fused or not
        assert float(np.float32(K.COMBINE_KAPPA) * K.COMBINE_RAW[j]) == K.COMBINE_KAPPA * float(K.COMBINE_RAW[j])


# ------------------------------------------------------------------------------------------------ the remaining statements, and the case tables
def test_pool_statements_are_adjoint_pairs():
    rng = np.random.default_rng(9)
    x, g = rng.standard_normal((2, 4, 4, 4)).astype(np.float32), rng.standard_normal((2, 2, 2, 4)).astype(np.float32)
    close((K.ref_avgpool_fwd(x).astype(np.float64) * g).sum(), (x.astype(np.float64) * K.ref_avgpool_bwd(g)).sum(), 1e-6)
    close(K.ref_avgpool_fwd(x), x.astype(np.float64).reshape(2, 2, 2, 2, 2, 4).mean(axis=(2, 4)), 1e-6)
    big = rng.standard_normal((2, 8, 8, 4)).astype(np.float32)
    close((K.ref_up2_fwd(x).astype(np.float64) * big).sum(), (x.astype(np.float64) * K.ref_up2_bwd(big)).sum(), 1e-6)
    assert np.array_equal(K.ref_up2_fwd(x)[:, 5, 2], x[:, 2, 1])
    w = rng.standard_normal((9, 3)).astype(np.float32)
    assert np.array_equal(K.ref_flip_taps(K.ref_flip_taps(w)), w) and np.array_equal(K.ref_flip_taps(w)[0], w[8])


def test_case_tables_reach_what_they_claim():
    assert K.row_split(513, K.RULE_BN) == (2, 257) and K.row_split(1030, K.RULE_BN) == (3, 344) and 1030 - 343 * 3 == 1
    assert K.row_split(1025, K.RULE_GFINAL) == (2, 513) and K.row_split(257, K.RULE_COEF) == (2, 129)
    for C in K.QRL_C + K.QRL_C_WIDE:
        assert 256 % (C // 4) == 0 and C <= 1024
    for C in K.ROWDOT_C:
        lpr = min(C // 4, 64)
        assert lpr & (lpr - 1) == 0
    assert {min(C // 4, 64) for C in K.ROWDOT_C} == {1, 2, 16, 64} and any(C // 4 > 64 for C in K.ROWDOT_C)
    assert all((r * min(C // 4, 64)) % 256 for r in K.ROWDOT_ROWS for C in K.ROWDOT_C if r * min(C // 4, 64) != 256)
    for n in K.SUM_N:
        a, b, ties = K.sum_inputs(n, seed=n)
        assert np.array_equal(a[ties], b[ties]) and np.abs(K.sum_partials(K.ref_sum_terms(2, a, b)).sum() - np.abs(a.astype(np.float64) - b).sum()) < 1e-6
    assert K.sum_partials(np.ones(65537))[0] == 257 and K.sum_partials(np.ones(65537))[1] == 256
    i = K.flat_inputs('sign_scale', 50, seed=0)
    assert np.array_equal(i['a'][K.tie_mask(50)], i['b'][K.tie_mask(50)])
    for t4, C in K.TOPGRAD_CASES:
        K.topgrad_rows(t4, C)
