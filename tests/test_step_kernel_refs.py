"""CPU: the fp64 statements of tests/step_kernel_cases.py (what tests/test_gpu_step_kernels.py holds the step's small kernels to) against the oracle --
final 1x1 conv + L1, reparameterisation and the loss scalars against the loss and gradients of oracle.vae.Model on one 32 x 32 case, the first-layer data
gradient against the oracle's conv backward, the optimizers against oracle.nn.*_tf_step, the TV gradient against a central finite difference."""
import numpy as np
import pytest

from oracle import nn as onn, vae as ovae
from tests import step_kernel_cases as K

TOL = 1e-12      # fp64 against fp64: the same formulas in another order


def close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert err <= tol, err


@pytest.fixture(scope='module')
def vae_case():
    """one VAE step of the oracle at 32 x 32, batch 3, dropout masks on both heads; the operands of its dense backward calls are recorded"""
    n, h, zdim = 3, 32, 16
    m = ovae.Model('VAE', h, h, 1, 8, zdim)
    p = {k: v.astype(np.float64) for k, v in ovae.init_params(m.spec, seed=5, perturb=True).items()}
    rng = np.random.default_rng(2)
    x = ovae.synthetic_slices(n, h, h, seed=1).astype(np.float64)
    eps = rng.standard_normal((n, zdim))
    masks = {'mu': onn.make_dropout_mask(rng, (n, zdim), 0.2, np.float64), 'sigma': onn.make_dropout_mask(rng, (n, zdim), 0.2, np.float64)}
    out, cache = m.forward(p, x, eps, masks)
    calls, real = [], onn.dense_bwd

    def recording(a, w, g):
        r = real(a, w, g)
        calls.append((g, r[0]))
        return r
    onn.dense_bwd = recording
    try:
        grads = m.backward(p, x, out, cache, masks)
    finally:
        onn.dense_bwd = real
    assert len(calls) == 3      # dense_dec (returns dz), dense_mu (takes d mu_raw), dense_sigma (takes d ls_raw)
    return dict(m=m, p=p, x=x, eps=eps, masks=masks, out=out, cache=cache, grads=grads, losses=m.losses(x, out), dz=calls[0][1], dmu_raw=calls[1][0],
                dls_raw=calls[2][0], n=n)


def test_final_against_the_oracle_model(vae_case):
    v = vae_case
    p, cache, n = v['p'], v['cache'], v['n']
    last = v['m'].n_pool - 1
    bnp = f'Decoder/batch_normalization_{last + 1}'
    c, wfk, bfk = cache[f'dec_c{last}'], p['Decoder/dec_Conv2D_final/kernel'], p['Decoder/dec_Conv2D_final/bias']
    mult = 1.0 / np.sqrt(1.0 + onn.BN_EPS)
    r = K.ref_final(c, p[bnp + '/gamma'], p[bnp + '/beta'], mult, ovae.LRELU_ALPHA, wfk.reshape(-1), bfk[0], v['x'][..., 0], 1.0 / n)
    close(r['x_hat'], v['out']['x_hat'][..., 0])
    close(r['l1'], v['losses']['L1'][..., 0])
    close(r['rec'].mean(), v['losses']['reconstructionLoss'])
    g, C = v['grads'], c.shape[-1]
    close(r['red'][:C], g['Decoder/dec_Conv2D_final/kernel'].reshape(-1))
    close(r['red'][3 * C:], g['Decoder/dec_Conv2D_final/bias'])
    close(r['red'][C:2 * C], g[bnp + '/beta'])                  # S1 = d beta
    close(r['red'][2 * C:3 * C] * mult, g[bnp + '/gamma'])      # S2 / sqrt(1 + eps) = d gamma
    gx = np.sign(v['out']['x_hat'] - v['x']) / n
    da, _, _ = onn.conv2d_bwd(cache['dec_out'], wfk, gx, 1)
    dc, _, _ = onn.bn_frozen_bwd(c, p[bnp + '/gamma'], onn.leaky_relu_bwd(cache[f'dec_bn{last}'], da, ovae.LRELU_ALPHA))
    close(r['d_c'], dc)
    # the caller-supplied d / d x_hat replaces the sign term and nothing else
    r2 = K.ref_final(c, p[bnp + '/gamma'], p[bnp + '/beta'], mult, ovae.LRELU_ALPHA, wfk.reshape(-1), bfk[0], v['x'][..., 0], 123.0, dxhat_in=gx[..., 0])
    close(r2['d_c'], dc)
    close(r2['red'], r['red'])
    # a pixel declared a tie contributes nothing to the backward
    z = np.zeros(v['x'].shape[:3], bool)
    z[0, 3, 4] = True
    r3 = K.ref_final(c, p[bnp + '/gamma'], p[bnp + '/beta'], mult, ovae.LRELU_ALPHA, wfk.reshape(-1), bfk[0], v['x'][..., 0], 1.0 / n, zero_sign=z)
    assert not r3['d_c'][0, 3, 4].any() and np.array_equal(r3['d_c'][~z], r['d_c'][~z])


def test_reparam_against_the_oracle_model(vae_case):
    v = vae_case
    p, cache, nm, n = v['p'], v['cache'], v['m'].nm, v['n']
    mu_raw = onn.dense_fwd(cache['flat'], p[nm['mu'] + '/kernel'], p[nm['mu'] + '/bias'])
    ls_raw = onn.dense_fwd(cache['flat'], p[nm['sigma'] + '/kernel'], p[nm['sigma'] + '/bias'])
    mu, ls, sg, z, kl = K.ref_reparam_fwd(mu_raw, ls_raw, n, v['masks']['mu'], v['masks']['sigma'], None, v['eps'])
    for a, b in ((mu, v['out']['z_mu']), (ls, v['out']['z_log_sigma']), (sg, v['out']['z_sigma']), (z, cache['z'])):
        close(a, b)
    close(kl.mean(), v['losses']['kl'])
    dmu, dls = K.ref_reparam_bwd(v['dz'], mu, sg, n, 1.0 / n, v['eps'], v['masks']['mu'], v['masks']['sigma'])
    close(dmu, v['dmu_raw'])
    close(dls, v['dls_raw'])


def test_reparam_context_branch_against_the_oracle_model(vae_case):
    """samples [n_vae, n): the ceVAE context branch -- the oracle runs it as a forward without noise (z = masked mu) whose KL is dropped (kl = False)"""
    v = vae_case
    n, zd = v['n'], v['eps'].shape[1]
    rng = np.random.default_rng(3)
    mu_raw, ls_raw, dz = rng.standard_normal((n, zd)), rng.standard_normal((n, zd)), rng.standard_normal((n, zd))
    mce = onn.make_dropout_mask(rng, (n - 1, zd), 0.2, np.float64)
    mu, ls, sg, z, kl = K.ref_reparam_fwd(mu_raw, ls_raw, 1, v['masks']['mu'], v['masks']['sigma'], mce, v['eps'])
    a = K.ref_reparam_fwd(mu_raw[:1], ls_raw[:1], 1, v['masks']['mu'][:1], v['masks']['sigma'][:1], None, v['eps'][:1])
    for got, want in zip((mu, ls, sg, z, kl), a):
        close(got[:1], want)
    close(mu[1:], mu_raw[1:] * mce)
    close(z[1:], mu_raw[1:] * mce)
    assert not ls[1:].any() and (sg[1:] == 1).all() and not kl[1:].any()
    dmu, dls = K.ref_reparam_bwd(dz, mu, sg, 1, 1.0, v['eps'], v['masks']['mu'], v['masks']['sigma'], mce)
    close(dmu[1:], dz[1:] * mce)      # d z / d mu_raw = mask, no KL term (oracle.vae.Model.backward with kl = False, eps = 0)
    assert not dls[1:].any()


def test_loss_finalize_against_the_oracle_losses(vae_case):
    v = vae_case
    n = v['n']
    rec = np.abs(v['out']['x_hat'] - v['x']).reshape(n, -1)
    mu, ls, sg = v['out']['z_mu'], v['out']['z_log_sigma'], v['out']['z_sigma']
    kl = 0.5 * (mu * mu + sg * sg - 2.0 * ls - 1.0).sum(axis=1)
    per, s = K.ref_loss_finalize(rec.reshape(n, 4, -1).sum(axis=2), n, kl, 1.0 / n, 1.0)
    close(per, rec.sum(axis=1))
    for k, name in ((0, 'reconstructionLoss'), (1, 'kl'), (2, 'loss')):
        close(s[k], v['losses'][name])
    assert s[3] == 0 and s[7] == 0 and s[5] == 0
    # ceVAE: the handle holds [x ; x_ce], n_vae = n user samples, rec_scale 0.5
    ce = ovae.CeVAE(32, 32, 1, 8, 16)
    rng = np.random.default_rng(4)
    x, x_ce = v['x'], v['x'] * (rng.random(v['x'].shape) > 0.1)
    out = dict(v['out'], x_hat_ce=v['out']['x_hat'] + 0.01 * rng.standard_normal(v['x'].shape))
    want = ce.ce_losses(x, x_ce, out)
    rp = np.concatenate([np.abs(out['x_hat'] - x).reshape(n, -1).sum(axis=1), np.abs(out['x_hat_ce'] - x_ce).reshape(n, -1).sum(axis=1)])[:, None]
    _, s = K.ref_loss_finalize(rp, n, kl, 1.0 / n, 0.5)
    for k, name in ((0, 'reconstructionLoss'), (1, 'kl'), (2, 'loss'), (4, 'Rec_vae'), (5, 'Rec_ce'), (6, 'loss_vae')):
        close(s[k], want[name])


@pytest.mark.parametrize('k', (0, 3))
def test_first_dgrad_against_the_oracle_conv_backward(k):
    N, HB, WB, CS = K.DGRAD_SHAPES[k]
    i = K.dgrad_inputs(N, HB, WB, CS, seed=40 + k)
    x = np.zeros((N, HB, WB, 1))
    dx, _, _ = onn.conv2d_bwd(x, i['W'].astype(np.float64), i['g'].astype(np.float64), 2)
    assert onn.same_pads(HB, 5, 2)[:2] == (i['desc'][4], i['desc'][9])
    acc = K.ref_first_dgrad(i['g'], i['W'], HB, WB, 2, 1)
    close(acc, dx[..., 0])
    # ceVAE anomaly map (oracle.vae.CeVAE.ce_backward): dx = conv backward + sign(x - x_hat) / n, anomaly = |x_hat - x| |dx|
    e = K.ref_dgrad_epilogue(acc, 'anomaly', x=i['x'], x_hat=i['x_hat'], inv_batch=0.5)
    want = dx[..., 0] + np.sign(i['x'].astype(np.float64) - i['x_hat']) * 0.5
    close(e['dx'], want)
    close(e['anomaly'], np.abs(i['x_hat'].astype(np.float64) - i['x']) * np.abs(want))
    assert i['ties'].sum() > 0 and np.array_equal(e['dx'][i['ties']], acc[i['ties']]) and not e['anomaly'][i['ties']].any()
    # restoration (oracle.vae.Model.restore_grads / restore): grads = backward - dxhat, x -= lr grads
    r = K.ref_dgrad_epilogue(acc, 'restore', dxhat=i['dxhat'], x_upd=i['x_upd'], lr=1e-3)
    close(r['dx'], dx[..., 0] - i['dxhat'])
    close(r['x_upd'], i['x_upd'] - 1e-3 * (dx[..., 0] - i['dxhat']))


@pytest.mark.parametrize('kind', (1, 2, 3))
def test_optimizers_against_the_tf_form_steps(kind):
    n = 257
    p, gs = K.optim_inputs(n, seed=kind)
    h = K.OPTIM_HYPER
    p = p.astype(np.float64)
    s1, s2 = np.zeros(n), np.ones(n)      # TF: momentum / accumulator slots start at zero, the rms slot at one
    po, ao, mso = p.copy(), s1.copy(), s2.copy()
    for g in gs:
        p, s1, s2 = K.ref_optim(kind, p, g, s1, s2, **h)
        gi = g.astype(np.float64) * h['gscale']
        if kind == 1:
            onn.sgd_tf_step(po, gi, h['lr'])
        elif kind == 2:
            onn.momentum_tf_step(po, gi, ao, h['lr'], h['momentum'])
        else:
            onn.rmsprop_tf_step(po, gi, mso, ao, h['lr'], h['momentum'], h['decay'], h['eps'])
        close(p, po)
        close(s1, ao)
        close(s2, mso)


def test_tv_gradient_against_a_central_difference():
    """away from ties (every residual and every difference of neighbouring residuals at least 0.02 from zero) the objective is smooth: its central difference in each pixel
    of xh is the stated gradient"""
    rng = np.random.default_rng(6)
    N, H, W = 2, 5, 4
    r = (rng.permutation(N * H * W) - 17.5).reshape(N, H, W) * 0.05      # distinct half-integer multiples of 0.05, none zero
    x = rng.uniform(0, 1, (N, H, W))
    xh = x - r
    assert min(np.abs(r).min(), np.abs(np.diff(r, axis=1)).min(), np.abs(np.diff(r, axis=2)).min()) > 0.02
    g = K.ref_tv_dxhat(x, xh, K.TV_INV_BATCH, K.TV_LAMBDA)
    h = 1e-3
    fd = np.zeros_like(g)
    for idx in np.ndindex(*g.shape):
        d = np.zeros_like(g)
        d[idx] = h
        fd[idx] = (K.tv_objective(x, xh + d, K.TV_INV_BATCH, K.TV_LAMBDA) - K.tv_objective(x, xh - d, K.TV_INV_BATCH, K.TV_LAMBDA)) / (2 * h)
    close(g, fd, tol=1e-9)
    # and the oracle's own statement of d TV / d r
    from oracle.gmvae import total_variation_grad
    close(g, np.sign(xh - x) * K.TV_INV_BATCH - K.TV_LAMBDA * total_variation_grad(r[..., None])[..., 0])


def test_tv_inputs_hold_ties_and_zeros_and_exact_differences():
    for k, s in enumerate(K.TV_SHAPES):
        if k < 2:
            continue      # one pixel, one row: no vertical neighbour
        x, xh = K.tv_inputs(*s, seed=k)      # (the seeds of tests/test_gpu_step_kernels.py)
        r = x.astype(np.float64) - xh
        assert np.array_equal((x - xh).astype(np.float64), r), 'an fp32 subtraction of the inputs is inexact'
        assert np.array_equal(r * 1024, np.round(r * 1024))
        assert (r == 0).any() and (np.diff(r, axis=1) == 0).any() and (np.diff(r, axis=2) == 0).any()
        g = K.ref_tv_dxhat(x, xh, K.TV_INV_BATCH, K.TV_LAMBDA)
        assert (g[r == 0] % K.TV_LAMBDA == 0).all()      # sign(0) = 0: no inv_batch term where r == 0


def test_spatial_latent_against_the_oracle_primitives():
    i = K.spatial_inputs(37, 16, seed=1)
    c, ga, be, dz, mask = (i[k].astype(np.float64) for k in ('c', 'gamma', 'beta', 'dz', 'mask'))
    rs0 = 1.0 / np.sqrt(1.0 + onn.BN_EPS)
    bn = onn.bn_frozen_fwd(c, ga, be)
    close(K.ref_spatial_z_fwd(c, ga, be, rs0, K.ALPHA, mask), onn.leaky_relu_fwd(bn, K.ALPHA) * mask)      # oracle.vae.SpatialAE.forward
    dc, s1, s2 = K.ref_spatial_z_bwd(dz, c, ga, be, rs0, K.ALPHA, mask)
    want_dc, dgamma, dbeta = onn.bn_frozen_bwd(c, ga, onn.leaky_relu_bwd(bn, dz * mask, K.ALPHA))
    close(dc, want_dc)
    close(s1, dbeta)
    close(s2 * rs0, dgamma)


def test_case_tables_reach_the_edges_they_claim():
    H, W = K.short_last_block_shape()
    assert K.final_blocks(H, W) > 1 and all(0 < K.final_last_block_pixels(H, W) < K.final_pass_pixels(C) for C in K.FINAL_C)
    assert [K.final_blocks(h, w) for _, h, w in K.FINAL_SHAPES] == [1, 1, 1, 8]
    assert any(z % 64 for z in K.REPARAM_ZDIM) and max(K.LOSS_N) > 256 and {16, 64} <= set(K.FINAL_C)
    for family in ('final', 'reparam', 'dgrad', 'optim', 'spatial'):
        for name, v in K.measured(family).items():
            assert 0 < v < K.POINTWISE_CAP / 4, (family, name, v)      # fp32 round-off, far below the cap: the bound in force is 4 x measured
