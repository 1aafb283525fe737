"""GPU: the small kernels of the materialised-graph engine (csrc/uad_gan_kernels.inc, all but the LayerNorm ones), ONE launch per assertion, against the fp64
statements of tests/gan_kernel_cases.py (pinned to the oracle on the CPU by tests/test_gan_kernel_refs.py) through the handle-less entries uad_op_gan_*,
which run the launch helpers -- and so the grid rules -- of the uad_gan_* phases.

Every output buffer is NaN before the launch and sits between two NaN guard bands of 64 floats: a value the kernel did not write, or wrote outside its
extent, fails the test; a slot that must stay unwritten (combine's other scalars, partial == NULL, the critic's mode-1 outputs) must still be NaN.  Ties and
kinks are built into the inputs (gan_kernel_cases.py); no element is left out of any comparison.

Bounds (max-norm relative, max|got - ref| <= bound * max|ref|):
  reduced quantities (column partials per workgroup, rowdot, sum partials, slopes and pen_col partials, every critic output): 1e-4 (tests/gpu_util.py REL_TOL);
  pointwise outputs: four times the largest error of the SAME expression evaluated in np.float32 against fp64 over this module's own inputs, capped at 1e-4
      (gan_kernel_cases.pointwise_bound; computed again at run time, on the CPU, never from a device result).  Measured -> bound in force:
        bn      a 1.22e-07 -> 4.88e-07   dc 7.86e-08 -> 3.14e-07
        heads   topgrad 2.12e-08 -> 8.47e-08   gfinal da 1.26e-07 -> 5.04e-07
        flat    tanh 5.89e-08 -> 2.35e-07   tanh_bwd 5.45e-08 -> 2.18e-07 (masked 8.92e-08 -> 3.57e-07)   diff_scale 8.74e-08 -> 3.50e-07
                diff_scale (accumulating) 4.09e-08 -> 1.64e-07   add 5.13e-08 -> 2.05e-07   add_scalar 5.61e-08 -> 2.25e-07
                lrelu_fwd 5.13e-08 -> 2.05e-07   lrelu_bwd 9.53e-09 -> 3.81e-08   interp 5.58e-08 -> 2.23e-07   |a - b| map 4.79e-08 -> 1.91e-07
                pen_grad 9.94e-08 -> 3.98e-07
  bit for bit: avgpool / up2 forward and backward, flip_taps, combine, sign_scale, the two copied thirds of interp, signed zeros of the LeakyReLU sites."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import gan_kernel_cases as K

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from tests.gpu_util import ptr, stream, assert_close, dev, REL_TOL
    from tests.test_gpu_step_kernels import Buf, bits, ok, ERR_INVALID, ERR_UNSUPPORTED
except Exception:  # collected on CPU boxes too
    _lib = None


def lib():
    return _lib.load()


def sync():
    torch.cuda.synchronize()


def coef4(v=K.COEF4):
    return (C.c_float * 4)(*v)


def same_bits(got, ref, what):
    assert np.array_equal(bits(got), bits(ref)), f'{what}: {int((bits(got) != bits(np.asarray(ref, np.float32))).sum())} of {got.size} values differ in their bits'


# ================================================================================================ frozen-stats BN
@functools.lru_cache(maxsize=4)
def bn_case(rows, Cc):
    i = K.bn_inputs(rows, Cc, seed=rows + Cc)
    return i, {k: dev(i[k]) for k in ('c', 'gamma', 'beta', 'da')}


@pytest.mark.parametrize('t4', K.FLAT_COUNTS)
def test_bn_act_fwd(t4):
    """t4 float4s as [t4, 4], and [t4 / 8, 32] where that is whole: the channel index wraps inside a workgroup"""
    for Cc in (4, 32):
        if (t4 * 4) % Cc:
            continue
        rows = t4 * 4 // Cc
        i, d = bn_case(rows, Cc)
        o = Buf(rows, Cc)
        ok(lib().uad_op_gan_bn_act_fwd(ptr(d['c']), ptr(d['gamma']), ptr(d['beta']), K.BN_RS0, K.ALPHA, rows, Cc, o.p, stream()))
        sync()
        got = o.host('a')
        assert_close(got, K.ref_bn_act_fwd(i['c'], i['gamma'], i['beta'], K.BN_RS0, K.ALPHA), tol=K.pointwise_bound('bn', 'fwd'), name=f't4={t4} C={Cc}')
        same_bits(got[i['zeros']], i['c'][i['zeros']], 'alpha * (+-0.0) keeps its sign')      # pre-activation +-0.0 -> alpha * (+-0.0)


@pytest.mark.parametrize('Cc', K.QRL_C)
@pytest.mark.parametrize('rows', K.QRL_ROWS)
def test_bn_act_bwd(rows, Cc):
    """the engine's 512-workgroup rule, and the 1024 rule once per shape; dc pointwise, the column partials PER WORKGROUP"""
    i, d = bn_case(rows, Cc)
    rdc, dn = K.ref_bn_act_bwd(i['da'], i['c'], i['gamma'], i['beta'], K.BN_RS0, K.ALPHA)
    for rule in (K.RULE_BN, K.RULE_GFINAL):
        B = lib().uad_op_gan_rows_blocks(rows, rule)
        assert B == K.row_split(rows, rule)[1]
        dc, cp = Buf(rows, Cc), Buf(B, 2, Cc)
        ok(lib().uad_op_gan_bn_act_bwd(ptr(d['da']), ptr(d['c']), ptr(d['gamma']), ptr(d['beta']), K.BN_RS0, K.ALPHA, rows, Cc, rule, dc.p, cp.p, stream()))
        sync()
        tag = f'rows={rows} C={Cc} rule={rule}'
        assert_close(dc.host('dc'), rdc, tol=K.pointwise_bound('bn', 'dc'), name=tag + ' dc')
        got = cp.host('colpart')
        assert_close(got[:, 0], K.block_sums(dn, rows, rule), tol=REL_TOL, name=tag + ' S1 partials')
        assert_close(got[:, 1], K.block_sums(dn * i['c'].astype(np.float64), rows, rule), tol=REL_TOL, name=tag + ' S2 partials')


# ================================================================================================ heads
@pytest.mark.parametrize('Cc', K.ROWDOT_C)
@pytest.mark.parametrize('rows', K.ROWDOT_ROWS)
def test_rowdot(rows, Cc):
    rng = np.random.default_rng(rows * 1000 + Cc)
    feat, w, b = rng.standard_normal((rows, Cc)).astype(np.float32), (rng.standard_normal(Cc) / np.sqrt(Cc)).astype(np.float32), np.float32([0.25])
    fd, wd, bd = dev(feat), dev(w), dev(b)
    for act in (0, 1, 2):
        o = Buf(rows)
        ok(lib().uad_op_gan_rowdot(act, ptr(fd), ptr(wd), ptr(bd), rows, Cc, o.p, stream()))
        sync()
        assert_close(o.host('out'), K.ref_rowdot(feat, w, b, act), tol=REL_TOL, name=f'rowdot<{act}> rows={rows} C={Cc}')


@pytest.mark.parametrize('t4,Cc', K.TOPGRAD_CASES)
def test_topgrad(t4, Cc):
    rows = K.topgrad_rows(t4, Cc)
    rpg = -(-rows // 4)
    assert rows < 4 or (rows - 1) // rpg == 3      # all four coefficient slots; with C = 4 a workgroup holds 256 rows, so the group boundaries fall inside one
    w = np.random.default_rng(t4 + Cc).standard_normal(Cc).astype(np.float32)
    wd, o = dev(w), Buf(rows, Cc)
    ok(lib().uad_op_gan_topgrad(ptr(wd), rows, rpg, Cc, coef4(), o.p, stream()))
    sync()
    assert_close(o.host('out'), K.ref_topgrad(w, rows, rpg, K.COEF4), tol=K.pointwise_bound('heads', 'topgrad'), name=f't4={t4} C={Cc}')


@pytest.mark.parametrize('Cc', K.QRL_C + K.QRL_C_WIDE)
@pytest.mark.parametrize('rows', K.COEF_ROWS)
def test_coef_colsum(rows, Cc):
    """four row groups (rows_per_group = ceil(rows / 4)): from 7 rows on a group boundary lies inside a workgroup's row range"""
    rpg = -(-rows // 4)
    feat = np.random.default_rng(rows + Cc).standard_normal((rows, Cc)).astype(np.float32)
    B = lib().uad_op_gan_rows_blocks(rows, K.RULE_COEF)
    assert B == K.row_split(rows, K.RULE_COEF)[1]
    fd, o = dev(feat), Buf(B, Cc)
    ok(lib().uad_op_gan_coef_colsum(ptr(fd), rows, rpg, Cc, coef4(), K.RULE_COEF, o.p, stream()))
    sync()
    assert_close(o.host('partial'), K.block_sums(K.ref_coef_colsum_terms(feat, rpg, K.COEF4), rows, K.RULE_COEF), tol=REL_TOL, name=f'rows={rows} C={Cc}')


@pytest.mark.parametrize('Cc', K.QRL_C)
@pytest.mark.parametrize('rows', K.GFINAL_ROWS)
def test_gfinal_bwd(rows, Cc):
    """sigmoid / tanh / linear x with / without partials (without: the partial buffer must stay NaN); the [C] slot of a partial row is the bias sum"""
    i = K.gfinal_inputs(rows, Cc, seed=rows + Cc)
    d = {k: dev(v) for k, v in i.items()}
    B = lib().uad_op_gan_rows_blocks(rows, K.RULE_GFINAL)
    assert B == K.row_split(rows, K.RULE_GFINAL)[1]
    for act in (0, 1, 2):
        rda, dv = K.ref_gfinal(i['dx'], i['x'], i['a'], i['wf'], act)
        rpart = K.block_sums(np.concatenate([dv[:, None] * i['a'].astype(np.float64), dv[:, None]], axis=1), rows, K.RULE_GFINAL)
        for with_partial in (True, False):
            tag = f'rows={rows} C={Cc} act={act} partial={with_partial}'
            da, part = Buf(rows, Cc), Buf(B, Cc + 1)
            ok(lib().uad_op_gan_gfinal_bwd(ptr(d['dx']), ptr(d['x']), ptr(d['a']), ptr(d['wf']), rows, Cc, act, K.RULE_GFINAL, da.p,
                                           part.p if with_partial else None, stream()))
            sync()
            assert_close(da.host('da'), rda, tol=K.pointwise_bound('heads', 'gfinal_da'), name=tag + ' da')
            if with_partial:
                got = part.host('partial')
                assert_close(got[:, :Cc], rpart[:, :Cc], tol=REL_TOL, name=tag + ' dw partials')
                assert_close(got[:, Cc], rpart[:, Cc], tol=REL_TOL, name=tag + ' db partials')
            else:
                assert part.untouched()


# ================================================================================================ elementwise
@pytest.mark.parametrize('n,hw', K.INTERP_CASES)
def test_interp(n, hw):
    xg, x, al = K.interp_inputs(n, hw)
    o, a, b, c = Buf(3, n, hw), dev(xg), dev(x), dev(al)
    ok(lib().uad_op_gan_interp(ptr(a), ptr(b), ptr(c), n, hw, o.p, stream()))
    sync()
    got = o.host('din')
    same_bits(got[0], xg, 'din[0] = xg')
    same_bits(got[1], x, 'din[1] = x')
    assert_close(got[2], K.ref_interp(xg, x, al)[2], tol=K.pointwise_bound('flat', 'interp'), name=f'n={n} HW={hw}')


@pytest.mark.parametrize('count', K.FLAT_COUNTS)
@pytest.mark.parametrize('name', sorted(K.FLAT_KINDS))
def test_flat(name, count):
    """count elements (float4s for the LeakyReLU kernels).  In-place kinds start from out0.  sign_scale: bit for bit, zero at the ties.  lrelu: the
    pre-activations +0.0 / -0.0 take the alpha side: alpha * (+-0.0) forward, alpha * g backward, bit for bit."""
    kind = K.FLAT_KINDS[name]
    n = count * 4 if name.startswith('lrelu') else count
    i = K.flat_inputs(name, n, seed=kind * 10007 + count)
    inplace = kind in (3, 5, 6)
    ref = K.ref_flat(kind, i['a'], i['b'], i['c'], K.FLAT_COEF, i['out0'])
    o = Buf(n, init=i['out0'] if inplace else None)
    a, b, c = dev(i['a']), dev(i['b']), (dev(i['c']) if i['c'] is not None else None)
    ok(lib().uad_op_gan_flat(kind, ptr(a), ptr(b), ptr(c), K.FLAT_COEF, n, o.p, stream()))
    sync()
    got = o.host(name)
    if name == 'sign_scale':
        same_bits(got + np.float32(0), ref.astype(np.float32) + np.float32(0), name)
        assert not got[K.tie_mask(n)].any()
        return
    assert_close(got, ref, tol=K.pointwise_bound('flat', name), name=f'{name} n={n}')
    if name == 'lrelu_fwd':
        z = np.zeros(n, bool)
        z[::5] = z[1::5] = True
        same_bits(got[z], i['a'][z], 'alpha * (+-0.0) keeps its sign')
    if name == 'lrelu_bwd':
        z = np.zeros(n, bool)
        z[::5] = z[1::5] = True
        same_bits(got[z], (np.float32(K.FLAT_COEF) * i['a'][z]).astype(np.float32), 'pre-activation +-0.0 takes the alpha side')


@pytest.mark.parametrize('n', K.SUM_N)
def test_sum(n):
    """the 256 partials one by one (idle workgroups write 0); mode 2 with the map (pointwise, exactly 0 at the ties) and without"""
    a, b, ties = K.sum_inputs(n, seed=n)
    ad, bd = dev(a), dev(b)
    assert lib().uad_op_gan_sum_blocks() == K.SUM_BLOCKS
    for mode, with_map in ((0, False), (1, False), (2, True), (2, False)):
        part, mp = Buf(K.SUM_BLOCKS), Buf(n)
        ok(lib().uad_op_gan_sum(mode, ptr(ad), ptr(bd) if mode else None, n, mp.p if with_map else None, part.p, stream()))
        sync()
        terms = K.ref_sum_terms(mode, a, b)
        assert_close(part.host('partial'), K.sum_partials(terms), tol=REL_TOL, name=f'sum<{mode}> n={n} map={with_map}')
        if with_map:
            got = mp.host('map')
            assert_close(got, terms, tol=K.pointwise_bound('flat', 'sum_map'), name=f'map n={n}')
            assert not got[ties].any()
        else:
            assert mp.untouched()


# ================================================================================================ slope penalty
@pytest.mark.parametrize('k', range(len(K.PEN_SHAPES)))
def test_pen_col(k):
    n, H, W = K.PEN_SHAPES[k]
    g = K.pen_inputs(n, H, W, seed=30 + k)
    s, t = K.ref_pen_col(g)
    B = lib().uad_op_gan_pen_col_blocks(n, W)
    assert B == -(-(n * W) // 256)
    gd, so, po = dev(g), Buf(n, W), Buf(B)
    ok(lib().uad_op_gan_pen_col(ptr(gd), n, H, W, so.p, po.p, stream()))
    sync()
    got = so.host('slopes')
    assert_close(got, s, tol=REL_TOL, name=f'slopes {n}x{H}x{W}')
    flat = np.zeros(B * 256)
    flat[:n * W] = t.reshape(-1)
    assert_close(po.host('partial'), flat.reshape(B, 256).sum(axis=1), tol=REL_TOL, name=f'partials {n}x{H}x{W}')
    if H > 1 and W > 1:
        assert got[0, 1] == 1.0, 'the unit column has slope exactly 1'


@pytest.mark.parametrize('k', range(len(K.PEN_GRAD_SHAPES)))
def test_pen_grad(k):
    n, H, W = K.PEN_GRAD_SHAPES[k]
    g = K.pen_inputs(n, H, W, seed=50 + k)
    s = K.ref_pen_col(g)[0].astype(np.float32)
    gd, sd, o = dev(g), dev(s), Buf(n, H, W)
    ok(lib().uad_op_gan_pen_grad(ptr(gd), ptr(sd), K.PEN_COEF, n, H, W, o.p, stream()))
    sync()
    assert_close(o.host('out'), K.ref_pen_grad(g, s, K.PEN_COEF), tol=K.pointwise_bound('flat', 'pen_grad'), name=f'{n}x{H}x{W}')


# ================================================================================================ pooling, upsampling, tap flip, combine: bit for bit
@pytest.mark.parametrize('Cc', K.POOL_C)
@pytest.mark.parametrize('H', K.POOL_H)
def test_pool_bits(H, Cc):
    """kinds 0 .. 3 = avgpool forward / backward, nearest x2 forward / backward, each on N in {1, 3}"""
    for N in K.POOL_N:
        rng = np.random.default_rng(100 * H + Cc + N)
        hi, lo = rng.standard_normal((N, H, H, Cc)).astype(np.float32), rng.standard_normal((N, H // 2, H // 2, Cc)).astype(np.float32)
        big = rng.standard_normal((N, 2 * H, 2 * H, Cc)).astype(np.float32)
        for kind, src, ref in ((0, hi, K.ref_avgpool_fwd(hi)), (1, lo, K.ref_avgpool_bwd(lo)), (2, hi, K.ref_up2_fwd(hi)), (3, big, K.ref_up2_bwd(big))):
            sd, o = dev(src), Buf(*ref.shape)
            ok(lib().uad_op_gan_pool(kind, ptr(sd), N, H, Cc, o.p, stream()))
            sync()
            same_bits(o.host('out'), ref, f'pool kind {kind} N={N} H={H} C={Cc}')


@pytest.mark.parametrize('Cc', K.FLIP_C)
@pytest.mark.parametrize('T', K.FLIP_T)
def test_flip_taps(T, Cc):
    w = np.random.default_rng(T * 100 + Cc).standard_normal((T, Cc)).astype(np.float32)
    wd, o = dev(w), Buf(T, Cc)
    ok(lib().uad_op_gan_flip_taps(ptr(wd), T, Cc, o.p, stream()))
    sync()
    same_bits(o.host('out'), K.ref_flip_taps(w), f'T={T} C={Cc}')


@pytest.mark.parametrize('phase', K.COMBINE_PHASES)
def test_combine(phase):
    raw, o = dev(np.array(K.COMBINE_RAW)), Buf(16)
    ok(lib().uad_op_gan_combine(phase, ptr(raw), K.COMBINE_KAPPA, o.p, stream()))
    sync()
    got, ref = o.host('scalars'), K.ref_combine(phase, K.COMBINE_RAW, K.COMBINE_KAPPA)
    for k in range(16):
        if k in ref:
            assert bits(got[k:k + 1])[0] == bits(np.array([ref[k]]))[0], f'phase {phase} scalar {k}: {got[k]!r} vs {ref[k]!r}'
        else:
            assert np.isnan(got[k]), f'phase {phase} wrote scalar {k}, which it does not define'


# ================================================================================================ latent critic
def launch_critic(i, d, zd, h1, h2, n, mode, hat):
    o = dict(d_fake=Buf(n), d_real=Buf(n), pen=Buf(n), slab=Buf(n, K.critic_size(zd, h1, h2)), dz_fake=Buf(n, zd))
    P = d['P']
    a = _lib.UadGanCritic(zd, h1, h2, mode, hat, ptr(P['W1']), ptr(P['b1']), ptr(P['W2']), ptr(P['b2']), ptr(P['W3']), ptr(P['b3']), ptr(d['zf']), ptr(d['zr']),
                          ptr(d['eps']), K.as_f32(1.0 / n), K.CRITIC_SCALE, o['d_fake'].p, o['d_real'].p, o['pen'].p, o['slab'].p, o['dz_fake'].p)
    ok(lib().uad_op_gan_critic(C.byref(a), n, stream()))
    sync()
    return o


@pytest.mark.parametrize('h1,h2', K.CRITIC_H)
@pytest.mark.parametrize('zd', K.CRITIC_ZD)
def test_critic(zd, h1, h2):
    """n in {1, 3} x both modes x both hat modes.  Critic step: d_fake, d_real, pen, the slab segment by segment (db3 exactly 0), dz_fake untouched.  Generator step:
    d_fake and dz_fake, everything else untouched."""
    for n in K.CRITIC_N:
        i = K.critic_case(zd, h1, h2, n)
        d = dict(P={k: dev(v) for k, v in i['P'].items()}, zf=dev(i['zf']), zr=dev(i['zr']), eps=dev(i['eps']))
        inv_n = K.as_f32(1.0 / n)
        for hat in (0, 1):
            tag = f'zd={zd} h=({h1},{h2}) n={n} hat={hat}'
            ref = K.ref_critic(i['P'], i['zf'], i['zr'], i['eps'], inv_n, K.CRITIC_SCALE, 0, hat)
            o = launch_critic(i, d, zd, h1, h2, n, 0, hat)
            for key in ('d_fake', 'd_real', 'pen'):
                assert_close(o[key].host(key), ref[key], tol=REL_TOL, name=f'{tag} {key}')
            slab = o['slab'].host('slab')
            for seg, sl in K.critic_segments(zd, h1, h2)[:-1]:      # each tensor's gradient against ITS OWN largest value: a small segment is not diluted by a large one
                assert_close(slab[:, sl], ref['slab'][:, sl], tol=REL_TOL, name=f'{tag} slab {seg}')
            assert not slab[:, -1].any() and not np.signbit(slab[:, -1]).any(), 'db3 is exactly +0'
            assert o['dz_fake'].untouched(), 'the critic step wrote dz_fake'
            ref1 = K.ref_critic(i['P'], i['zf'], i['zr'], i['eps'], inv_n, K.CRITIC_SCALE, 1, hat)
            o = launch_critic(i, d, zd, h1, h2, n, 1, hat)
            assert_close(o['d_fake'].host('d_fake'), ref1['d_fake'], tol=REL_TOL, name=tag + ' mode 1 d_fake')
            assert_close(o['dz_fake'].host('dz_fake'), ref1['dz_fake'], tol=REL_TOL, name=tag + ' dz_fake')
            assert all(o[key].untouched() for key in ('d_real', 'pen', 'slab')), 'the generator step wrote a critic-step output'


# ================================================================================================ refusals
def test_out_of_domain_calls_are_refused_and_launch_nothing():
    """one call per domain rule of the entries (host checks only: nothing outside a kernel's domain is ever launched): the error code comes back and every
    output is still NaN"""
    L = lib()
    some, out, out2 = dev(np.ones(8192)), Buf(8192), Buf(8192)
    s, o, o2, st, c4 = ptr(some), out.p, out2.p, stream(), coef4()
    U, I = ERR_UNSUPPORTED, ERR_INVALID
    assert L.uad_op_gan_bn_act_fwd(s, s, s, 1.0, 0.3, 4, 6, o, st) == U                       # C % 4
    assert L.uad_op_gan_bn_act_fwd(s, s, s, 1.0, 0.3, 0, 8, o, st) == I                       # rows < 1
    assert L.uad_op_gan_bn_act_bwd(s, s, s, s, 1.0, 0.3, 4, 96, 512, o, o2, st) == U          # C / 4 = 24 does not divide 256
    assert L.uad_op_gan_bn_act_bwd(s, s, s, s, 1.0, 0.3, 4, 512, 512, o, o2, st) == U         # C > 256: one thread per channel
    assert L.uad_op_gan_bn_act_bwd(s, s, s, s, 1.0, 0.3, 1, 2048, 512, o, o2, st) == U        # C > 1024: no row lane
    assert L.uad_op_gan_bn_act_bwd(s, s, s, s, 1.0, 0.3, 4, 32, 300, o, o2, st) == I          # not one of the engine's rules
    assert L.uad_op_gan_bn_act_bwd(s, s, s, s, 1.0, 0.3, 4, 32, 512, o, None, st) == I        # no colpart
    assert L.uad_op_gan_rows_blocks(0, 512) == 0 and L.uad_op_gan_rows_blocks(5, 100) == 0
    assert L.uad_op_gan_rowdot(0, s, s, s, 4, 48, o, st) == U                                 # 12 lanes per row: no power of two
    assert L.uad_op_gan_rowdot(0, s, s, s, 4, 6, o, st) == U                                  # C % 4
    assert L.uad_op_gan_rowdot(3, s, s, s, 4, 8, o, st) == I                                  # unknown activation
    assert L.uad_op_gan_rowdot(0, s, s, None, 4, 8, o, st) == I                               # no bias
    assert L.uad_op_gan_topgrad(s, 9, 2, 8, c4, o, st) == I                                   # five groups, four coefficients
    assert L.uad_op_gan_topgrad(s, 4, 1, 6, c4, o, st) == U                                   # C % 4
    assert L.uad_op_gan_coef_colsum(s, 4, 1, 96, c4, 256, o, st) == U                         # C / 4 does not divide 256
    assert L.uad_op_gan_coef_colsum(s, 1, 1, 2048, c4, 256, o, st) == U                       # C > 1024
    assert L.uad_op_gan_coef_colsum(s, 9, 2, 8, c4, 256, o, st) == I                          # five groups
    assert L.uad_op_gan_gfinal_bwd(s, s, s, s, 4, 96, 0, 1024, o, o2, st) == U                # C / 4 does not divide 256
    assert L.uad_op_gan_gfinal_bwd(s, s, s, s, 4, 512, 0, 1024, o, o2, st) == U               # partials with C > 256
    assert L.uad_op_gan_gfinal_bwd(s, s, s, s, 1, 2048, 0, 1024, o, None, st) == U            # C > 1024 even without partials
    assert L.uad_op_gan_gfinal_bwd(s, s, s, s, 4, 8, 3, 1024, o, o2, st) == I                 # unknown activation
    assert L.uad_op_gan_gfinal_bwd(s, s, None, s, 4, 8, 0, 1024, o, o2, st) == I              # partials without a
    assert L.uad_op_gan_interp(s, s, s, 2, 0, o, st) == I
    assert L.uad_op_gan_flat(9, s, s, None, 0.2, 16, o, st) == I                              # unknown kind
    assert L.uad_op_gan_flat(7, s, None, None, 0.2, 6, o, st) == U                            # LeakyReLU on a count that is no multiple of 4
    assert L.uad_op_gan_flat(1, s, None, None, 0.2, 16, o, st) == I                           # tanh_bwd without z
    assert L.uad_op_gan_flat(0, s, None, None, 0.2, 0, o, st) == I
    assert L.uad_op_gan_sum(3, s, s, 16, None, o, st) == I
    assert L.uad_op_gan_sum(1, s, None, 16, None, o, st) == I                                 # mode 1 without b
    assert L.uad_op_gan_sum(0, s, None, 16, o2, o, st) == I                                   # a map outside mode 2
    assert L.uad_op_gan_pen_col(s, 1, 0, 4, o, o2, st) == I and L.uad_op_gan_pen_col_blocks(0, 4) == 0
    assert L.uad_op_gan_pen_grad(s, s, 1.0, 1, 4, 0, o, st) == I
    assert L.uad_op_gan_pool(0, s, 1, 3, 4, o, st) == U and L.uad_op_gan_pool(1, s, 1, 5, 4, o, st) == U      # odd H for the average pooling
    assert L.uad_op_gan_pool(2, s, 1, 2, 6, o, st) == U                                       # C % 4
    assert L.uad_op_gan_pool(4, s, 1, 2, 4, o, st) == I
    assert L.uad_op_gan_flip_taps(s, 0, 4, o, st) == I
    assert L.uad_op_gan_combine(8, s, 0.5, o, st) == I and L.uad_op_gan_combine(1, None, 0.5, o, st) == I
    def crit(zd=8, h1=8, h2=8, mode=0, hat=0, slab=o2, dz=o2):
        a = _lib.UadGanCritic(zd, h1, h2, mode, hat, s, s, s, s, s, s, s, s, s, 1.0, 10.0, o, o, o, slab, dz)
        return L.uad_op_gan_critic(C.byref(a), 1, st)
    assert crit(zd=513) == U and crit(h1=401) == U and crit(h2=401) == U                      # the kernel's LDS arrays
    assert crit(zd=0) == I and crit(mode=2) == I and crit(hat=2) == I
    assert crit(slab=None) == I and crit(mode=1, dz=None) == I
    # float4 operands 4 bytes off a 16-byte boundary, in every entry that has any
    s4, o4 = C.c_void_p(some.data_ptr() + 4), C.c_void_p(out.t.data_ptr() + 4)
    assert L.uad_op_gan_bn_act_fwd(s4, s, s, 1.0, 0.3, 4, 8, o, st) == I and L.uad_op_gan_bn_act_fwd(s, s, s, 1.0, 0.3, 4, 8, o4, st) == I
    assert L.uad_op_gan_bn_act_bwd(s, s4, s, s, 1.0, 0.3, 4, 32, 512, o, o2, st) == I
    assert L.uad_op_gan_rowdot(0, s4, s, s, 4, 8, o, st) == I and L.uad_op_gan_topgrad(s, 4, 1, 8, c4, o4, st) == I
    assert L.uad_op_gan_coef_colsum(s4, 4, 1, 8, c4, 256, o, st) == I and L.uad_op_gan_gfinal_bwd(s, s, s, s4, 4, 8, 0, 1024, o, o2, st) == I
    assert L.uad_op_gan_flat(7, s4, None, None, 0.2, 8, o, st) == I and L.uad_op_gan_pool(2, s, 1, 2, 4, o4, st) == I
    # extents beyond one grid / the kernels' 32-bit indices (host checks: no tensor of that size exists or is touched)
    assert L.uad_op_gan_bn_act_fwd(s, s, s, 1.0, 0.3, 1 << 42, 8, o, st) == U and L.uad_op_gan_topgrad(s, 1 << 32, 1 << 30, 1024, c4, o, st) == U
    assert L.uad_op_gan_flat(0, s, None, None, 0.2, 1 << 42, o, st) == U and L.uad_op_gan_interp(s, s, s, 1 << 30, 1 << 30, o, st) == U
    assert L.uad_op_gan_pen_col(s, 1 << 16, 4, 1 << 16, o, o2, st) == I and L.uad_op_gan_pen_col_blocks(1 << 16, 1 << 16) == 0
    assert L.uad_op_gan_pen_grad(s, s, 1.0, 1 << 16, 4, 1 << 16, o, st) == I and L.uad_op_gan_pen_grad(s, s, 1.0, 1 << 10, 1 << 30, 1 << 10, o, st) == U
    assert L.uad_op_gan_pool(2, s, 1 << 20, 1 << 15, 64, o, st) == U
    assert L.uad_op_gan_flip_taps(s, 1 << 16, 1 << 16, o, st) == U
    assert L.uad_op_gan_flip_taps(o, 4, 4, o, st) == I                                        # out aliasing w
    assert crit(slab=None) == I                                                               # (leaves the critic's message as the last error)
    sync()
    assert out.untouched() and out2.untouched(), 'a refused call wrote to an output'
    assert b'gan_critic' in L.uad_last_error()


# ================================================================================================ census
# every __global__ this module is about (template instances included) -> the test that launches it
CENSUS = {
    'bn_act_fwd_kernel': 'test_bn_act_fwd', 'bn_act_bwd_kernel': 'test_bn_act_bwd',
    'rowdot_kernel<0>': 'test_rowdot', 'rowdot_kernel<1>': 'test_rowdot', 'rowdot_kernel<2>': 'test_rowdot',
    'topgrad_kernel': 'test_topgrad', 'coef_colsum_kernel': 'test_coef_colsum', 'gfinal_bwd_kernel': 'test_gfinal_bwd',
    'interp_kernel': 'test_interp', 'tanh_kernel': 'test_flat[tanh-*]', 'tanh_bwd_kernel': 'test_flat[tanh_bwd-*], [tanh_bwd_mask-*]',
    'diff_scale_kernel<false>': 'test_flat[diff_scale-*]', 'diff_scale_kernel<true>': 'test_flat[diff_scale_acc-*]', 'sign_scale_kernel': 'test_flat[sign_scale-*]',
    'add_kernel': 'test_flat[add-*]', 'add_scalar_kernel': 'test_flat[add_scalar-*]',
    'sum_kernel<0>': 'test_sum', 'sum_kernel<1>': 'test_sum', 'sum_kernel<2>': 'test_sum',
    'pen_col_kernel': 'test_pen_col', 'pen_grad_kernel': 'test_pen_grad',
    'avgpool_fwd_kernel': 'test_pool_bits', 'avgpool_bwd_kernel': 'test_pool_bits', 'up2_fwd_kernel': 'test_pool_bits', 'up2_bwd_kernel': 'test_pool_bits',
    'lrelu_fwd_kernel': 'test_flat[lrelu_fwd-*]', 'lrelu_bwd_kernel': 'test_flat[lrelu_bwd-*]', 'flip_taps_kernel': 'test_flip_taps',
    'combine_kernel': 'test_combine', 'critic_kernel': 'test_critic',
}


def test_census():
    """each kernel of the table is in the built library and has a test here"""
    blob = open(_lib.LIB_PATH, 'rb').read()
    for kernel, where in CENSUS.items():
        assert kernel.split('<')[0].encode() in blob, f'{kernel} is not in the library'
        assert where.split('[')[0].split(' ')[0] in globals(), where
