"""GPU: every instance of the k5 s2 spatial kernels, one launch at a time, against the fp64 numpy oracle (oracle/nn.py + the epilogue written out).

run_plan (csrc/uad_conv_plan.hip) and launch_w_tr dispatch to the instances listed in WANTED below; the whole-model tests reach them only through a training step and
a max-norm over whole tensors.  Here each (kind, instance, epilogue form, math mode) is one test of four steps:

1. plan: uad_op_conv_plan (host only) has to name the instance the case is called after -- path, splits, slab reduction, column block, D-kind generation and
   channel range, three-plane route taken or refused.  A case that falls to the generic kernel fails.
2. inputs: seeded numpy, rounded to fp32 before the oracle sees them.  Activation-backward cases draw their pre-activations away from the kink (asserted on
   the CPU); the fused final reads the device's pattern words and is flip-aware (tests/gpu_util.py: kink_overrides, FLIP_BOUND; cap 1e-5 * elements + 8; the seed of
   its inputs is held to that cap on the CPU by tests/test_ops_spatial_seeds.py).
3. reference: oracle/nn.py in fp64, the epilogue in numpy.
4. bars (the project's own): outputs 1e-4 max-norm relative in f32 / bf16x3 and 1e-5 in bf16x6; column sums 3e-4 in f32 / bf16x3 and, in bf16x6, within
   3 x the exact-fp32 kernel's own error on the same inputs + 1e-7; every map a second time on its one-pixel frame against the whole tensor's max.

Final table of shapes (k5 s2 P = 1, HB = 2 HS; the smallest N at which the planner gives the instance in ALL three modes, i.e. >= 256 workgroups after splitting):

    F 64-column unsplit          32 -> 64   HS 32  N 16        F 64-column split x4      128 -> 128  HS 8   N 32
    F 32-column                  16 -> 32   HS 32  N 32        F not a power of two      32 -> 64    24 x 48  N 15
    D 64-column cst 128 / 64 / 32   128 -> 128  HS 16  N 32 / 16 / 8 (unsplit / x2 / x4)
    D 32-column cst 64 / 32         64 -> 32    HS 32  N 32 / 16 (unsplit / x2);  32 -> 32  HS 32  N 32
    D fallbacks                  96 -> 64  HS 16  N 64 (unsplit, cst 96) / N 32 (x2, cst 48);  96 -> 32  HS 32  N 32 / N 16 (x2);  48 -> 32  HS 32  N 32
                                 (N 16 / 8 of the 96-channel shapes are spatial in the bf16 modes only -- 128 workgroups -- and run the same instances)
    D not a power of two         64 -> 64   24 x 48  N 15
    fused final                  32 -> 32 and 64 -> 32 at 32 x 32 (N 32) and 24 x 32 (N 43)
    W                            256 x 32 and 128 x 64 channels (big x small), HS 8, N 64 (even last split) / 65 (short last split)

test_instance_census closes the file: every instance of WANTED is hit by a case (plans recomputed, nothing launched) or named in UNREACHABLE with the reason.
UAD_PARITY_LOG=<file>: one JSON line per case with the plan and the worst error per quantity (profiles/r17_ops_spatial.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import nn as onn

pytestmark = pytest.mark.gpu

try:
    import torch
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from tests.gpu_util import FLIP_BOUND, REL_TOL, desc, dev, kink_overrides, ptr, stream, xform
except Exception:  # collected on CPU boxes too
    _lib = None
    REL_TOL = 1e-4

MODES = ('f32', 'bf16x3', 'bf16x6')
TOL = {'f32': REL_TOL, 'bf16x3': REL_TOL, 'bf16x6': 1e-5}      # tests/step_parity.py: TOL
SUM_TOL = 3e-4                                                  # tests/test_gpu_ops.py: S1 / S2
EPI_BIAS, EPI_BWD, EPI_FINAL, EPI_FINAL_TRAIN, EPI_FINAL_DC = 0, 1, 2, 3, 4
XF_IN, XF_SMALL, XF_FB = 1, 2, 4
GEN = {0: 'none', 1: 'lane=pixel', 2: 'class-seq', 3: 'bf16-fallback', 4: 'f32'}
ALPHA = 0.3


def lib():
    return _lib.load()


class _Math:
    """UAD_MATH for the calls inside (the op entry points read it per call)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.get('UAD_MATH')
        if self.mode == 'f32':
            os.environ.pop('UAD_MATH', None)
        else:
            os.environ['UAD_MATH'] = self.mode

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('UAD_MATH', None)
        else:
            os.environ['UAD_MATH'] = self.old


@pytest.fixture(params=MODES)
def math_mode(request):
    m = _Math(request.param)
    m.__enter__()
    yield request.param
    m.__exit__()


def plan(d, kind, epi=EPI_BIAS, xf=0):
    out = (C.c_longlong * 12)()
    _lib.check(lib().uad_op_conv_plan(C.byref(d), ord(kind), epi, xf, out))
    v = list(out)
    if kind == 'W':
        return {'kernel': v[0], 'splits': v[1], 'short_last': v[2], 'csblocks': v[3], 'x6': v[5], 'math': v[10]}
    return {'path': v[0], 'splits': v[1], 'inkernel': v[2], 'colblock': v[3], 'tiles': v[4], 'x6': v[5], 'gen': GEN[v[6]], 'cst': v[7],
            'unsupported': v[9], 'math': v[10], 'fin_tile': v[11]}


def r32(a):
    """fp32-rounded values as fp64: device and oracle read the same numbers."""
    return np.asarray(a, np.float32).astype(np.float64)


def act(c, sc, sh, alpha):
    bn = c * sc + sh
    return np.where(bn > 0, bn, alpha * bn)


def rel_err(got, ref, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), 'non-finite values'
    return float(np.abs(got - ref).max() / max(np.abs(ref).max() if scale is None else scale, 1e-30))


def map_errors(got, ref):
    """(whole-tensor max-norm relative error, the same over the one-pixel frame of every [N, H, W, C] map -- still relative to the whole tensor's max)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    frame = np.zeros(ref.shape[1:3], bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    return rel_err(got, ref), rel_err(got[:, frame], ref[:, frame], scale)


class Record:
    """errors of one case; check() asserts a bar and keeps the figure for the log"""

    def __init__(self, case, mode, pl, instance):
        self.row = {'case': case, 'math': mode, 'plan': pl, 'instance': instance, 'err': {}}

    def check_map(self, name, got, ref, tol):
        e, f = map_errors(got, ref)
        self.row['err'][name] = e
        self.row['err'][name + ' (frame)'] = f
        print(f'{name}: {e:.3e}, frame {f:.3e} (bar {tol:.0e})')
        assert e <= tol, f'{name}: max-norm relative error {e:.3e} > {tol:.1e}'
        assert f <= tol, f'{name}: error on the one-pixel frame {f:.3e} > {tol:.1e} of the tensor max'

    def check_sum(self, name, got, ref, mode, got_f32=None, ref_f32=None):
        """column sums: 3e-4 in f32 / bf16x3; bf16x6: within 3 x the exact-fp32 kernel's error on the same inputs + 1e-7 (test_bf16x6_products_are_fp32_grade).
        ref_f32: the reference of the exact-fp32 run where it differs from `ref` (an oracle differentiated with that run's own derivative sides)"""
        e = rel_err(got, ref)
        self.row['err'][name] = e
        if mode == 'bf16x6':
            e32 = rel_err(got_f32, ref if ref_f32 is None else ref_f32)
            self.row['err'][name + ' (exact-fp32 kernel)'] = e32
            print(f'{name}: {e:.3e} (exact-fp32 kernel {e32:.3e})')
            assert e <= 3 * e32 + 1e-7, f'{name}: {e:.3e} > 3 x {e32:.3e} + 1e-7'
        else:
            print(f'{name}: {e:.3e} (bar {SUM_TOL:.0e})')
            assert e <= SUM_TOL, f'{name}: {e:.3e} > {SUM_TOL:.1e}'

    def write(self):
        if os.environ.get('UAD_PARITY_LOG'):
            with open(os.environ['UAD_PARITY_LOG'], 'a') as fh:
                fh.write(json.dumps(self.row) + '\n')


# ------------------------------------------------------------------------------------------------------------------ instances
def f_instance(p, mode, form):
    """name of the kernel instance run_plan's F branch launches for this plan"""
    if p['path'] != 1:
        return 'generic'
    if mode == 'f32' or p['x6'] == 0:
        return f'conv5_f_kernel bn{p["colblock"]}'
    return f'conv5_f16 bn{p["colblock"]} {form} npl{3 if p["x6"] == 1 else 2}'


def d_instance(p, mode, form, ck):
    if p['path'] != 1:
        return 'generic'
    if p['gen'] == 'f32':
        return f'conv5_d_kernel bn{p["colblock"]} ck{ck}' + (' final' if form.startswith('final') else '')
    if p['gen'] == 'lane=pixel':
        f = form if not form.startswith('final') else ('final-train t16' if p['fin_tile'] == 16 else form)
        return f'conv5_d16s bn{p["colblock"]} cst{p["cst"]} {f} npl{3 if p["x6"] == 1 else 2}'
    if p['gen'] == 'class-seq':
        return f'conv5_d16 bn{p["colblock"]} cst{p["cst"]}'
    return f'conv5_bf16<KIND_D> bn{p["colblock"]} ck{ck}'


def w_instance(p, xa, xs):
    if p['kernel'] != 1:
        return 'generic'
    if p['math'] == 0 or p['x6'] == 0:
        return 'conv5_w_kernel'
    return f'conv5_w_bf16_tr ncsb{p["csblocks"]} xa{int(xa)} xs{int(xs)} npl{3 if p["x6"] == 1 else 2}'


def reduction(p):
    return 'unsplit' if p['splits'] == 1 else 'in-kernel' if p['inkernel'] else 'splitk_epilogue'


D_INST = {64: (128, 64, 32), 32: (64, 32)}      # the channel ranges of the instance list, by column block (run_plan / x6_route)


def d_expected(colblock, splits, cs, form, mode, has_xf):
    """what run_plan has to pick for a D launch, written out from its branch: generation, slab reduction and three-plane route"""
    cst = cs // splits if cs % splits == 0 else 0
    inst = cst in D_INST[colblock]
    lp_form = {'bias': has_xf, 'bwd': not has_xf, 'final': has_xf, 'final-train': has_xf, 'final-dc': False}[form]      # conv5_d16s_takes
    if mode == 'f32':
        return {'gen': 'f32', 'inkernel': 0, 'x6': -1, 'cst': 0}
    if mode == 'bf16x6':
        if lp_form and inst:
            return {'gen': 'lane=pixel', 'inkernel': int(splits > 1), 'x6': 1, 'cst': cst}
        return {'gen': 'f32', 'inkernel': 0, 'x6': 0, 'cst': 0}
    if not inst:
        return {'gen': 'bf16-fallback', 'inkernel': 0, 'x6': -1, 'cst': cst}
    return {'gen': 'lane=pixel' if lp_form else 'class-seq', 'inkernel': int(splits > 1), 'x6': -1, 'cst': cst}


def assert_plan(p, want, what):
    got = {k: p[k] for k in want}
    assert got == want, f'{what}: the planner gives {p}, the case is named after {want}'


# ------------------------------------------------------------------------------------------------------------------ F kind
# name: (N, HS, WS, Cin, Cout, column block, splits)
F_CASES = {'64col-unsplit': (16, 32, 32, 32, 64, 64, 1), '64col-split4': (32, 8, 8, 128, 128, 64, 4), '32col': (32, 32, 32, 16, 32, 32, 1),
           'npot-24x48': (15, 24, 48, 32, 64, 64, 1)}
F_FORMS = ('plain', 'xf', 'bwd')


def f_plan_of(name, form, mode):
    N, HS, WS, Cin, Cout, cb, sp = F_CASES[name]
    d = desc(N, 2 * HS, 2 * WS, Cin, HS, WS, Cout, 5, 2, 1)
    with _Math(mode):
        p = plan(d, 'F', EPI_BWD if form == 'bwd' else EPI_BIAS, XF_IN if form == 'xf' else 0)
    return d, p, f_instance(p, mode, 'xf' if form == 'xf' else 'plain')


@pytest.mark.parametrize('form', F_FORMS)
@pytest.mark.parametrize('name', list(F_CASES))
def test_conv_f_spatial(name, form, math_mode):
    """Conv2D forward (bias; activation on load with mul and add) and, as 'bwd', the ConvT data gradient with the producer's activation backward and S1 / S2."""
    N, HS, WS, Cin, Cout, cb, sp = F_CASES[name]
    d, p, inst = f_plan_of(name, form, math_mode)
    bf = math_mode != 'f32'
    assert_plan(p, {'path': 1, 'splits': sp, 'colblock': cb, 'inkernel': int(sp > 1 and bf), 'x6': 1 if math_mode == 'bf16x6' else -1, 'gen': 'none'}, f'F {name} {form}')
    rec = Record(f'F {name} {form}', math_mode, p, inst + ' / ' + reduction(p))
    rng = np.random.default_rng(11)
    x = r32(rng.standard_normal((N, 2 * HS, 2 * WS, Cin)))
    w = r32(rng.standard_normal((5, 5, Cin, Cout)) / np.sqrt(25 * Cin))
    xd, wd = dev(x), dev(w)
    out = torch.empty((N, HS, WS, Cout), device='cuda')
    if form == 'bwd':
        # kernel [5,5,Cout_T = Cin, Cin_T = Cout] of a ConvT whose output gradient is x: d / d input, then the input's BN + LeakyReLU backward
        sc, sh = r32(rng.uniform(0.5, 1.5, Cout)), r32(rng.uniform(-0.5, 0.5, Cout))
        cprev = away_from_kink(rng.standard_normal((N, HS, WS, Cout)), sc, sh)
        da = onn.conv2d_fwd(x, w, None, 2)
        pos = cprev * sc + sh > 0
        dbn = np.where(pos, da, ALPHA * da)
        s1, s2 = torch.empty(Cout, device='cuda'), torch.empty(Cout, device='cuda')
        a_, keep = xform(sc, sh, ALPHA)
        cd = dev(cprev)

        def run(o, a1, a2):
            _lib.check(lib().uad_op_conv_f_bwdact(C.byref(d), ptr(xd), ptr(wd), ptr(cd), C.byref(a_), ptr(o), ptr(a1), ptr(a2), stream()))
        run(out, s1, s2)
        rec.check_map('d_c', out.cpu().numpy(), dbn * sc, TOL[math_mode])
        f1 = f2 = None
        if math_mode == 'bf16x6':
            with _Math('f32'):
                o2, f1, f2 = torch.empty_like(out), torch.empty_like(s1), torch.empty_like(s2)
                run(o2, f1, f2)
                f1, f2 = f1.cpu().numpy(), f2.cpu().numpy()
        rec.check_sum('S1', s1.cpu().numpy(), dbn.reshape(-1, Cout).sum(0), math_mode, f1)
        rec.check_sum('S2', s2.cpu().numpy(), (dbn * cprev).reshape(-1, Cout).sum(0), math_mode, f2)
    else:
        b = r32(rng.standard_normal(Cout))
        bd = dev(b)
        if form == 'xf':
            sc, sh = r32(rng.uniform(0.5, 1.5, Cin)), r32(rng.uniform(-0.5, 0.5, Cin))
            mul, add = r32(rng.uniform(0, 2, (N, HS, WS, Cout))), r32(rng.standard_normal((N, HS, WS, Cout)))
            ref = (onn.conv2d_fwd(act(x, sc, sh, ALPHA), w, b, 2)) * mul + add
            xf_, keep = xform(sc, sh, ALPHA)
            md, ad = dev(mul), dev(add)
            _lib.check(lib().uad_op_conv_f(C.byref(d), ptr(xd), C.byref(xf_), ptr(wd), ptr(bd), ptr(md), ptr(ad), ptr(out), stream()))
        else:
            ref = onn.conv2d_fwd(x, w, b, 2)
            _lib.check(lib().uad_op_conv_f(C.byref(d), ptr(xd), None, ptr(wd), ptr(bd), None, None, ptr(out), stream()))
        rec.check_map('out', out.cpu().numpy(), ref, TOL[math_mode])
    rec.write()


def away_from_kink(c, sc, sh, margin=1e-3):
    """fp32-rounded pre-BN values whose pre-activation sc * c + sh lies at least 1e-6 from the kink (asserted): the derivative side is then the same in any
    arithmetic and nothing has to be excused"""
    c = r32(c)
    near = np.abs(c * sc + sh) < margin
    c = r32(np.where(near, c + 0.01 / sc, c))
    assert np.abs(c * sc + sh).min() > 1e-6
    return c


# ------------------------------------------------------------------------------------------------------------------ D kind
# name: (N, HS, WS, CS, CB, column block, splits, CK of the streaming kernels)
D_CASES = {'64col-cst128': (32, 16, 16, 128, 128, 64, 1, 32), '64col-cst64': (16, 16, 16, 128, 128, 64, 2, 32), '64col-cst32': (8, 16, 16, 128, 128, 64, 4, 32),
           '32col-cst64': (32, 32, 32, 64, 32, 32, 1, 32), '32col-cst32-split2': (16, 32, 32, 64, 32, 32, 2, 32), '32col-cst32': (32, 32, 32, 32, 32, 32, 1, 32),
           'fallback-96to64': (64, 16, 16, 96, 64, 64, 1, 32), 'fallback-96to32': (32, 32, 32, 96, 32, 32, 1, 32), 'fallback-48to32': (32, 32, 32, 48, 32, 32, 1, 16),
           # ... and at the smallest N that is spatial in all three modes: two-way split, cst 48, slabs reduced by splitk_epilogue_kernel in the bf16 modes too
           'fallback-96to64-split2': (32, 16, 16, 96, 64, 64, 2, 32), 'fallback-96to32-split2': (16, 32, 32, 96, 32, 32, 2, 32),
           'npot-24x48': (15, 24, 48, 64, 64, 64, 1, 32)}
D_FORMS = ('bias', 'bias-xf', 'bwd')


def d_plan_of(name, form, mode):
    N, HS, WS, CS, CB, cb, sp, ck = D_CASES[name]
    d = desc(N, 2 * HS, 2 * WS, CB, HS, WS, CS, 5, 2, 1)
    with _Math(mode):
        p = plan(d, 'D', EPI_BWD if form == 'bwd' else EPI_BIAS, XF_IN if form == 'bias-xf' else 0)
    return d, p, d_instance(p, mode, 'bwd' if form == 'bwd' else 'bias', ck)


@pytest.mark.parametrize('form', D_FORMS)
@pytest.mark.parametrize('name', list(D_CASES))
def test_conv_d_spatial(name, form, math_mode):
    """Conv2DTranspose forward: bias without activation on load (class-sequential kernel), bias with it plus mul and add (lane = pixel); and, as 'bwd', the Conv2D
    data gradient with the producer's activation backward and S1 / S2 (lane = pixel; unsplit, reduced in the kernel, or by splitk_epilogue_kernel in f32).

    Found by this test: with one accumulator per fragment the three-plane lane = pixel kernel left every element ~4.5e-9 of the max too low, and the seven
    [bf16x6-*-bwd] cases on that route missed the column-sum rule on S1 (0.9e-6 .. 3.4e-6 against 0.5e-6 .. 1.8e-6 allowed); with the correction products in an accumulator
    of their own (uad_conv16s.inc: NACC) S1 is 0.7e-7 .. 2.7e-7.  DESIGN.md section 23."""
    N, HS, WS, CS, CB, cb, sp, ck = D_CASES[name]
    d, p, inst = d_plan_of(name, form, math_mode)
    want = d_expected(cb, sp, CS, 'bwd' if form == 'bwd' else 'bias', math_mode, form == 'bias-xf')
    want.update(path=1, splits=sp, colblock=cb, unsupported=0)
    assert_plan(p, want, f'D {name} {form}')
    rec = Record(f'D {name} {form}', math_mode, p, inst + ' / ' + reduction(p))
    rng = np.random.default_rng(12)
    x = r32(rng.standard_normal((N, HS, WS, CS)))
    w = r32(rng.standard_normal((5, 5, CB, CS)) / np.sqrt(25 * CS / 4))
    xd, wd = dev(x), dev(w)
    out = torch.empty((N, 2 * HS, 2 * WS, CB), device='cuda')
    if form == 'bwd':
        sc, sh = r32(rng.uniform(0.5, 1.5, CB)), r32(rng.uniform(-0.5, 0.5, CB))
        cprev = away_from_kink(rng.standard_normal((N, 2 * HS, 2 * WS, CB)), sc, sh)
        da = onn.conv2d_transpose_fwd(x, w, None, 2)          # = d / d input of the Conv2D whose output gradient is x
        pos = cprev * sc + sh > 0
        dbn = np.where(pos, da, ALPHA * da)
        s1, s2 = torch.empty(CB, device='cuda'), torch.empty(CB, device='cuda')
        a_, keep = xform(sc, sh, ALPHA)
        cd = dev(cprev)

        def run(o, a1, a2):
            _lib.check(lib().uad_op_conv_d_bwdact(C.byref(d), ptr(xd), ptr(wd), ptr(cd), C.byref(a_), ptr(o), ptr(a1), ptr(a2), stream()))
        run(out, s1, s2)
        rec.check_map('d_c', out.cpu().numpy(), dbn * sc, TOL[math_mode])
        f1 = f2 = None
        if math_mode == 'bf16x6':
            with _Math('f32'):
                o2, f1, f2 = torch.empty_like(out), torch.empty_like(s1), torch.empty_like(s2)
                run(o2, f1, f2)
                f1, f2 = f1.cpu().numpy(), f2.cpu().numpy()
        rec.check_sum('S1', s1.cpu().numpy(), dbn.reshape(-1, CB).sum(0), math_mode, f1)
        rec.check_sum('S2', s2.cpu().numpy(), (dbn * cprev).reshape(-1, CB).sum(0), math_mode, f2)
    else:
        b = r32(rng.standard_normal(CB))
        bd = dev(b)
        if form == 'bias-xf':
            sc, sh = r32(rng.uniform(0.5, 1.5, CS)), r32(rng.uniform(-0.5, 0.5, CS))
            mul, add = r32(rng.uniform(0, 2, out.shape)), r32(rng.standard_normal(out.shape))
            ref = onn.conv2d_transpose_fwd(act(x, sc, sh, ALPHA), w, b, 2) * mul + add
            xf_, keep = xform(sc, sh, ALPHA)
            md, ad = dev(mul), dev(add)
            _lib.check(lib().uad_op_conv_d(C.byref(d), ptr(xd), C.byref(xf_), ptr(wd), ptr(bd), ptr(md), ptr(ad), ptr(out), stream()))
        else:
            ref = onn.conv2d_transpose_fwd(x, w, b, 2)
            _lib.check(lib().uad_op_conv_d(C.byref(d), ptr(xd), None, ptr(wd), ptr(bd), None, None, ptr(out), stream()))
        rec.check_map('out', out.cpu().numpy(), ref, TOL[math_mode])
    rec.write()


# ------------------------------------------------------------------------------------------------------------------ fused final
# name: (N, HS, WS, CS); CB = 32.  32 x 32 runs the 16 x 16 training instance, 24 rows do not tile by 16 (8 x 16 instance)
FIN_CASES = {'32to32-hs32': (32, 32, 32, 32), '64to32-hs32': (32, 32, 32, 64), '32to32-hs24': (43, 24, 32, 32), '64to32-hs24': (43, 24, 32, 64)}
FIN_FORMS = ('final', 'final-train', 'final-dc')
FIN_SEED = 13


def fin_plan_of(name, form, mode):
    N, HS, WS, CS = FIN_CASES[name]
    d = desc(N, 2 * HS, 2 * WS, 32, HS, WS, CS, 5, 2, 1)
    with _Math(mode):
        p = plan(d, 'D', {'final': EPI_FINAL, 'final-train': EPI_FINAL_TRAIN, 'final-dc': EPI_FINAL_DC}[form], XF_IN)
        pf = plan(d, 'F', EPI_BIAS, XF_FB)
    return d, p, d_instance(p, mode, form, 32), pf


def fin_inputs(name):
    N, HS, WS, CS = FIN_CASES[name]
    rng = np.random.default_rng(FIN_SEED)
    t = {'x_in': r32(rng.standard_normal((N, HS, WS, CS))), 'w': r32(rng.standard_normal((5, 5, 32, CS)) / np.sqrt(25 * CS / 4)),
         'b': r32(0.1 * rng.standard_normal(32)), 'isc': r32(rng.uniform(0.5, 1.5, CS)), 'ish': r32(rng.uniform(-0.5, 0.5, CS)),
         'sc': r32(rng.uniform(0.5, 1.5, 32)), 'sh': r32(rng.uniform(-0.5, 0.5, 32)), 'wf': r32(rng.standard_normal(32) / np.sqrt(32)),
         'bf': r32(rng.standard_normal(1) * 0.1), 'x': r32(rng.uniform(0, 1, (N, 2 * HS, 2 * WS)))}
    return t


def fin_forward(t, dtype=np.float64):
    """the last decoder block and the final 1x1 conv in the given precision: pre-BN output c, BN output bn, x_hat"""
    g = {k: v.astype(dtype) for k, v in t.items()}
    c = onn.conv2d_transpose_fwd(act(g['x_in'], g['isc'], g['ish'], dtype(ALPHA)), g['w'], g['b'], 2)
    bn = c * g['sc'] + g['sh']
    a = np.where(bn > 0, bn, dtype(ALPHA) * bn)
    return c, bn, a, a @ g['wf'] + g['bf'][0]


@pytest.mark.parametrize('form', FIN_FORMS)
@pytest.mark.parametrize('name', list(FIN_CASES))
def test_conv_d_fused_final(name, form, math_mode):
    """The last decoder block with BN + LeakyReLU, the final C -> 1 conv and the L1 term in its epilogue: forward only, training with the compressed gradient (pattern
    words + d / d x_hat; then the F-kind launch that expands them on load), training with the uncompressed gradient (the exact-fp32 and class-sequential kernels)."""
    N, HS, WS, CS = FIN_CASES[name]
    d, p, inst, pf = fin_plan_of(name, form, math_mode)
    has_lp = form != 'final-dc'
    want = d_expected(32, 1, CS, form, math_mode, True)
    compressed_ok = not (form == 'final-train' and want['gen'] == 'f32')
    want.update(path=1, splits=1, colblock=32, unsupported=0 if compressed_ok else 1)
    if form == 'final-train' and math_mode == 'bf16x3':
        want['fin_tile'] = 16 if (CS == 32 and HS % 16 == 0) else 8
    assert_plan(p, want, f'final {name} {form}')
    t = fin_inputs(name)
    dv = {k: dev(v) for k, v in t.items()}
    inv = 1.0 / N
    xf_ = _lib.UadXform(ptr(dv['isc']), ptr(dv['ish']), ALPHA)
    bn_ = _lib.UadXform(ptr(dv['sc']), ptr(dv['sh']), ALPHA)
    npix = N * 4 * HS * WS
    xh, l1, recs = torch.empty(npix, device='cuda'), torch.empty(npix, device='cuda'), torch.empty(1, device='cuda')
    bits = torch.zeros(npix, device='cuda', dtype=torch.int32) if form == 'final-train' else None
    dxh = torch.empty(npix, device='cuda') if form == 'final-train' else None
    dc = torch.empty((N, 2 * HS, 2 * WS, 32), device='cuda') if form == 'final-dc' else None
    red = torch.empty(97, device='cuda') if form != 'final' else None

    def run(xh_, l1_, recs_, red_, dc_):
        return lib().uad_op_conv_d_final(C.byref(d), ptr(dv['x_in']), C.byref(xf_), ptr(dv['w']), ptr(dv['b']), C.byref(bn_), ptr(dv['wf']), ptr(dv['bf']),
                                         ptr(dv['x']), inv, ptr(xh_), ptr(l1_), ptr(recs_), ptr(bits), ptr(dxh), ptr(dc_), ptr(red_), stream())
    rc = run(xh, l1, recs, red, dc)
    if not compressed_ok:
        assert rc == 3, 'the exact-fp32 route has no compressed gradient: UAD_ERR_UNSUPPORTED, as the plan says'      # (a refused route is a normal outcome)
        return
    _lib.check(rc)
    rec = Record(f'final {name} {form}', math_mode, p, inst)
    c, bn, a, xh_ref = fin_forward(t)
    shp = (N, 2 * HS, 2 * WS)
    xh_dev = xh.cpu().numpy().reshape(shp)
    rec.check_map('x_hat', xh_dev[..., None], xh_ref[..., None], TOL[math_mode])
    rec.check_map('l1', l1.cpu().numpy().reshape(shp)[..., None], np.abs(xh_ref - t['x'])[..., None], TOL[math_mode])
    def sides_from_dc(dc_a, xh_a):
        """derivative sides of a run that wrote the uncompressed gradient: sign of its own x_hat - x (fp32 subtraction, as the kernel does) and, per element, which of
        the two slopes d_c = sign / n * w_f * lrelu' * scale carries"""
        sg_ = np.sign(xh_a.astype(np.float32) - t['x'].astype(np.float32)).astype(np.float64)
        base = sg_[..., None] * inv * (t['wf'] * t['sc'])
        ratio = np.divide(dc_a, base, out=np.ones_like(dc_a), where=base != 0)
        assert ((np.abs(ratio - 1) < 1e-3) | (np.abs(ratio - ALPHA) < 1e-3))[base != 0].all(), "d_c is not sign / n * w_f * lrelu' * scale"
        return np.where(base != 0, ratio > 0.65, bn > 0), sg_

    def held_sides(pos_, sg_, mode, tag):
        """every disagreement with the oracle a rounding tie of the mode, their number under the cap; returns the count"""
        _, flips, _ = kink_overrides([(np.where(pos_, 1.0, -1.0) * np.abs(bn), bn, ALPHA)], math=mode, tag=tag)
        sdiff = sg_ != np.sign(xh_ref - t['x'])
        if sdiff.any():
            mag = float(np.abs(xh_ref - t['x'])[sdiff].max() / np.abs(xh_ref).max())
            assert mag <= FLIP_BOUND[mode], f'{tag}: {int(sdiff.sum())} L1 sign disagreements with |x_hat - x| up to {mag:.2e} of the max'
        nflip = flips + int(sdiff.sum())
        cap = 1e-5 * bn.size + 8
        assert nflip <= cap, f'{tag}: {nflip} flipped derivative sides > {cap:.0f}'
        return nflip

    def oracle_sums(pos_, sg_):
        """the oracle differentiated with the given sides: (red[97] = d wf | S1 | S2 | d bf, d loss / d c)"""
        sgn = sg_ * inv
        sel = np.where(pos_, 1.0, ALPHA) * sgn[..., None]
        return np.concatenate([(sgn[..., None] * a).reshape(-1, 32).sum(0), t['wf'] * sel.reshape(-1, 32).sum(0),
                               t['wf'] * (sel * c).reshape(-1, 32).sum(0), [sgn.sum()]]), sel * t['wf'] * t['sc']

    f32 = None
    if math_mode == 'bf16x6':      # the exact-fp32 kernel on the same inputs (forward and uncompressed forms: the only ones it has)
        with _Math('f32'):
            f32 = {'rec': torch.empty(1, device='cuda'), 'red': torch.empty(97, device='cuda')}
            o1, o2 = torch.empty_like(xh), torch.empty_like(l1)
            o3 = torch.empty((N, 2 * HS, 2 * WS, 32), device='cuda') if form != 'final' else None
            saved = bits, dxh
            bits = dxh = None
            _lib.check(run(o1, o2, f32['rec'], f32['red'] if form != 'final' else None, o3))
            bits, dxh = saved
            f32 = {k: v.cpu().numpy() for k, v in f32.items()}
            if form != 'final':
                # its sums are measured against the oracle differentiated with ITS OWN sides, so that a tie it resolves differently from the three-plane run does
                # not pass for error of the exact-fp32 kernel and widen the allowance
                p32, s32 = sides_from_dc(o3.cpu().numpy().astype(np.float64), o1.cpu().numpy().reshape(shp))
                held_sides(p32, s32, 'f32', f'final {name} (exact-fp32 kernel)')
                f32['ref_red'] = oracle_sums(p32, s32)[0]
    rec.check_sum('rec', recs.cpu().numpy(), np.abs(xh_ref - t['x']).sum(keepdims=True).reshape(1), math_mode, None if f32 is None else f32['rec'])
    if form != 'final':
        # derivative sides: the device's where it says (pattern words; sign of d / d x_hat), every disagreement with the oracle a rounding tie of the mode
        if form == 'final-train':
            words = bits.cpu().numpy().view(np.uint32).reshape(shp)
            pos = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
            dx_dev = dxh.cpu().numpy().astype(np.float64).reshape(shp)
            sg = np.sign(dx_dev)
            assert np.allclose(np.abs(dx_dev[dx_dev != 0]), inv, rtol=1e-6), 'fin_dxhat is not sign(x_hat - x) / n'
        else:
            dc_dev = dc.cpu().numpy().astype(np.float64)
            pos, sg = sides_from_dc(dc_dev, xh_dev)
        rec.row['flips'] = held_sides(pos, sg, math_mode, f'final {name}')
        ref_red, ref_dc = oracle_sums(pos, sg)
        rd = red.cpu().numpy()
        for k, (lo, hi) in {'d_wf': (0, 32), 'S1': (32, 64), 'S2': (64, 96), 'd_bf': (96, 97)}.items():
            rec.check_sum(k, rd[lo:hi], ref_red[lo:hi], math_mode, None if f32 is None else f32['red'][lo:hi], None if f32 is None else f32['ref_red'][lo:hi])
        if form == 'final-dc':
            rec.check_map('d_c', dc_dev, ref_dc, TOL[math_mode])
        else:
            # the consumer: the block's data gradient with the gradient expanded from (bits, dxhat) while it is staged
            assert pf['path'] == 1 and pf['unsupported'] == int(math_mode == 'bf16x6' and pf['colblock'] == 64), pf      # (three planes: the 32-column instance only)
            rec.row['plan_f'] = pf
            gin = torch.empty((N, HS, WS, CS), device='cuda')
            rc = lib().uad_op_conv_f_final_bwd(C.byref(d), ptr(bits), ptr(dxh), ptr(dv['wf']), C.byref(bn_), ptr(dv['w']), None, None, None, ptr(gin), stream())
            if pf['unsupported']:
                assert rc == 3, 'a launch the plan reports as refused answers UAD_ERR_UNSUPPORTED'
            else:
                _lib.check(rc)
                rec.row['instance_f'] = f_instance(pf, math_mode, 'fb_bits')
                ref_gin = onn.conv2d_transpose_bwd(np.zeros((N, HS, WS, CS)), t['w'], ref_dc, 2)[0]
                rec.check_map('d_input (final backward on load)', gin.cpu().numpy(), ref_gin, TOL[math_mode])
    rec.write()


# ------------------------------------------------------------------------------------------------------------------ W kind
# name: (N, HS, CB, CS): one 8 x 8 tile per sample and eight (cb, cs) block pairs, so choose_w5 (384 workgroup slabs in the bf16 modes, 512 in f32) has 48 / 64 splits
# to give: 64 tiles split evenly in every mode, 65 leave 33 splits of two tiles with a short last one
W_CASES = {'cs32-even': (64, 8, 256, 32), 'cs32-short': (65, 8, 256, 32), 'cs64-even': (64, 8, 128, 64), 'cs64-short': (65, 8, 128, 64)}
W_FORMS = {'act-big': (True, False), 'act-small': (False, True), 'plain': (False, False), 'act-both': (True, True)}


def w_plan_of(name, form, mode):
    N, HS, CB, CS = W_CASES[name]
    xa, xs = W_FORMS[form]
    d = desc(N, 2 * HS, 2 * HS, CB, HS, HS, CS, 5, 2, 1)
    with _Math(mode):
        p = plan(d, 'W', 0, (XF_IN if xa else 0) | (XF_SMALL if xs else 0))
    return d, p, w_instance(p, xa, xs)


@pytest.mark.parametrize('form', list(W_FORMS))
@pytest.mark.parametrize('name', list(W_CASES))
def test_conv_w_spatial(name, form, math_mode):
    """Filter gradient of the k5 s2 tile kernel (choose_w5): one or two 32-channel blocks per workgroup, even or short last split, the operand forms of the
    backward; in bf16x6 the forms w_tr_x6_takes accepts run three planes, the others are reported refused and run the exact-fp32 kernel at the f32 bar."""
    N, HS, CB, CS = W_CASES[name]
    xa, xs = W_FORMS[form]
    d, p, inst = w_plan_of(name, form, math_mode)
    bf = math_mode != 'f32'
    takes = xa != xs                                           # w_tr_x6_takes without the pattern word
    x6 = -1 if math_mode != 'bf16x6' else int(takes)
    use16 = bf and x6 != 0
    want = {'kernel': 1, 'csblocks': 2 if (use16 and CS == 64) else 1, 'x6': x6}
    assert_plan(p, want, f'W {name} {form}')
    assert p['splits'] > 1 and p['short_last'] == int('short' in name), p
    rec = Record(f'W {name} {form}', math_mode, p, inst + (' / short last split' if p['short_last'] else ' / even splits'))
    rng = np.random.default_rng(14)
    big = r32(rng.standard_normal((N, 2 * HS, 2 * HS, CB)))
    small = r32(rng.standard_normal((N, HS, HS, CS)))
    scb, shb = r32(rng.uniform(0.5, 1.5, CB)), r32(rng.uniform(-0.5, 0.5, CB))
    scs, shs = r32(rng.uniform(0.5, 1.5, CS)), r32(rng.uniform(-0.5, 0.5, CS))
    _, ref, _ = onn.conv2d_bwd(act(big, scb, shb, ALPHA) if xa else big, np.zeros((5, 5, CB, CS)), act(small, scs, shs, ALPHA) if xs else small, 2)
    xb, k1 = xform(scb, shb, ALPHA) if xa else (None, ())
    xs_, k2 = xform(scs, shs, ALPHA) if xs else (None, ())
    bd, sd = dev(big), dev(small)
    dw = torch.empty((5, 5, CB, CS), device='cuda')
    _lib.check(lib().uad_op_conv_w(C.byref(d), ptr(bd), C.byref(xb) if xb else None, ptr(sd), C.byref(xs_) if xs_ else None, ptr(dw), stream()))
    e = rel_err(dw.cpu().numpy(), ref)
    tol = TOL['f32'] if x6 == 0 else TOL[math_mode]           # a refused three-plane route is the exact-fp32 kernel: held to its bar
    rec.row['err']['dW'] = e
    print(f'dW: {e:.3e} (bar {tol:.0e})')
    assert e <= tol, f'dW: {e:.3e} > {tol:.1e}'
    rec.write()


# ------------------------------------------------------------------------------------------------------------------ census
def _wanted():
    w = []
    for npl in (2, 3):
        for bn, csts in D_INST.items():
            for cst in csts:
                w += [f'conv5_d16s bn{bn} cst{cst} bias npl{npl}', f'conv5_d16s bn{bn} cst{cst} bwd npl{npl}']
        for cst in (64, 32):
            w += [f'conv5_d16s bn32 cst{cst} final npl{npl}', f'conv5_d16s bn32 cst{cst} final-train npl{npl}']
        for bn in (64, 32):
            w += [f'conv5_f16 bn{bn} plain npl{npl}', f'conv5_f16 bn{bn} xf npl{npl}', f'conv5_f16 bn{bn} fb_bits npl{npl}', f'conv5_f16 bn{bn} fb_dxhat npl{npl}']
        for ncsb in (1, 2):
            for xa, xs in ((0, 0), (0, 1), (1, 0), (1, 1)):
                if npl == 2 or xa != xs:
                    w.append(f'conv5_w_bf16_tr ncsb{ncsb} xa{xa} xs{xs} npl{npl}')
            w += [f'conv5_w_bf16_tr ncsb{ncsb} fb_bits xs{xs} npl{npl}' for xs in ((0, 1) if npl == 2 else (1,))]
    w.append('conv5_d16s bn32 cst32 final-train t16 npl2')
    for bn, csts in D_INST.items():
        w += [f'conv5_d16 bn{bn} cst{cst}' for cst in csts]
    w += ['conv5_bf16<KIND_D> bn64 ck32', 'conv5_bf16<KIND_D> bn32 ck32', 'conv5_bf16<KIND_D> bn32 ck16']
    w += ['conv5_d_kernel bn64 ck32', 'conv5_d_kernel bn32 ck32', 'conv5_d_kernel bn32 ck16', 'conv5_d_kernel bn32 ck32 final']
    w += ['conv5_f_kernel bn64', 'conv5_f_kernel bn32', 'conv5_w_kernel']
    w += ['F splitk_epilogue', 'D f32 splitk_epilogue', 'D bf16-fallback splitk_epilogue', 'F in-kernel', 'D lane=pixel in-kernel', 'D class-seq in-kernel']
    return w


# Instances run_plan's spatial branch / launch_w_tr can launch that no case of this file reaches, each with its reason (reviewed, not silently empty).
UNREACHABLE = {
    **{f'conv5_f16 bn{bn} fb_dxhat npl{npl}': 'final backward on load from the stored pre-BN output (FB = 1) is the restoration pass of the spatial GMVAE; the op entry point passes '
                                              'the pattern-word form only (uad_op_conv_f_final_bwd); held by tests/test_gpu_gmvae.py through the restore step' for bn in (64, 32) for npl in (2, 3)},
    'conv5_f16 bn64 fb_bits npl3': 'run_plan refuses it: final backward on load in three planes exists on the 32-column instance only (the entry point answers UAD_ERR_UNSUPPORTED)',
    **{f'conv5_w_bf16_tr ncsb{n} fb_bits xs{xs} npl{npl}': 'the filter gradient with the pattern word as its big operand is out of this file\'s scope (no op entry point passes it); '
                                                           'held by the training-step parity tests (tests/step_parity.py)' for n in (1, 2) for xs, npl in ((0, 2), (1, 2), (1, 3))},
}


def test_instance_census():
    """Host only: recomputes the plan of every case of this file in the three modes (nothing is launched) and names the instance each runs.  Every instance of
    WANTED has to be hit, or be listed in UNREACHABLE with its reason; nothing listed there may occur.  Run with -s for the table."""
    hit = {}

    def add(inst, where):
        hit.setdefault(inst, []).append(where)
    for mode in MODES:
        for name in F_CASES:
            for form in F_FORMS:
                _, p, inst = f_plan_of(name, form, mode)
                add(inst, f'F {name} {form} {mode}')
                if p['splits'] > 1:
                    add('F ' + reduction(p), f'F {name} {form} {mode}')
        for name in D_CASES:
            for form in D_FORMS:
                _, p, inst = d_plan_of(name, form, mode)
                add(inst, f'D {name} {form} {mode}')
                if p['splits'] > 1:
                    add(f'D {p["gen"]} ' + ('in-kernel' if p['inkernel'] else 'splitk_epilogue'), f'D {name} {form} {mode}')
        for name in FIN_CASES:
            for form in FIN_FORMS:
                _, p, inst, pf = fin_plan_of(name, form, mode)
                if not p['unsupported']:
                    add(inst, f'final {name} {form} {mode}')
                    if form == 'final-train' and not pf['unsupported']:
                        add(f_instance(pf, mode, 'fb_bits'), f'final {name} {form} {mode}')
        for name in W_CASES:
            for form in W_FORMS:
                _, p, inst = w_plan_of(name, form, mode)
                add(inst, f'W {name} {form} {mode}')
    wanted = _wanted()
    missing = []
    for inst in wanted:
        where = hit.get(inst, [])
        print(f'{inst}: {len(where)} cases' + (f', first {where[0]}' if where else (' -- UNREACHABLE: ' + UNREACHABLE[inst] if inst in UNREACHABLE else ' -- MISSING')))
        if not where and inst not in UNREACHABLE:
            missing.append(inst)
        assert not (where and inst in UNREACHABLE), f'{inst} is listed as unreachable but {where[0]} runs it'
    stray = sorted(set(hit) - set(wanted))
    assert not missing, f'no case reaches: {missing}'
    assert not stray, f'cases run instances the census does not know: {stray}'
    assert not set(UNREACHABLE) - set(wanted), 'UNREACHABLE names an instance that is not in WANTED'
