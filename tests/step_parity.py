"""One whole step of a VAE-family handle against the fp64 oracle, flip-aware -- the body test_gpu_shapes.py (ragged batches over the planner's
paths), test_gpu_handle_reuse.py (one handle stepped through a batch sequence) and test_gpu_bottleneck.py (latent widths and intermediate
resolutions over the dense bottleneck's routes) share.

A Step holds the inputs of one (architecture, size, batch) and the oracle's forward on them (computed once, kept in a small module-level cache so that
both files and every math mode reuse it).  Step.run(eng, math) does what tests/test_gpu_scale_parity.py does per mode: forward, the activation pattern
the device used (tests/gpu_util.py: device_activation_pattern, BEFORE the backward), reconstruction and scalars against the oracle, backward, and
EVERY gradient tensor of eng.spec against the oracle differentiated with the device's pattern.

Bars (all the project's own): 1e-4 max-norm relative in 'f32' and 'bf16x3' (gpu_util.REL_TOL), 1e-5 in 'bf16x6'
(test_ae_vae_bf16x6_holds_1e5_at_baseline_batch); the ceVAE anomaly map L1_vae * |d loss_vae / d x| -- a product of two quantities held to the bar --
at twice the bar (2e-4 as in test_cevae_gradients_at_baseline_batch; 2e-5 in bf16x6); flips are rounding ties (FLIP_BOUND, asserted inside
device_activation_pattern) and at most 1e-5 * (BN pre-activations) + 8 per mode (2e-5 for the ceVAE's two branches), the scale tests' cap."""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import gmvae as og
from oracle import nn as onn
from oracle import vae as ovae
from tests.gpu_util import REL_TOL, assert_close, assert_grads_close, device_activation_pattern
from unsupervised_anomaly_detection_brain_mri_amd import _lib

MODES = ('f32', 'bf16x3', 'bf16x6')
TOL = {'f32': REL_TOL, 'bf16x3': REL_TOL, 'bf16x6': 1e-5}

# test_gpu_shapes.py: (arch, height, n), each on a handle of max_batch = n.  The first eight are the sweep the file always had; the rest close the plan census
# (128 x 128 at 16 / 31: the 128- vs 256-workgroup min_wgs edge and one below a multiple of 32; 65: one past the 64-sample chunk of the bottleneck gradient
# on a max_batch-65 handle; 256 x 256 at 1: the generic kernels)
SHAPE_CASES = [('VAE', 128, 1), ('VAE', 128, 7), ('VAE', 128, 33), ('AE', 128, 64), ('VAE', 64, 19), ('VAE', 256, 3), ('ceVAE', 128, 9), ('AE', 32, 40),
               ('VAE', 128, 16), ('VAE', 128, 31), ('VAE', 128, 65), ('VAE', 256, 1)]
# test_gpu_handle_reuse.py: (arch, height, max_batch, batch sequence) -- the trainers' pattern: one handle at the batch size, full batches, ragged tails
REUSE_CASES = [('VAE', 128, 64, (64, 33, 1, 64, 7, 64)), ('ceVAE', 128, 16, (16, 9, 16)), ('GMVAE_spatial', 256, 16, (16, 5, 16)), ('AE', 32, 80, (80, 40, 64))]


def make_engine(arch, h, max_batch, zdim=128, inter=8):
    from unsupervised_anomaly_detection_brain_mri_amd.engine import Engine
    if arch == 'GMVAE_spatial':
        return Engine(arch, h, h, 1, inter, max_batch=max_batch, dim_c=9, dim_z=1, dim_w=1, c_lambda=1.0)
    return Engine(arch, h, h, 1, inter, zdim, max_batch=max_batch)


def _f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def _log(rec):
    """UAD_PARITY_LOG=<file>: one JSON line per (case, math mode) with the worst error per quantity and the flip census (profiles/ notes are made from it)."""
    if os.environ.get('UAD_PARITY_LOG'):
        with open(os.environ['UAD_PARITY_LOG'], 'a') as fh:
            fh.write(json.dumps(rec) + '\n')


class Result:
    """What one device step left: clones of the reconstruction(s), scalars and the flat gradient buffer (bit comparisons), the pattern and the errors."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def same_bits(self, other):
        return {k: bool(torch.equal(v, other.bits[k])) for k, v in self.bits.items()}


class Step:
    def __init__(self, arch, h, n, zdim=128, inter=8):
        self.arch, self.h, self.n, self.zdim, self.inter = arch, h, n, zdim, inter
        self.n_pool = int(np.log2(h // inter))
        self.tag = f'{arch} {h}x{h} n={n}' + ('' if (zdim, inter) == (128, 8) else f' zdim={zdim} inter={inter}')
        flat = inter * inter * (min(32 << (self.n_pool - 1), 128) // 8)
        self.x = ovae.synthetic_slices(n, h, h, seed=n, dtype=np.float32)
        rng = np.random.default_rng(n)
        mrng = np.random.default_rng(1000 + n)      # the dropout masks draw from a stream of their own: slices, eps and x_ce stay what the sweep always fed
        if arch == 'GMVAE_spatial':
            self.m = og.GMVAE(h, h, 1, inter, 9, 1, 1, 1.0)
            self.p32 = og.init_params(self.m.spec, seed=7, dtype=np.float32, perturb=True)
            self.e_w = rng.standard_normal((n, inter, inter, 1)).astype(np.float32)
            self.e_z = rng.standard_normal((n, inter, inter, 1)).astype(np.float32)
            self.bn = {'enc': self.m.bn[:self.n_pool], 'dec_in': self.m.bn[self.n_pool], 'dec': self.m.bn[self.n_pool + 1:]}
            self.p64, self.x64 = _f64(self.p32), self.x.astype(np.float64)
            self.out, self.cache = self.m.forward(self.p64, self.x64, self.e_w.astype(np.float64), self.e_z.astype(np.float64))
            self.ls = self.m.losses(self.x64, self.out)
            self.n_bn = sum(v.size for k, v in self.cache.items() if 'bn' in k)
            return
        self.m = ovae.CeVAE(h, h, 1, inter, zdim) if arch == 'ceVAE' else ovae.Model(arch, h, h, 1, inter, zdim)
        self.p32 = ovae.init_params(self.m.spec, seed=11, dtype=np.float32, perturb=True)
        self.eps = rng.standard_normal((n, zdim)).astype(np.float32)
        self.x_ce = self.x * (rng.random(self.x.shape) > 0.05).astype(np.float32) if arch == 'ceVAE' else None
        keys = {'AE': ('z',), 'VAE': ('mu', 'sigma', 'dec'), 'ceVAE': ('mu', 'sigma', 'dec', 'mu_ce', 'dec_ce')}[arch]
        shapes = {'z': (n, zdim), 'mu': (n, zdim), 'sigma': (n, zdim), 'dec': (n, flat), 'mu_ce': (n, zdim), 'dec_ce': (n, flat)}
        self.masks = {k: onn.make_dropout_mask(mrng, shapes[k], 0.2) for k in keys}      # keep 0.8: the three dropout sites are live
        self.bn = {'enc': [f'Encoder/batch_normalization_{i}' for i in range(self.n_pool)], 'dec_in': 'Decoder/batch_normalization',
                   'dec': [f'Decoder/batch_normalization_{i + 1}' for i in range(self.n_pool)]}
        self.p64, self.x64, self.m64 = _f64(self.p32), self.x.astype(np.float64), _f64(self.masks)
        e64 = None if arch == 'AE' else self.eps.astype(np.float64)
        if arch == 'ceVAE':
            self.xc64 = self.x_ce.astype(np.float64)
            self.out, self.cache = self.m.ce_forward(self.p64, self.x64, self.xc64, e64, self.m64)
            self.ls = self.m.ce_losses(self.x64, self.xc64, self.out)
            self.n_bn = sum(v.size for k, v in self.cache[1].items() if 'bn' in k)
        else:
            self.out, self.cache = self.m.forward(self.p64, self.x64, e64, self.m64)
            self.ls = self.m.losses(self.x64, self.out)
            self.n_bn = sum(v.size for k, v in self.cache.items() if 'bn' in k)

    @property
    def flip_cap(self):
        return (2e-5 if self.arch == 'ceVAE' else 1e-5) * self.n_bn + 8

    # ---------------------------------------------------------------- device side
    def forward(self, eng):
        if self.arch == 'GMVAE_spatial':
            return eng.gm_forward(self.x, self.e_w, self.e_z, want_backward=True)
        kw = {'x_ce': self.x_ce} if self.arch == 'ceVAE' else {}
        return eng.forward(self.x, None if self.arch == 'AE' else self.eps, self.masks, want_backward=True, **kw)

    def train_step(self, eng, lr=0.0):
        """the training entry (forward + backward + Adam in one call); lr = 0 keeps the parameters"""
        if self.arch == 'GMVAE_spatial':
            return eng.gm_train_step(self.x, self.e_w, self.e_z, lr=lr)
        kw = {'x_ce': self.x_ce} if self.arch == 'ceVAE' else {}
        return eng.train_step(self.x, None if self.arch == 'AE' else self.eps, self.masks, lr=lr, **kw)

    def pattern(self, eng, got, math):
        n, np_ = self.n, self.n_pool
        if self.arch == 'ceVAE':
            av, fv = device_activation_pattern(eng, self.p32, self.x, got['x_hat'], self.cache[1], np_, self.bn, rows=slice(0, n), math=math, xhat_oracle=self.out['x_hat'])
            ac, fc = device_activation_pattern(eng, self.p32, self.x_ce, got['x_hat_ce'], self.cache[3], np_, self.bn, rows=slice(n, 2 * n), math=math,
                                               xhat_oracle=self.out['x_hat_ce'])
            flips = type(fv)({f'vae/{k}': v for k, v in fv.items()})
            flips.update({f'ce/{k}': v for k, v in fc.items()})
            flips.l1_sign = getattr(fv, 'l1_sign', 0) + getattr(fc, 'l1_sign', 0)
            flips.mag = {**{f'vae/{k}': v for k, v in fv.mag.items()}, **{f'ce/{k}': v for k, v in fc.mag.items()}}
            return (av, ac), flips
        if self.arch == 'GMVAE_spatial':
            return device_activation_pattern(eng, self.p32, self.x, got['x_hat'], self.cache, np_, self.bn, final_kernel='dec_Conv2D_final/kernel', math=math,
                                             xhat_oracle=self.out['xz_mu'])
        return device_activation_pattern(eng, self.p32, self.x, got['x_hat'], self.cache, np_, self.bn, math=math, xhat_oracle=self.out['x_hat'])

    def check_forward(self, got, math):
        """reconstruction(s), latent outputs and scalars against the oracle; returns {quantity: relative error}"""
        tol, err = TOL[math], {}
        sc = got['scalars'].cpu().numpy()
        if self.arch == 'GMVAE_spatial':
            err['x_hat'] = assert_close(got['x_hat'].cpu().numpy(), self.out['xz_mu'], tol=tol, name=f'xz_mu ({math})')
            table = ((0, 'mean_p_loss'), (1, 'conditional_prior_loss'), (2, 'loss'), (3, 'w_prior_loss'), (4, 'c_prior_loss'))
            floor = 1e-3      # (test_gmvae_spatial_gradients_at_baseline_batch: the prior terms may sit near zero)
        else:
            err['x_hat'] = assert_close(got['x_hat'].cpu().numpy(), self.out['x_hat'], tol=tol, name=f'x_hat ({math})')
            floor = 0.0
            if self.arch == 'ceVAE':
                err['x_hat_ce'] = assert_close(got['x_hat_ce'].cpu().numpy(), self.out['x_hat_ce'], tol=tol, name=f'x_hat_ce ({math})')
                table = ((0, 'reconstructionLoss'), (1, 'kl'), (2, 'loss'), (4, 'Rec_vae'), (5, 'Rec_ce'), (6, 'loss_vae'))
            elif self.arch == 'VAE':
                table = ((0, 'reconstructionLoss'), (1, 'kl'), (2, 'loss'))
            else:
                table = ((0, 'reconstructionLoss'), (2, 'loss'))
        if self.arch != 'GMVAE_spatial':
            # the latent outputs the caller receives (ceVAE: the VAE branch's): the fused bottleneck stores them from one workgroup's first k-group only, the
            # unfused chain from its reparam kernel; nothing downstream reads z_log_sigma back, so only this comparison holds it
            for key in (('z',) if self.arch == 'AE' else ('z_mu', 'z_log_sigma', 'z_sigma')):
                err[key] = assert_close(got[key].cpu().numpy(), self.out[key], tol=tol, name=f'{key} ({math})')
        for idx, key in table:
            ref = float(self.ls[key])
            err[key] = abs(float(sc[idx]) - ref) / max(abs(ref), floor, 1e-30)
            assert abs(float(sc[idx]) - ref) <= tol * max(abs(ref), floor), f'{self.tag} {math}: {key} {sc[idx]!r} vs oracle {ref!r} (relative {err[key]:.2e} > {tol:g})'
        return err

    def oracle_grads(self, act):
        if self.arch == 'ceVAE':
            return self.m.ce_backward(self.p64, self.x64, self.xc64, self.out, self.cache, self.m64, act_v=act[0], act_c=act[1])
        if self.arch == 'GMVAE_spatial':
            return self.m.backward(self.p64, self.x64, self.out, self.cache, act=act)
        return self.m.backward(self.p64, self.x64, self.out, self.cache, self.m64, act=act)

    def run(self, eng, math, leg='fwd+bwd', grads_like=None):
        """One forward + backward on `eng` (already in mode `math`) held to the oracle.  grads_like: a Result of the same step whose gradients have passed
        -- if this step's buffers carry the same bits the oracle's backward is not repeated."""
        names = [nm for nm, _, _ in eng.spec]
        got = self.forward(eng)
        act, flips = self.pattern(eng, got, math)
        eng.backward()
        torch.cuda.synchronize()
        err = self.check_forward(got, math)
        bits = {'x_hat': got['x_hat'].clone(), 'scalars': got['scalars'].clone(), 'grads': eng.buffer(_lib.BUF_GRADS).clone()}
        if self.arch == 'ceVAE':
            bits['x_hat_ce'], bits['anomaly'] = got['x_hat_ce'].clone(), got['anomaly'].clone()
        res = Result(bits=bits, act=act, flips=flips, err=err, g=None, math=math, n=self.n)
        if grads_like is not None and all(res.same_bits(grads_like).values()):
            res.g, res.worst = grads_like.g, grads_like.worst
        else:
            res.g = self.oracle_grads(act)
            res.worst = self.check_grads(eng.get_grads(), res.g, names, math, flips, got.get('anomaly'))
        self.report(math, leg, res)
        tot = sum(flips.values())
        assert tot <= self.flip_cap, f'{self.tag} {math}: {tot} flips over the cap {self.flip_cap:.0f}: {dict(flips)} (largest |pre-activation| of the site max: {flips.mag})'
        return res

    def check_grads(self, grads, g, names, math, flips, anomaly=None):
        worst = assert_grads_close(grads, g, names, tol=TOL[math], flips=flips)
        if anomaly is not None:
            worst['anomaly'] = assert_close(anomaly.cpu().numpy(), g['anomaly'], tol=2 * TOL[math], name=f'anomaly ({math})')
        return worst

    def report(self, math, leg, res):
        w = max(res.worst, key=res.worst.get)
        fl = {k: v for k, v in res.flips.items() if v}
        mags = {k: float(f'{v:.1e}') for k, v in (res.flips.mag or {}).items()}
        print(f'\n[{self.tag} {math} {leg}] x_hat {res.err["x_hat"]:.2e} loss {res.err["loss"]:.2e}; worst gradient tensor {w}: {res.worst[w]:.2e}; flips '
              f'{sum(res.flips.values())} of {self.n_bn} (cap {self.flip_cap:.0f}) {fl} |pre-activation| <= {mags}; L1-sign disagreements {res.flips.l1_sign}')
        _log({'case': self.tag, 'math': math, 'leg': leg, 'err': {k: float(v) for k, v in res.err.items()}, 'worst_grad': [w, float(res.worst[w])],
              'flips': int(sum(res.flips.values())), 'flip_sites': fl, 'flip_mag': mags, 'l1_sign': int(res.flips.l1_sign), 'bn_preacts': int(self.n_bn)})


_STEPS = OrderedDict()


def step(arch, h, n, keep=5, zdim=128, inter=8):
    """The Step of (arch, h, n[, zdim, inter]), its oracle forward computed once: the test files and the three math modes share it (a few stay cached: an
    oracle cache of 64 slices at 128 x 128 holds every layer's fp64 activations, ~1.5 GB)."""
    key = (arch, h, n) if (zdim, inter) == (128, 8) else (arch, h, n, zdim, inter)
    if key in _STEPS:
        _STEPS.move_to_end(key)
        return _STEPS[key]
    while len(_STEPS) >= keep:
        _STEPS.popitem(last=False)
    _STEPS[key] = Step(arch, h, n, zdim, inter)
    return _STEPS[key]


# ---------------------------------------------------------------- launch plans (uad_debug_plan; nothing is launched)
def planned_blocks(eng):
    """(side, layer, kind) of every planned launch of a handle: encoder blocks 1.. (block 0 runs the one-channel first-layer kernels), every decoder block"""
    n_pool = int(np.log2(eng.h // eng.inter))
    return [(side, i, k) for side, first in (('enc', 1), ('dec', 0)) for i in range(first, n_pool) for k in 'FDW']


def has_bottleneck(eng):
    return eng.arch in ('AE', 'VAE', 'ceVAE')


def check_capacity(eng, n, shrink=1, kinds='FDWB'):
    """Every buffer uad_create sized at max_batch holds what the plan at batch n asks for: filter-gradient slabs (W, the first layer's included), BN column
    partials (data gradients), slab workspace (F / D).  The last holds by construction -- plan_gemm refuses a split whose slabs exceed the capacity it is given,
    and the handle gives it the allocated size -- and is asserted as the planner's own invariant; the first two are what uad_create has to get right.
    B: the dense bottleneck's row (AE / VAE / ceVAE) -- the slabs of its four dense / 1x1 filter gradients (generic kernel) and the scratch of its bias column
    sums, whichever route the handle takes (the GEMMs are one environment switch away on every handle).
    shrink: divide the capacities (the test's own proof that it can fail); kinds: which launches to check."""
    if 'B' in kinds and has_bottleneck(eng):
        p = eng.debug_plan('bott', 0, 'B', n)
        assert p['need'] <= p['cap'] // shrink, f'{eng.arch} max_batch {eng.max_batch} {eng.math}: the bottleneck at n = {n} needs {p["need"]} filter-gradient slab floats, allocated {p["cap"] // shrink}: {p}'
        assert p['cs_need'] <= p['cs_cap'] // shrink, f'{eng.arch} max_batch {eng.max_batch} {eng.math}: the bottleneck at n = {n} needs {p["cs_need"]} column-sum scratch floats, allocated {p["cs_cap"] // shrink}: {p}'
    for side, layer, kind in [('enc', 0, 'W')] + planned_blocks(eng):
        if kind not in kinds:
            continue
        p = eng.debug_plan(side, layer, kind, n)
        what = 'filter-gradient slab floats' if kind == 'W' else 'slab-workspace floats'
        assert p['need'] <= p['cap'] // shrink, f'{eng.arch} max_batch {eng.max_batch} {eng.math}: {side}{layer}.{kind} at n = {n} needs {p["need"]} {what}, allocated {p["cap"] // shrink}: {p}'
        if kind != 'W':
            assert p['cp_need'] <= p['cp_cap'] // shrink, f'{eng.arch} max_batch {eng.max_batch} {eng.math}: {side}{layer}.{kind} at n = {n} needs {p["cp_need"]} column-partial floats, allocated {p["cp_cap"] // shrink}'
