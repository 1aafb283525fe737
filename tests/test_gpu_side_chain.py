"""GPU: the one-launch gradient finish of the train step's side stream (uad_launch_grad_finish, csrc/uad_reduce.hip) against the separate launches it
replaces -- slab sum (reduce_partials*), BN / bias finalize (bn_grad_finalize*), and for the last decoder block the column sum of the fused loss
epilogue's partials + final_gradfin -- through uad_op_grad_finish(fused = 1 | 0).

Which rule applies: the fused launch keeps the summation order of every kernel it replaces (the slab forms run the same workgroup bodies; the BN part
gives each thread two of the old kernel's 32 tile lanes with separate accumulators and folds them in the old order; the fused-final part spreads the
s-lanes of reduce_partials_kernel over workgroups and folds them in index order).  So EVERY output is held to bit-identity with the old kernels, dW
included.  The fp64 comparison below is a check of the restated formulas on top of that, at the bound tests/test_gpu_ops.py already uses for these
column sums against fp64 (S1 / S2: 3e-4 max-norm relative)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from tests.gpu_util import ptr, stream, assert_close
except Exception:  # collected on CPU boxes too
    _lib = None

RSTD = float(np.float32(1.0) / np.sqrt(np.float32(1.0) + np.float32(1e-3)))
SUM_TOL = 3e-4      # tests/test_gpu_ops.py: S1 / S2 against fp64
S_MAX, L_MAX = 171, 25 * 128 * 128
_POOL = {}


def lib():
    return _lib.load()


def pool():
    """one buffer of random slab values for every case (a [S][L] case reads a prefix of it; never written)"""
    if 'slabs' not in _POOL:
        g = torch.Generator(device='cuda').manual_seed(7)
        _POOL['slabs'] = torch.randn(S_MAX * L_MAX + 4, device='cuda', generator=g)
    return _POOL['slabs']


def scratch():
    return torch.zeros(int(lib().uad_op_grad_finish_scratch_floats()), device='cuda')


class Part:
    """inputs of one call + the outputs of the fused and of the separate launches"""

    def __init__(self, slabs=None, S=0, L=0, T=0, Cc=0, fin_T=0, fin_C=0, seed=0):
        g = torch.Generator(device='cuda').manual_seed(100 + seed)
        self.S, self.L, self.T, self.C, self.fin_T, self.fin_C = S, L, T, Cc, fin_T, fin_C
        self.slabs = slabs
        self.colpart = torch.randn((T, 2, Cc), device='cuda', generator=g) if T else None
        self.gamma = torch.rand(Cc, device='cuda', generator=g) + 0.5 if T else None
        self.fin = torch.randn((fin_T, 3 * fin_C + 1), device='cuda', generator=g) if fin_T else None
        self.fin_gamma = torch.rand(fin_C, device='cuda', generator=g) + 0.5 if fin_T else None
        self.out = {}

    def launch(self, fused, scr):
        o = {}
        if self.slabs is not None:
            o['dW'] = torch.full((self.L,), float('nan'), device='cuda')
        if self.T:
            o.update({k: torch.full((self.C,), float('nan'), device='cuda') for k in ('dgamma', 'dbeta', 'dbias')})
        if self.fin_T:
            o.update({k: torch.full((self.fin_C,), float('nan'), device='cuda') for k in ('dwf', 'fin_dgamma', 'fin_dbeta', 'fin_dbias')})
            o['dbf'] = torch.full((1,), float('nan'), device='cuda')
            o['fin_red'] = torch.zeros(3 * self.fin_C + 1, device='cuda')
        a = _lib.UadGradFinish(ptr(self.slabs), self.S, self.L, ptr(o.get('dW')),
                               ptr(self.colpart), self.T, self.C, ptr(self.gamma), RSTD, ptr(o.get('dgamma')), ptr(o.get('dbeta')), ptr(o.get('dbias')),
                               ptr(self.fin), self.fin_T, self.fin_C, ptr(self.fin_gamma), ptr(o.get('dwf')), ptr(o.get('dbf')),
                               ptr(o.get('fin_dgamma')), ptr(o.get('fin_dbeta')), ptr(o.get('fin_dbias')), ptr(o.get('fin_red')))
        _lib.check(lib().uad_op_grad_finish(C.byref(a), int(fused), ptr(scr), stream()))
        o.pop('fin_red', None)
        self.out[bool(fused)] = o

    def check_bits(self, tag):
        for k, v in self.out[True].items():
            a, b = v.cpu().numpy(), self.out[False][k].cpu().numpy()
            assert np.isfinite(b).all(), f'{tag} {k}: the separate launches left a value unwritten'
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                f'{tag} {k}: fused and separate launches differ in {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} values'

    def check_fp64(self, tag):
        """fp64 restatement of bn_grad_finalize_kernel and final_gradfin_kernel"""
        o = {k: v.cpu().numpy() for k, v in self.out[True].items()}
        if self.T:
            cp, ga = self.colpart.cpu().numpy().astype(np.float64), self.gamma.cpu().numpy().astype(np.float64)
            s1, s2 = cp[:, 0].sum(0), cp[:, 1].sum(0)
            for k, ref in (('dbeta', s1), ('dgamma', RSTD * s2), ('dbias', ga * RSTD * s1)):
                print(f'{tag} {k}: {assert_close(o[k], ref, tol=SUM_TOL, name=tag + " " + k):.2e}')
        if self.fin_T:
            Cf = self.fin_C
            red = self.fin.cpu().numpy().astype(np.float64).sum(0)
            ga = self.fin_gamma.cpu().numpy().astype(np.float64)
            s1, s2 = red[Cf:2 * Cf], red[2 * Cf:3 * Cf]
            for k, ref in (('dwf', red[:Cf]), ('dbf', red[3 * Cf:]), ('fin_dbeta', s1), ('fin_dgamma', RSTD * s2), ('fin_dbias', ga * RSTD * s1)):
                print(f'{tag} {k}: {assert_close(o[k], ref, tol=SUM_TOL, name=tag + " " + k):.2e}')
        if self.slabs is not None and self.S * self.L <= 9 * 25 * 32 * 64:
            ref = self.slabs[:self.S * self.L].cpu().numpy().astype(np.float64).reshape(self.S, self.L).sum(0)
            assert_close(o['dW'], ref, name=tag + ' dW')


def slab_view(S, L, misaligned=False):
    off = 1 if misaligned else 0      # one float = 4 bytes off the 16-byte grid: the scalar form
    return pool()[off:off + S * L]


SLAB_CASES = [(S, L) for S in (1, 2, 9, 171) for L in (25 * 32 * 32, 25 * 32 * 64, 25 * 128 * 128)]
BN_CASES = [(T, Cc) for T in (1, 127, 128, 511, 2049) for Cc in (32, 64, 128)]


@pytest.mark.parametrize('k', range(len(SLAB_CASES) + 1))
def test_slab_sum_bits(k):
    """every slab count x slab length (+ one slab pointer 4 bytes off: the scalar form), each with a BN part in the same launch"""
    mis = k == len(SLAB_CASES)
    S, L = (171, 25 * 32 * 64) if mis else SLAB_CASES[k]
    T, Cc = BN_CASES[(5 * k + 3) % len(BN_CASES)]
    p = Part(slab_view(S, L, mis), S, L, T, Cc, seed=k)
    scr = scratch()
    p.launch(True, scr)
    p.launch(False, scr)
    torch.cuda.synchronize()
    p.check_bits(f'S={S} L={L} T={T} C={Cc}{" misaligned" if mis else ""}')
    p.check_fp64(f'S={S} L={L}')
    assert not scr[:64].any(), 'an arrival counter was left non-zero'


@pytest.mark.parametrize('T,Cc', BN_CASES)
def test_bn_finalize_bits(T, Cc):
    """every colpart row count (one tile range, the 8 / 16 / 32-range thresholds and their neighbours) x width, behind a slab part"""
    p = Part(slab_view(9, 25 * 32 * 32), 9, 25 * 32 * 32, T, Cc, seed=T + Cc)
    scr = scratch()
    p.launch(True, scr)
    p.launch(False, scr)
    torch.cuda.synchronize()
    p.check_bits(f'T={T} C={Cc}')
    p.check_fp64(f'T={T} C={Cc}')


@pytest.mark.parametrize('T', [64, 2048])
@pytest.mark.parametrize('fin_T', [8, 64, 2048])
def test_bn_and_fused_final_outputs(T, fin_T):
    """BN / bias outputs and the fused-final outputs (C = 32) against fp64 and, bit for bit, against the old kernels; fin_T = 8 is the four-lane form"""
    p = Part(slab_view(9, 25 * 32 * 32), 9, 25 * 32 * 32, T, 32, fin_T, 32, seed=T + fin_T)
    scr = scratch()
    p.launch(True, scr)
    p.launch(False, scr)
    torch.cuda.synchronize()
    p.check_bits(f'T={T} fin_T={fin_T}')
    p.check_fp64(f'T={T} fin_T={fin_T}')
    assert not scr[:64].any(), 'an arrival counter was left non-zero'


def test_scratch_reuse_back_to_back():
    """two fused launches on one stream sharing the scratch, different T and C (and a fused-final part in the first): counters reset, no stale partials"""
    a = Part(slab_view(9, 25 * 32 * 32), 9, 25 * 32 * 32, 2048, 128, 2048, 32, seed=1)
    b = Part(slab_view(2, 25 * 32 * 64), 2, 25 * 32 * 64, 511, 32, 64, 32, seed=2)
    scr = scratch()
    a.launch(True, scr)
    b.launch(True, scr)
    a.launch(True, scr)
    last = {k: v.clone() for k, v in a.out[True].items()}
    torch.cuda.synchronize()
    ref = scratch()
    a.launch(False, ref)
    b.launch(False, ref)
    torch.cuda.synchronize()
    a.check_bits('first')
    b.check_bits('second')
    a.check_fp64('first')
    b.check_fp64('second')
    assert all(torch.equal(v, a.out[True][k]) for k, v in last.items())


def test_parts_alone_and_limits():
    """a launch with only one of the parts; widths the launch does not take are refused, not run"""
    scr = scratch()
    for kw in (dict(T=128, Cc=64), dict(fin_T=64, fin_C=32), dict(slabs=slab_view(9, 25 * 32 * 32), S=9, L=25 * 32 * 32)):
        p = Part(**kw)
        p.launch(True, scr)
        p.launch(False, scr)
        torch.cuda.synchronize()
        p.check_bits(str(sorted(k for k in kw if k != 'slabs')))
    p = Part(T=4, Cc=544)
    with pytest.raises(Exception):
        p.launch(True, scr)


_STEP_SCRIPT = r'''
import sys, numpy as np, torch
from unsupervised_anomaly_detection_brain_mri_amd.engine import Engine
from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import synthetic_slices
eng = Engine('VAE', 64, 64, 1, 8, 64, max_batch=8, math='bf16x3')
eng.set_params(np.random.default_rng(0).standard_normal(eng.nparams).astype(np.float32) * 0.05)
outs = []
for step, n in enumerate((3, 8, 3, 8)):          # the same handle again and again, fresh inputs every step
    x = synthetic_slices(n, 64, 64, seed=20 + step)
    eps = np.random.default_rng(200 + step).standard_normal((n, 64)).astype(np.float32)
    eng.forward(x, eps, None, want_backward=True)
    eng.backward()
    torch.cuda.synchronize()
    outs.append(eng.get_buffer_host(1).copy())          # BUF_GRADS: every gradient tensor
np.save(sys.argv[1], np.stack(outs))
'''


def test_whole_step_with_and_without_the_switch(tmp_path):
    """One VAE step at 64 x 64, batch 3 and batch 8, twice each on one handle: every gradient tensor of the fused side chain equals, bit for bit,
    that of UAD_NO_SIDE_FUSE (the switch is read once per process: one fresh interpreter per setting)."""
    res = {}
    for tag, env in (('fused', {}), ('separate', {'UAD_NO_SIDE_FUSE': '1'})):
        out = str(tmp_path / (tag + '.npy'))
        e = {k: v for k, v in os.environ.items() if k != 'UAD_NO_SIDE_FUSE'}
        r = subprocess.run([sys.executable, '-c', _STEP_SCRIPT, out], cwd=ROOT, env=dict(e, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
        res[tag] = np.load(out)
    f, s = res['fused'], res['separate']
    assert f.shape == s.shape and np.isfinite(s).all() and np.abs(s).max() > 0
    assert np.array_equal(f.view(np.uint32), s.view(np.uint32)), f'{int((f.view(np.uint32) != s.view(np.uint32)).sum())} gradient values differ'
    assert not np.array_equal(s[0], s[2]) and not np.array_equal(s[1], s[3])          # the steps really had different gradients
