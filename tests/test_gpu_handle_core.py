"""The handle core both engines build on (csrc/uad_handle.h): the tensor table, the flat-buffer round trips, and above all that every way of
writing parameters -- set_buffer, the raw buffer(PARAMS) pointer, a math-mode switch -- leaves the next run on packs of the NEW parameters.
One AE-family handle (uad_*) and one GAN-family handle (uad_gan_*, the AnoVAE-GAN variant: it has the second Adam slots), each at the
smallest configuration tests/test_gpu_model.py and tests/test_gpu_fanogan.py create.  Outputs are compared bit for bit with a fresh handle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    from unsupervised_anomaly_detection_brain_mri_amd.engine import Engine
    from unsupervised_anomaly_detection_brain_mri_amd.gan_engine import GanEngine
except Exception:
    Engine = None

H, INTER, ZDIM, N = 32, 8, 16, 2
UAD_ERR_INVALID = 1
HANDLES = ['vae', 'anovaegan']
_RNG = np.random.default_rng(7)
X = _RNG.random((N, H, H, 1), dtype=np.float32)
EPS = _RNG.standard_normal((N, ZDIM)).astype(np.float32)


def _make(kind, math='f32'):
    if kind == 'vae':
        return Engine('VAE', H, H, 1, INTER, ZDIM, max_batch=N, math=math)
    return GanEngine(H, H, 1, INTER, ZDIM, max_batch=N, scale=10.0, math=math, variant='anovaegan', kl_weight=0.8)


def _buffers(kind):
    common = [_lib.BUF_PARAMS, _lib.BUF_GRADS, _lib.BUF_ADAM_M, _lib.BUF_ADAM_V]
    return common + ([_lib.BUF_ADAM_M2, _lib.BUF_ADAM_V2] if kind == 'anovaegan' else [])


def _vector(eng, seed):
    """A seeded parameter vector: small kernels, scales near one -- every layer stays finite and far from saturation."""
    rng = np.random.default_rng(seed)
    p = (0.05 * rng.standard_normal(eng.nparams)).astype(np.float32)
    for name, shape, off in eng.spec:
        if name.endswith('/gamma'):
            p[off:off + int(np.prod(shape))] += 1.0
    return p


def _run(eng, kind):
    """The bits of a run without backward: every packed 5x5 kernel of the encoder and the decoder / generator is read."""
    if kind == 'vae':
        out = eng.forward(X, EPS, want_backward=False)['x_hat']
    else:
        out = eng.reconstruct(X, eps=EPS)['reconstruction']
    bits = out.cpu().numpy().view(np.uint32).copy()
    assert np.isfinite(bits.view(np.float32)).all()
    return bits


@functools.lru_cache(maxsize=None)
def _fresh(kind, math, seed, switch_to=None):
    """The reference: a new handle that has only ever seen this parameter vector (computed once per case, shared by the tests)."""
    eng = _make(kind, math)
    eng.set_params(_vector(eng, seed))
    if switch_to:
        eng.set_math(switch_to)
    bits = _run(eng, kind)
    eng.close()
    return bits


@pytest.mark.parametrize('kind', HANDLES)
def test_tensor_table_tiles_the_flat_buffer(kind):
    eng = _make(kind)
    assert sum(int(np.prod(s)) for _, s, _ in eng.spec) == eng.nparams == int(eng._fn('param_count')(eng.handle))
    end = 0
    for _, shape, off in sorted(eng.spec, key=lambda t: t[2]):
        assert off == end
        end = off + int(np.prod(shape))
    assert end == eng.nparams
    off, rank, shape = C.c_longlong(), C.c_int(), (C.c_int * 4)()
    for idx in (-1, len(eng.spec)):
        assert eng._fn('tensor_info')(eng.handle, idx, None, 0, C.byref(off), C.byref(rank), shape) == UAD_ERR_INVALID
        assert b'out of range' in eng.lib.uad_last_error()
    eng.close()


@pytest.mark.parametrize('kind', HANDLES)
def test_buffer_round_trip_and_count_check(kind):
    eng = _make(kind)
    rng = np.random.default_rng(11)
    sent = {}
    for which in _buffers(kind):         # all written first, then all read: no buffer aliases another
        sent[which] = rng.standard_normal(eng.nparams).astype(np.float32)
        eng.set_buffer_host(which, sent[which])
    for which in _buffers(kind):
        assert np.array_equal(eng.get_buffer_host(which).view(np.uint32), sent[which].view(np.uint32)), which
    host = np.zeros(eng.nparams + 1, np.float32)
    for fn in ('set_buffer', 'get_buffer'):
        for count in (eng.nparams - 1, eng.nparams + 1):
            assert eng._fn(fn)(eng.handle, _lib.BUF_PARAMS, host.ctypes.data_as(C.c_void_p), count) == UAD_ERR_INVALID
            assert f'expected {eng.nparams}'.encode() in eng.lib.uad_last_error()
    if kind == 'vae':                    # a handle without the second slots refuses them
        assert eng._fn('get_buffer')(eng.handle, _lib.BUF_ADAM_M2, host.ctypes.data_as(C.c_void_p), eng.nparams) == UAD_ERR_INVALID
    eng.close()


@pytest.mark.parametrize('write', ['set_buffer', 'raw_pointer', 'set_buffer_then_get_buffer'])
@pytest.mark.parametrize('math', ['f32', 'bf16x3'])
@pytest.mark.parametrize('kind', HANDLES)
def test_a_parameter_write_invalidates_the_packs(kind, math, write):
    a = _make(kind, math)
    p1, p2 = _vector(a, 1), _vector(a, 2)
    a.set_params(p1)
    first = _run(a, kind)                # packs of p1 are now valid
    if write == 'raw_pointer':
        a.buffer(_lib.BUF_PARAMS, write=True).copy_(torch.from_numpy(p2))
    else:
        a.set_params(p2)
    if write == 'set_buffer_then_get_buffer':      # a read in between (checkpoint save) must not mark the stale packs valid
        assert np.array_equal(a.get_buffer_host(_lib.BUF_PARAMS), p2)
    second = _run(a, kind)
    a.close()
    assert not np.array_equal(first, second)
    assert np.array_equal(second, _fresh(kind, math, 2))


@pytest.mark.parametrize('math,to', [('f32', 'bf16x3'), ('bf16x3', 'f32')])
@pytest.mark.parametrize('kind', HANDLES)
def test_a_math_mode_switch_repacks(kind, math, to):
    a = _make(kind, math)
    p = _vector(a, 3)
    a.set_params(p)
    _run(a, kind)                        # packs of the first mode are valid
    a.set_math(to)
    got = _run(a, kind)
    a.close()
    assert np.array_equal(got, _fresh(kind, math, 3, switch_to=to))
