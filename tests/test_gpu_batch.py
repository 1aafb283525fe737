"""GPU: uad_brain_boxes / uad_brain_boxes_f32 and uad_assemble_batch (csrc/uad_batch.hip) through DeviceOps on the case builders of
tests/batch_cases.py -- boxes equal to np.argwhere's, masking bit-equal to batch * mask, the noise bit-equal to uad_rng_fill's own numbers and
held to oracle.rng.normal -- then rank invariance, DeviceDataset's instance_noise and last_boxes, and one ceVAE and one CE epoch whose device
route must end with the bits of the host route (trainers/CE.py: masked_shard)."""
import random

import numpy as np
import pytest
import torch

from tests import batch_cases as bc

pytestmark = pytest.mark.gpu

try:
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.engine import rng_fill
    from unsupervised_anomaly_detection_brain_mri_amd.models import autoencoder, context_encoder_variational_autoencoder
    from unsupervised_anomaly_detection_brain_mri_amd.trainers import CE, Phase, ceVAE
    from unsupervised_anomaly_detection_brain_mri_amd.utils import slice_cache as sc
    from unsupervised_anomaly_detection_brain_mri_amd.utils.default_config_setup import get_config, get_options
    from unsupervised_anomaly_detection_brain_mri_amd.utils.synthetic import synthetic_slices
except Exception:
    pass


@pytest.fixture(scope='module')
def ops():
    return DeviceOps()


@pytest.mark.parametrize('shape', bc.BOX_SHAPES, ids=bc.shape_id)
def test_brain_boxes_equal_argwhere(ops, shape):
    for lut_kind in (None, 'brain', 'random'):
        labels, lut, want = bc.label_store(shape, lut_kind)
        ref = bc.boxes_reference(want)
        assert np.array_equal(ops.brain_boxes(labels, lut).cpu().numpy(), ref), lut_kind
        # a store whose base is 1, 2, 3 bytes off its alignment: a view into a larger device buffer
        flat = torch.from_numpy(labels.reshape(-1))
        for off in (1, 2, 3):
            buf = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device=ops.device)
            buf[off:off + flat.numel()] = flat.to(ops.device)
            view = buf[off:off + flat.numel()].view(labels.shape)
            assert view.data_ptr() % 16 == off
            assert np.array_equal(ops.brain_boxes(view, lut).cpu().numpy(), ref), (lut_kind, off)
    masks, want = bc.f32_masks(shape)
    got = ops.brain_boxes(masks)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), bc.boxes_reference(want))


@pytest.mark.parametrize('n', [1, 3, 64])
@pytest.mark.parametrize('shape', bc.ASM_SHAPES, ids=bc.shape_id)
def test_assemble_batch_gathers_and_masks_the_words(ops, shape, n):
    N = max(n, 5)
    src = bc.source(N, shape, seed=n)
    src_d = torch.from_numpy(src).to(ops.device)
    rects = bc.rects_case('mixed', n, shape)
    assert bc.masks_something(rects, shape)
    for kind in ('perm', 'repeat') + ((None,) if n == N else ()):
        idx = bc.index_case(kind, N, n)
        want_x, want_ce, _ = bc.assemble_reference(src, idx, rects)
        x, ce = ops.assemble_batch(src_d, idx, rects)
        assert bc.same_bits(x.cpu().numpy(), want_x), kind
        assert bc.same_bits(ce.cpu().numpy(), want_ce), kind
        x2, ce2 = ops.assemble_batch(src_d, idx, rects, want_x=False)
        assert x2 is None and torch.equal(ce2.view(torch.int32), ce.view(torch.int32))
    got = ops.context_mask(src_d[:n], torch.from_numpy(rects).to(ops.device))          # a device table
    assert bc.same_bits(got.cpu().numpy(), bc.assemble_reference(src[:n], None, rects)[1])
    none = bc.rects_case('none', n, shape)                                               # the named no-window case
    assert bc.same_bits(ops.context_mask(src_d[:n], none).cpu().numpy(), bc.assemble_reference(src[:n], None, none)[1])


@pytest.mark.parametrize('sigma', [0.01, 1.0])
def test_assemble_batch_noise_is_rng_fills(ops, sigma):
    shape, n, N = (26, 30, 1), 8, 11
    src = bc.source(N, shape, seed=2, special=False)
    src_d = torch.from_numpy(src).to(ops.device)
    idx = bc.index_case('repeat', N, n)
    rects = bc.rects_case('mixed', n, shape)
    assert bc.masks_something(rects, shape)
    seed, step, s0 = 0x1234567890ABCDEF, (1 << 33) + 17, 40
    # rng_fill numbers its jobs 0, 1, 2, ...: the third job is stream id 2
    fill = rng_fill([('a', shape, 'normal', 0.0), ('b', shape, 'normal', 0.0), ('c', shape, 'normal', 0.0)], n, seed, step, s0, device=ops.device)['c']
    noise = (sigma, seed, step, s0, 2)
    x, ce = ops.assemble_batch(src_d, idx, rects, noise)
    gathered = src_d[torch.from_numpy(idx).long().to(ops.device)]
    term = fill * torch.tensor(sigma, dtype=torch.float32, device=ops.device)            # multiply, then add: two fp32 ops
    want = gathered + term
    assert torch.equal(x.view(torch.int32), want.view(torch.int32))
    mask = torch.from_numpy(bc.rect_masks(rects, shape)).to(ops.device)
    assert torch.equal(ce.view(torch.int32), (x * mask).view(torch.int32))
    ref = bc.noise_reference(n, shape, noise)
    g = gathered.cpu().numpy()
    err = np.abs(x.cpu().numpy().astype(np.float64) - (g.astype(np.float64) + np.float64(np.float32(sigma)) * ref.astype(np.float64)))
    bound = bc.noise_bound(g, ref, sigma)
    print(f'assemble noise sigma {sigma}: max err {err.max():.3e}, worst ratio to the bound {(err / bound).max():.3f}')
    assert (err <= bound).all()
    # rank invariance: one call of 8 = two calls of 4 with sample0 = 40, 44; a repeated call repeats its bits
    xa, _ = ops.assemble_batch(src_d, idx[:4], rects[:4], noise)
    xb, _ = ops.assemble_batch(src_d, idx[4:], rects[4:], (sigma, seed, step, s0 + 4, 2))
    assert torch.equal(torch.cat([xa, xb]).view(torch.int32), x.view(torch.int32))
    again, _ = ops.assemble_batch(src_d, idx, rects, noise)
    assert torch.equal(again.view(torch.int32), x.view(torch.int32))
    other, _ = ops.assemble_batch(src_d, idx, rects, (sigma, seed, step + 1, s0, 2))
    assert not torch.equal(other, x)


def test_bad_arguments_raise(ops):
    shape = (26, 30, 1)
    src = torch.from_numpy(bc.source(4, shape)).to(ops.device)
    ok = bc.rects_case('mixed', 4, shape)
    outside = ok.copy()
    outside[2, 0] = (10, 15, 20, 20)                                 # leaves the slice on the right
    for bad in (outside, ok[:3], ok.reshape(4, 12)):
        with pytest.raises(ValueError):
            ops.context_mask(src, bad)
    with pytest.raises(ValueError):
        ops.assemble_batch(src, noise=(-0.5, 0, 0, 0, 0))
    with pytest.raises(ValueError):
        ops.assemble_batch(src, index=[0, 4])
    with pytest.raises(ValueError):
        ops.assemble_batch(src, want_x=False)
    with pytest.raises(ValueError):
        ops.assemble_batch(src[:, :, :29])                           # 26 * 29 elements: not a multiple of 4
    with pytest.raises(ValueError):
        ops.brain_boxes(np.zeros((2, 4, 4), np.float32), lut=np.ones(256, np.uint8))
    # the entry point's own checks
    import ctypes as C
    out = torch.empty_like(src)
    st = ops._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert ops.lib.uad_assemble_batch(p(src), None, 4, 26, 30, 1, None, -1.0, 0, 0, 0, 0, p(out), None, st) == 1
    assert ops.lib.uad_assemble_batch(p(src), None, 4, 26, 30, 1, None, 0.0, 0, 0, 0, 0, None, None, st) == 1
    assert ops.lib.uad_assemble_batch(p(src), None, 4, 26, 29, 1, None, 0.0, 0, 0, 0, 0, p(out), None, st) == 1
    assert ops.lib.uad_assemble_batch(p(src), None, 0, 26, 30, 1, None, 0.0, 0, 0, 0, 0, p(out), None, st) == 1
    assert ops.lib.uad_brain_boxes(None, 1, 4, 4, None, p(out), st) == 1
    ds = sc.DeviceDataset(synthetic_slices(8, 32, 32, seed=0), np.zeros(8, int))
    ds.next_batch(4)
    with pytest.raises(ValueError, match='no label maps'):
        ds.last_boxes()
    with pytest.raises(ValueError, match='no label maps'):
        ds.brain_boxes('TRAIN')


# ---------------------------------------------------------------------------------------------------------------- DeviceDataset
def _labelled(n, h, seed=0):
    """Synthetic slices with a tissue-class map: a brain (labels 1 .. 3) ellipse of random size and position on skull / background."""
    rng = np.random.default_rng(seed)
    imgs = synthetic_slices(n, h, h, seed=seed)
    yy, xx = np.mgrid[:h, :h]
    labs = np.zeros((n, h, h), np.uint8)
    for i in range(n):
        cy, cx = rng.integers(h // 2 - 4, h // 2 + 5, 2)
        ry, rx = rng.integers(h // 4, h // 2 - 5, 2)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        labs[i] = np.where(inside, rng.integers(1, 4, (h, h)), rng.choice([0, 7], (h, h))).astype(np.uint8)
    return imgs, labs


def test_device_dataset_instance_noise_and_boxes():
    imgs, labs = _labelled(20, 32, seed=3)
    sets = np.array([0] * 12 + [1] * 8)
    plain, kw0 = sc.DeviceDataset(imgs, sets, labs, seed=5), sc.DeviceDataset(imgs, sets, labs, seed=5, instance_noise=0.0)
    a, b = sc.DeviceDataset(imgs, sets, labs, seed=5, instance_noise=0.01), sc.DeviceDataset(imgs, sets, labs, seed=5, instance_noise=0.01)
    lut = sc.brainmask_lut()
    prev = None
    for step in range(4):                                            # crosses the epoch boundary of the TRAIN split
        x0, _, m0 = plain.next_batch(8, return_brainmask=True)
        assert torch.equal(kw0.next_batch(8)[0].view(torch.int32), x0.view(torch.int32))
        xa, xb = a.next_batch(8)[0], b.next_batch(8)[0]
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))                       # the same seed: the same noise
        ref = bc.noise_reference(8, (32, 32, 1), (0.01, 5, step, 0, sc.DeviceDataset.NOISE_STREAM))
        g = x0.cpu().numpy()
        err = np.abs(xa.cpu().numpy().astype(np.float64) - (g.astype(np.float64) + np.float64(np.float32(0.01)) * ref.astype(np.float64)))
        assert (err <= bc.noise_bound(g, ref, 0.01)).all()
        assert prev is None or not torch.equal(xa - x0, prev)                                # consecutive batches: other numbers
        prev = xa - x0
        # the boxes of the batch = np.argwhere boxes of its host brain masks
        rows = plain._keep_host
        want = bc.boxes_reference(lut[labs[rows]] != 0)
        assert np.array_equal(plain.last_boxes(), want) and np.array_equal(a.last_boxes(), want)
        assert np.array_equal(bc.boxes_reference(m0.cpu().numpy() != 0), want)
    # VAL has a step counter of its own, starting at 0
    v = a.next_batch(4, set='VAL')[0]
    g = plain.next_batch(4, set='VAL')[0].cpu().numpy()
    ref = bc.noise_reference(4, (32, 32, 1), (0.01, 5, 0, 0, sc.DeviceDataset.NOISE_STREAM))
    assert (np.abs(v.cpu().numpy().astype(np.float64) - (g.astype(np.float64) + np.float64(np.float32(0.01)) * ref)) <= bc.noise_bound(g, ref, 0.01)).all()
    assert np.array_equal(a.brain_boxes('VAL'), bc.boxes_reference(lut[labs[12:]] != 0)) and a.brain_boxes().shape == (20, 4)


# ---------------------------------------------------------------------------------------------------------------- trainers
def _epoch(trainer_cls, network, tmp_path, host_route, per_sample=False):
    imgs, labs = _labelled(12, 64, seed=1)
    ds = sc.DeviceDataset(imgs, np.zeros(12, int), labs, seed=2)
    opt = get_options(batchsize=4, learningrate=1e-3, numEpochs=1, zDim=64, outputWidth=64, outputHeight=64,
                      config={'CHECKPOINTDIR': str(tmp_path / 'ck'), 'SAMPLEDIR': str(tmp_path / 'smp')})
    cfg = get_config(trainer_cls, opt, 'ADAM', [8, 8], 0.2, ds)
    cfg.contextMaskPerSample = per_sample
    model = trainer_cls(None, cfg, network=network, seed=11)
    model.mask_rng = random.Random(5)
    model.host_context_mask = host_route
    out = model.process(ds, 0, Phase.TRAIN)
    params = model.engine.get_buffer_host().copy()
    state = model.mask_rng.getstate()
    model.engine.close()
    return params, out, state


@pytest.mark.parametrize('which', ['ceVAE', 'CE'])
def test_the_device_route_trains_the_bits_of_the_host_route(which, tmp_path):
    trainer_cls, network = (ceVAE, context_encoder_variational_autoencoder) if which == 'ceVAE' else (CE, autoencoder)
    p_host, s_host, r_host = _epoch(trainer_cls, network, tmp_path, host_route=True)
    p_dev, s_dev, r_dev = _epoch(trainer_cls, network, tmp_path, host_route=False)
    assert np.isfinite(p_dev).all() and set(s_dev) == set(s_host)
    assert np.array_equal(p_host.view(np.uint32), p_dev.view(np.uint32))
    assert all(np.float32(s_host[k]).tobytes() == np.float32(s_dev[k]).tobytes() for k in s_host)
    assert r_host == r_dev                                           # the same draws on both routes
    # per-sample masks (config.contextMaskPerSample): runs, draws the same numbers, and trains something else than the last sample's mask for all
    p_per, s_per, r_per = _epoch(trainer_cls, network, tmp_path, host_route=False, per_sample=True)
    assert np.isfinite(p_per).all() and r_per == r_dev and not np.array_equal(p_per, p_dev)
    p_per_host = _epoch(trainer_cls, network, tmp_path, host_route=True, per_sample=True)[0]
    assert np.array_equal(p_per_host.view(np.uint32), p_per.view(np.uint32))
