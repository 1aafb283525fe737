"""GPU: one handle, many batch sizes -- the trainers' pattern (trainers/AEMODEL.py: process feeds whatever next_batch returns into a handle created at
max_batch = batchsize: full batches, then the epoch's ragged tail).  uad_create sizes the slab workspace, the filter-gradient slabs and the column
partials at max_batch while uad_forward plans at n, and the arrival counters of the in-kernel slab reduction, the slabs, the bottleneck's sibling
exchange and the compressed loss gradient persist between calls.  So, per architecture, ONE handle at the trainer's size is stepped through a batch
sequence, in 'f32', 'bf16x3' and 'bf16x6', and

* every step is held to the fp64 oracle as in tests/test_gpu_shapes.py (tests/step_parity.py: flip-aware, 1e-4 / 1e-4 / 1e-5 on reconstruction,
  scalars and every gradient tensor);
* no state leaks between steps: two back-to-back steps at the same n on the same inputs leave bit-identical reconstruction, scalars and gradients
  (run-to-run determinism, established first), and, given that, every later step at a batch size seen before is bit-identical to the first one;
* the VAE sequence is driven through the training entry too (forward + backward + optimizer step in one call, lr = 0 so the parameters stay) and its
  gradients are held to the oracle at the same bars;
* test_buffers_sized_at_max_batch_hold_every_smaller_plan checks on the host (uad_debug_plan: nothing is launched) that for every n <= max_batch no
  plan asks for more slab workspace, filter-gradient slab or column-partial floats than uad_create allocated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

try:
    from tests.step_parity import MODES, REUSE_CASES, check_capacity, make_engine, step
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
except Exception:
    make_engine = None


def test_vae_sequence_through_the_training_entry():
    """The same VAE sequence through train_step (uad_forward + uad_backward(UAD_SEG_ALL) + uad_adam_step -- the three calls the exported uad_train_step
    issues, and nothing else: in this library the training entry has NO kernel path of its own.  The compressed loss gradient and the deferred slab
    reductions already run in every want_backward forward + backward of a split-bf16 mode, so beyond test_batch_sequence_on_one_handle this leg adds only the
    optimizer launch and the weight repack on the side stream BETWEEN steps of different batch sizes) with lr = 0.
    The pattern cannot be read between the forward and the backward of one call, so each batch size first runs as forward + backward (held to the oracle,
    pattern read): the training step's forward has to leave the same bits -- then it took the same pattern -- and its gradients are held to the oracle
    differentiated with that pattern.  Bit-equality of the two legs' gradients is printed, not asserted."""
    arch, h, max_batch, seq = REUSE_CASES[0]
    assert arch == 'VAE'
    eng = make_engine(arch, h, max_batch)
    p32 = step(arch, h, seq[0]).p32
    eng.set_params(p32)
    names = [nm for nm, _, _ in eng.spec]
    flat0 = eng.get_buffer_host(_lib.BUF_PARAMS).copy()
    for math in MODES:
        eng.set_math(math)
        ref = {}
        for n in sorted(set(seq), reverse=True):
            ref[n] = step(arch, h, n, keep=len(set(seq)) + 1).run(eng, math, leg='fwd+bwd')
        for k, n in enumerate(seq):
            s = step(arch, h, n, keep=len(set(seq)) + 1)
            got = s.train_step(eng, lr=0.0)
            torch.cuda.synchronize()
            s.check_forward(got, math)
            assert torch.equal(got['x_hat'], ref[n].bits['x_hat']) and torch.equal(got['scalars'], ref[n].bits['scalars']), \
                f'{math} step {k} (n = {n}): the training step\'s forward differs from the forward + backward leg\'s'
            worst = s.check_grads(eng.get_grads(), ref[n].g, names, math, ref[n].flips)
            w = max(worst, key=worst.get)
            print(f'[VAE train_step {math} step {k} n={n}] worst gradient tensor {w}: {worst[w]:.2e}; gradients bit-identical to the forward + backward leg: '
                  f'{bool(torch.equal(eng.buffer(_lib.BUF_GRADS), ref[n].bits["grads"]))}')
    assert np.array_equal(eng.get_buffer_host(_lib.BUF_PARAMS), flat0), 'lr = 0 moved the parameters'
    eng.close()


@pytest.mark.parametrize('arch,h,max_batch,seq', REUSE_CASES, ids=[f'{a}-{h}-mb{mb}' for a, h, mb, _ in REUSE_CASES])
def test_batch_sequence_on_one_handle(arch, h, max_batch, seq):
    eng = make_engine(arch, h, max_batch)
    eng.set_params(step(arch, h, seq[0]).p32)
    for math in MODES:
        eng.set_math(math)
        # run-to-run determinism at the first batch size: the premise of the bit comparisons below
        s0 = step(arch, h, seq[0], keep=len(set(seq)) + 1)
        first = {seq[0]: s0.run(eng, math, leg='step 0')}
        again = s0.run(eng, math, leg='step 0 again', grads_like=first[seq[0]])
        same = again.same_bits(first[seq[0]])
        print(f'[{arch} {h}x{h} max_batch {max_batch} {math}] back-to-back steps at n = {seq[0]} bit-identical: {same}')
        assert all(same.values()), f'{math}: two back-to-back steps at n = {seq[0]} differ: {same}'
        for k, n in enumerate(seq[1:], 1):
            r = step(arch, h, n, keep=len(set(seq)) + 1).run(eng, math, leg=f'step {k}', grads_like=first.get(n))
            if n in first:
                same = r.same_bits(first[n])
                assert all(same.values()), f'{math}: step {k} (n = {n}) differs from the first step at that batch size -- state left by the steps between: {same}'
            else:
                first[n] = r
    eng.close()


# handles whose max_batch is NOT where the split counts peak (the k5 filter gradient's split count is not monotone in the batch: choose_w5 gives enc1 of a
# 128 x 128 handle 136 slabs at 17 slices and 256 at 16), next to the four the sequences above run on
SIZING_HANDLES = [(a, h, mb) for a, h, mb, _ in REUSE_CASES] + [('VAE', 128, 17), ('VAE', 128, 24), ('VAE', 64, 70), ('ceVAE', 128, 9), ('AE', 256, 5), ('VAE', 32, 100)]


@pytest.mark.parametrize('arch,h,max_batch', SIZING_HANDLES, ids=[f'{a}-{h}-mb{mb}' for a, h, mb in SIZING_HANDLES])
def test_buffers_sized_at_max_batch_hold_every_smaller_plan(arch, h, max_batch):
    """Host arithmetic only (a handle is created, nothing is launched): for n = 1 .. max_batch and every planned block, the slab-workspace floats, the
    filter-gradient slab floats and the column-partial floats the plan at N = n asks for fit what uad_create allocated.  The check can fail: against
    halved capacities it has to."""
    eng = make_engine(arch, h, max_batch)
    for math in MODES:
        eng.set_math(math)
        for n in range(1, max_batch + 1):
            check_capacity(eng, n)
    # the filter-gradient slab check on its own (the workspace check is not involved): at some n a plan needs the whole allocation, so half of it is too little
    with pytest.raises(AssertionError, match='filter-gradient slab floats') as e_w:
        for n in range(1, max_batch + 1):
            check_capacity(eng, n, shrink=2, kinds='W')
    print(f'\n[halved capacity] {e_w.value}')
    eng.close()
