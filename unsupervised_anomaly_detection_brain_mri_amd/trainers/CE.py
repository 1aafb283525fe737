"""trainers/CE.py — the context encoder: an autoencoder that READS the context-masked batch and is scored against the clean one
(CE.py:19-21,33-34,87-92), plus `retrieve_masked_batch` (CE.py:123-139), the host-side masking the ceVAE trainer imports too
(ceVAE.py:8,93), its draw alone (`draw_context_squares`) and `masked_shard`, which masks a device batch on the device.  On the device this is the AE handle with io.x_ce set (include/uad_hip.h): encoder input = x_ce, L1 target = x."""
import random as _random
from collections import defaultdict

import numpy as np

from .AE import AE
from .AEMODEL import Phase


SIDE = 20                      # CE.py:128: the squares are 20 x 20


def draw_context_squares(boxes, rng=None):
    """The draw of retrieve_masked_batch (CE.py:127-137) without the pixels: boxes [n,4] of (row_min, row_max, col_min, col_max), the brain
    bounding box of each sample, -> int32 [n,3,4] of (row, col, height, width) windows, height 0 = unused (the table of
    DeviceOps.context_mask).  rng.randint is consumed in the reference's order: one draw of the count (1 .. 3) per sample, then two draws per
    square and only when the box is larger than a square in both directions (r0 < r1 - 20 and c0 < c1 - 20); a square that does not fit
    draws nothing and leaves its slot unused.  A box of (-1,-1,-1,-1) -- an empty brain mask -- raises ValueError, as np.argwhere's min() does
    in the reference.  rng: object with randint(a, b), both ends inclusive; default the `random` module like the reference."""
    rng = _random if rng is None else rng
    boxes = np.asarray(boxes).reshape(-1, 4)
    if len(boxes) and int(boxes[:, 1].min()) < 0:
        raise ValueError(f'sample {int(np.argmax(boxes[:, 1] < 0))} has an empty brain mask: no bounding box to draw squares in')
    rects = np.zeros((len(boxes), 3, 4), np.int32)
    for i, (r0, r1, c0, c1) in enumerate(boxes.tolist()):
        for k in range(rng.randint(1, 3)):
            if r0 < r1 - SIDE and c0 < c1 - SIDE:
                r = rng.randint(r0, r1 - SIDE)
                c = rng.randint(c0, c1 - SIDE)
                rects[i, k] = (r, c, SIDE, SIDE)
    return rects


def squares_to_mask(rects, shape, dtype=np.float32):
    """[3,4] windows of one sample -> its [H,W,C] mask of `shape`: 0 inside a window, 1 elsewhere."""
    mask = np.ones(shape, dtype)
    for r, c, h, w in np.asarray(rects).tolist():
        if h:
            mask[r:r + h, c:c + w] = 0
    return mask


def retrieve_masked_batch(batch, brainmasks, rng=None, per_sample=False):
    """Zero 1-3 random 20x20 squares inside each slice's brain bounding box.

    Behaviour kept from the reference, defect included: the per-sample loop re-binds the name of the
    mask array, so what multiplies the batch at the end is the LAST sample's [H,W,C] mask, broadcast over all samples
    (the earlier samples' squares are drawn -- consuming RNG -- and then discarded).  per_sample=True (config.contextMaskPerSample)
    multiplies every sample by its own mask instead; the draws are the same.
    rng: object with randint(a, b), both ends inclusive; default the `random` module like the reference."""
    if hasattr(batch, 'cpu'):            # device tensors of utils.slice_cache.DeviceDataset: the masking RNG and geometry are host-side
        batch = batch.cpu().numpy()
    if hasattr(brainmasks, 'cpu'):
        brainmasks = brainmasks.cpu().numpy()
    batch = np.asarray(batch)
    boxes = []
    for bm in brainmasks:
        rows, cols = np.nonzero(np.asarray(bm).reshape(batch.shape[1], batch.shape[2], -1).any(axis=-1))
        boxes.append((int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())))
    rects = draw_context_squares(boxes, rng)
    if per_sample:
        return batch * np.stack([squares_to_mask(r, batch.shape[1:], batch.dtype) for r in rects])
    return batch * squares_to_mask(rects[-1], batch.shape[1:], batch.dtype)


def masked_shard(trainer, dataset, phase):
    """The next batch of this rank and its context-masked companion -> (batch, x_ce or None): the head of the process() loops of CE and ceVAE
    (CE.py:76-77, ceVAE.py:92-93).  The squares are drawn in every phase, so the host RNG stream does not depend on the route or the phase.
    Device route -- the dataset offers last_boxes() (utils.slice_cache.DeviceDataset) and trainer.host_context_mask is not set: the boxes of
    the shard come from the dataset's host table, the squares are drawn on the host, their 48 bytes a sample go up through the dataset's
    pinned staging ring without blocking, and engine.context_mask multiplies on the device -- no download of the batch or of the brain
    masks, no brain-mask gather, no host x_ce; VAL / TEST draw and do no device work (x_ce is unused there: None).  Defect A3 is the
    default on both routes: every sample is multiplied by the LAST sample's mask (the last row of this rank's shard, replicated);
    config.contextMaskPerSample = True hands each sample its own squares.  Host route: retrieve_masked_batch, as before."""
    rng = getattr(trainer, 'mask_rng', None)
    per_sample = bool(getattr(trainer.config, 'contextMaskPerSample', False))
    if hasattr(dataset, 'last_boxes') and not getattr(trainer, 'host_context_mask', False):
        batch = trainer._shard(dataset, phase)[0]
        if getattr(batch, 'is_cuda', False):
            lo = trainer.rank * len(batch) if getattr(getattr(trainer, 'dp', None), 'world', 1) > 1 else 0
            rects = draw_context_squares(dataset.last_boxes()[lo:lo + len(batch)], rng)
            if phase != Phase.TRAIN:
                return batch, None
            if not per_sample:
                rects = np.repeat(rects[-1:], len(rects), axis=0)
            return batch, trainer.engine.context_mask(batch, dataset.upload_int32(rects))
        raise TypeError('a dataset that offers last_boxes() must serve device batches')
    batch, _, brainmasks = trainer._shard(dataset, phase, return_brainmask=True)
    return batch, retrieve_masked_batch(batch, brainmasks, rng=rng, per_sample=per_sample)


class CE(AE):
    """loss = reconstructionLoss = mean_n sum |x - network(x_ce)| (CE.py:33-34).  TRAIN feeds the masked batch, VAL / reconstruct() feed
    x_ce = x (:91,112).  Accepts the AE-family networks (autoencoder, autoencoder_spatial): the trainer's loss has no KL term."""

    class Config(AE.Config):
        def __init__(self):            # CE.py:13-15
            super().__init__()
            self.model_name = self.modelname = 'CE'

    def step(self, batch, phase, *, x_ce=None, eps=None, dropout_masks=None, fetch_maps=True):
        phase = Phase(phase) if not isinstance(phase, Phase) else phase
        train = phase == Phase.TRAIN
        masks = self._noise(len(batch), dropout=train)[1] if dropout_masks is None else dropout_masks
        c = self.config
        if train:
            out = self.dp.train_step(batch, None, masks, lr=c.learningrate, beta1=c.beta1, want_l1=fetch_maps, x_ce=x_ce)
        else:
            out = self.engine.forward(batch, None, masks, want_backward=False, want_l1=fetch_maps, x_ce=x_ce)
        sc = self.dp.allreduce_scalars(out['scalars'].clone()).cpu().numpy()
        run = {'reconstructionLoss': np.float32(sc[0]), 'loss': np.float32(sc[0])}
        if fetch_maps:
            run['reconstruction'] = out['x_hat'].cpu().numpy()
            run['L1'] = out['L1'].cpu().numpy()
        return run

    def process(self, dataset, epoch, phase, optim=None):       # CE.py:70-101
        phase = Phase(phase) if not isinstance(phase, Phase) else phase
        scalars = defaultdict(list)
        num_batches = self._num_batches(dataset, phase)
        for idx in range(num_batches):
            batch, masked_batch = masked_shard(self, dataset, phase)      # drawn in every phase (:77), fed in TRAIN only (:91)
            run = self.step(batch, phase, x_ce=masked_batch if phase == Phase.TRAIN else None, fetch_maps=False)
            print(f'Epoch ({phase.value}): [{epoch:2d}] [{idx:4d}/{num_batches:4d}] loss: {run["loss"]:.8f}')
            for k, v in run.items():
                if np.ndim(v) == 0:
                    scalars[k].append(v)
        out = {k: np.mean(v) for k, v in scalars.items()}
        for k, v in out.items():
            self.curves.setdefault(f'{phase.value}/{k}', []).append(float(v))
        self.log_to_tensorboard(epoch, out, None, phase)
        return out
