"""`ResidentDataset`: a training set uploaded once into device pools; iterating it plans one epoch of `_batches.ResidentBatch`
objects on the host (`_samplers`).  The only module of the input side that owns device memory, and only from the first write on: the
device context is imported inside `_allocate`.  `datacoder` re-exports the name.
"""
from typing import Optional

import numpy as np

from ._batches import GMAX, CompactBatch, ResidentBatch, pad_ground_truth
from ._samplers import _MOSAIC_KEYS, _epoch_plan, _random_mosaics, _split_crop_options, random_crop_windows, random_mosaic


class ResidentDataset:
    """A training set kept in device memory as the files hold it -- uint8 pixels, uint8 class indices, ground-truth rows: 1.2 MB per
    480x640 sample -- uploaded once.  Iterating it is ONE EPOCH of the reference's chain (NB03#cell8:
    `.shuffle(len).map(read_and_encode).batch(B).map(augmentation_rgb_channels)`): a new permutation of the samples, a new flip
    draw per sample when `encoder.augmentation_horizontal_flip`, one colour draw set per batch when `rgb_augmentation`, the last
    partial batch kept unless `drop_remainder` -- all from the dataset's own Generator(seed); TF's RNG streams are not reproduced.
    The batches are `ResidentBatch` objects: `Model.fit(ds, epochs=N)` builds each one on the device (ssdseg_gather_inputs,
    ssdseg_gather_gt, ssdseg_encode_targets), so after the upload no pixel crosses PCIe and the host does no per-sample work.
    `samples`: an iterable of `read_compact` tuples (their flip flag is ignored); `capacity`: slots to allocate (default: the number
    of samples), filled with `append` / `write` without holding the set on the host.
    `random_crop`: None (the chain above, nothing else drawn), or a dict of random_crop_windows' keywords plus optional `fill` (r, g,
    b) / `fill_class`: every batch then carries one crop window per sample, drawn from the same Generator AFTER the epoch's
    permutation, flips and colour draws, and the device crops before it flips and colours (ssdseg_crop_inputs, ssdseg_crop_gt).
    `mosaic`: None, or a dict of random_mosaic's keywords plus optional `fill` / `fill_class`: every batch then carries a Mosaic over
    its own samples, drawn from the same Generator AFTER the epoch's plan likewise, and the device assembles each image from four
    samples of the batch in the crop's place (ssdseg_mosaic_inputs, ssdseg_mosaic_gt).  Not together with `random_crop`.
    In both, fill_class=255 (any index >= 4) is the void fill: what lies outside the samples gets all-zero one-hot rows, which
    `cross_entropy` ignores as it stands and the other mask losses and the mask metric ignore with `ignore_void=True`."""

    GMAX = GMAX     # ground-truth rows per sample, the loaders' own

    def __init__(self, encoder, samples=None, *, capacity: Optional[int] = None, batch_size: int = 16, shuffle: bool = True,
                 rgb_augmentation: bool = False, drop_remainder: bool = False, seed=None, random_crop=None, mosaic=None):
        samples = list(samples) if samples is not None else []
        capacity = len(samples) if capacity is None else int(capacity)
        if capacity <= 0 or capacity < len(samples):
            raise ValueError(f"resident dataset: capacity {capacity} for {len(samples)} samples")
        if int(batch_size) <= 0:
            raise ValueError("resident dataset: batch_size must be positive")
        self.encoder = encoder
        self.capacity, self.batch_size = capacity, int(batch_size)
        self.shuffle, self.rgb_augmentation, self.drop_remainder = bool(shuffle), bool(rgb_augmentation), bool(drop_remainder)
        self.height, self.width = int(encoder.image_height), int(encoder.image_width)
        self.random_crop = None
        if random_crop is not None:
            self.random_crop = _split_crop_options(random_crop)
            random_crop_windows(np.random.default_rng(0), 1, self.height, self.width, **self.random_crop[0])      # bad options fail here
        self.mosaic = None
        if mosaic is not None:
            if random_crop is not None:
                raise ValueError("resident dataset: random_crop or mosaic, not both")
            self.mosaic = _split_crop_options(mosaic, "mosaic", _MOSAIC_KEYS)
            random_mosaic(np.random.default_rng(0), 1, self.height, self.width, **self.mosaic[0])                # bad options fail here
        self.num_samples = 0
        self._rng = np.random.default_rng(seed)
        self.ctx = self.images = self.masks = self.gt = self.cnt = None
        self._gt_labels = {}      # slot -> the labels of its ground-truth rows (int32): what evaluation counts per class on the host
        for sample in samples:
            self.append(*sample[:3])

    def _allocate(self) -> None:
        """the four pools, on the first write (planning an epoch needs no device)"""
        from . import _engine
        self.ctx = ctx = _engine.default_context()
        self.images = ctx.empty((self.capacity, self.height, self.width, 3), np.uint8)
        self.masks = ctx.empty((self.capacity, self.height, self.width), np.uint8)
        self.gt = ctx.empty((self.capacity, self.GMAX, 5))
        self.cnt = ctx.empty(self.capacity, np.int32)

    def write(self, slot: int, image_u8, mask_u8, gt) -> None:
        """sample `slot` <- (uint8 image (H, W, 3), uint8 class-index mask (H, W), ground truth (G, 5)); slots up to the highest one
        written count as samples"""
        slot = int(slot)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"resident dataset: slot {slot} outside [0, {self.capacity})")
        image = np.ascontiguousarray(image_u8, np.uint8)
        mask = np.ascontiguousarray(mask_u8, np.uint8)
        if image.shape != (self.height, self.width, 3) or mask.shape != (self.height, self.width):
            raise ValueError(f"resident dataset: image {image.shape} / mask {mask.shape} for samples of {self.height}x{self.width}")
        g = np.asarray(gt, np.float32).reshape(-1, 5)
        if g.shape[0] > self.GMAX:
            raise ValueError(f"more than {self.GMAX} ground-truth boxes in one image")
        rows, cnt = pad_ground_truth([g], self.GMAX)
        if self.images is None:
            self._allocate()
        hw = self.height * self.width
        self.images.view(slot * hw * 3, image.shape).upload(image)
        self.masks.view(slot * hw, mask.shape).upload(mask)
        self.gt.view(slot * self.GMAX * 5, rows[0].shape).upload(rows[0])
        self.cnt.view(slot, (1,)).upload(cnt)
        self._gt_labels[slot] = g[:, 0].astype(np.int32)
        self.num_samples = max(self.num_samples, slot + 1)

    def append(self, image_u8, mask_u8, gt) -> int:
        slot = self.num_samples
        self.write(slot, image_u8, mask_u8, gt)
        return slot

    def __len__(self):
        """batches per epoch"""
        n, b = self.num_samples, self.batch_size
        return n // b if self.drop_remainder else -(-n // b)

    def batch(self, index, flip=None, rgb_draws=None, **geometric) -> ResidentBatch:
        """an explicit batch: these samples, seen through these crop windows or assembled by this mosaic (ResidentBatch's keywords),
        mirrored where flagged, with these colour draws"""
        return ResidentBatch(self, index, flip, rgb_draws, **geometric)

    def __iter__(self):
        plan = _epoch_plan(self._rng, self.num_samples, self.batch_size, self.shuffle, bool(self.encoder.augmentation_horizontal_flip),
                           self.rgb_augmentation, self.drop_remainder)
        # the geometric step of every batch is drawn after the WHOLE plan: the plan's draws are those of a dataset without one
        geometric = [{}] * len(plan)
        if self.mosaic is not None and plan:        # one draw for the epoch's batches
            kw, fill = self.mosaic
            mosaics = _random_mosaics(self._rng, [len(index) for index, _, _ in plan], self.height, self.width, **kw)
            geometric = [dict(mosaic=mosaic, mosaic_fill=fill) for mosaic in mosaics]
        elif self.random_crop is not None:
            kw, fill = self.random_crop
            geometric = [dict(crop_windows=random_crop_windows(self._rng, len(index), self.height, self.width, **kw), crop_fill=fill)
                         for index, _, _ in plan]
        return iter([ResidentBatch(self, index, flip, draws, **step) for (index, flip, draws), step in zip(plan, geometric)])

    def to_compact(self, batch: ResidentBatch) -> CompactBatch:
        """the named samples downloaded into an equal CompactBatch (same windows or mosaic, same flips, same draws): for debugging and
        tests"""
        hw = self.height * self.width
        images = np.stack([self.images.view(int(i) * hw * 3, (self.height, self.width, 3)).download() for i in batch.index])
        masks = np.stack([self.masks.view(int(i) * hw, (self.height, self.width)).download() for i in batch.index])
        cnt = self.cnt.download()
        gts = [self.gt.view(int(i) * self.GMAX * 5, (self.GMAX, 5)).download()[:cnt[i]] for i in batch.index]
        flip = np.zeros(len(batch), np.uint8) if batch.flip is None else batch.flip.copy()
        return CompactBatch(images, masks, gts, flip, self.encoder, **batch.augment())
