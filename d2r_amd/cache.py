"""--cache_dataset device: the preprocessed dataset in device memory.

A sample's token ids, its label and its CLIP pixel values are pure functions of the files on disk
(processor/dataset.py:64-102), and the pixel values are a function of the cropped uint8 image and the channel alone
(d2r_amd.image).  So a split is decoded and resized once per run, whatever the format of its files, and every later batch is
built on the device from

  * ``crops``      uint8 [N, row_bytes]: the planar [3, S, S] crop of every image (150,528 bytes at S = 224), lossless;
  * ``input_ids``, ``input_mask``, ``segment_ids`` int64 [N, L] and ``labels`` int64 [N];
  * the constant ``img_mask`` row and the [3, 256] normalisation table.

``prefill`` makes one sequential pass over the split through the loader's own workers, collate function and packed-images device
path (either --image_decode mode) that ends in d2r_clip_preprocess_u8 with the dataset indices as slots.  ``CachedLoader`` then
stands in for the DataLoader: it draws the index batches from the original loader's batch_sampler, uploads them with one small
copy and yields the trainer's 6-tuple built by d2r_gather_rows / d2r_clip_cache_gather (five launches per batch), already on the
device.  It consumes torch's default generator exactly as the loader it replaces, and the prefill leaves that generator as it
found it: the dropout seeds come from it (functional._next_dropout_seed), so a run with the cache takes the very steps of a run
without.

The cache holds the un-augmented crops.  A training loader may carry an ``Augmenter`` (d2r_amd.augment, --aug_crop_scale /
--aug_flip): its batches' pixel values then come from d2r_clip_cache_augment, the same launch with a box and a flip per sample -
or, with a photometric option on (--aug_brightness / --aug_contrast / --aug_saturation / --aug_hue / --aug_grayscale / --aug_erase),
from d2r_clip_cache_augment_photo, which also jitters the colours, greys and erases per sample.  It may also carry a
``TokenAugmenter`` (d2r_amd.text_augment, --aug_token_delete / --aug_token_mask / --aug_token_replace): one d2r_token_augment launch
then takes the place of the three d2r_gather_rows of the token tensors and deletes, masks or replaces tokens on the way (K23).
"""
from __future__ import annotations

import logging
import time

import torch
from torch.utils.data import DataLoader, Dataset

from . import image as I
from .jpeg import DecodeLog, PackedJpegImages

_logger = logging.getLogger(__name__)


class IndexedImages:
    """The images element of a prefill batch: the collated packed images (PackedImages / PackedJpegImages), the dataset indices of
    the batch's samples (host int64 [B]) and how many of them fell back to inf.png.  The batch stays the trainer's 6-tuple."""

    def __init__(self, packed, indices: torch.Tensor, fallbacks: int):
        self.packed, self.indices, self.fallbacks = packed, indices, fallbacks

    def __len__(self):
        return int(self.indices.numel())

    def pin_memory(self, device=None):  # DataLoader(pin_memory=True) calls this in its pinning thread
        packed = self.packed.pin_memory() if hasattr(self.packed, "pin_memory") else self.packed
        return IndexedImages(packed, self.indices, self.fallbacks)


class _IndexedSamples(Dataset):
    """dataset[i] with i and the inf.png fallbacks that loading it cost appended (the workers' own counters never reach the parent)."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        before = getattr(self.dataset, "fallbacks", 0)
        sample = self.dataset[idx]
        return (*sample, idx, getattr(self.dataset, "fallbacks", 0) - before)


class _IndexedCollate:
    """The loader's collate function on the samples proper; the last element of its batch wrapped into IndexedImages."""

    def __init__(self, collate_fn):
        self.collate_fn = collate_fn

    def __call__(self, samples):
        batch = self.collate_fn([s[:-2] for s in samples])
        indices = torch.tensor([s[-2] for s in samples], dtype=torch.int64)
        return (*batch[:-1], IndexedImages(batch[-1], indices, sum(s[-1] for s in samples)))


def cache_bytes(n: int, max_seq: int, S: int) -> int:
    """Device bytes a split of n samples holds: crops, three [n, max_seq] int64 tensors, labels."""
    return n * (I.cache_row_bytes(S) + 3 * 8 * max_seq + 8)


def check_fit(needs, free: int) -> None:
    """needs: [(split, bytes)] in allocation order.  Exits, naming the split that no longer fits into `free` bytes."""
    total = 0
    for split, need in needs:
        total += need
        if total > free:
            raise SystemExit(f"--cache_dataset device: the {split} split needs {need} bytes of device memory ({total} bytes with the "
                             f"splits before it), {free} bytes are free; run without --cache_dataset")


class DeviceDatasetCache:
    """The device-resident tensors of one split (see the module docstring) and the two operations on them: ``fill`` (one prefill
    batch) and ``gather`` (one training batch by index)."""

    def __init__(self, n: int, max_seq: int, S: int, norm: tuple, device, split: str = "data", logger=None):
        if n < 1:
            raise ValueError(f"the {split} split is empty: nothing to cache")
        self.n, self.max_seq, self.S, self.split = n, max_seq, S, split
        self.device = torch.device(device)
        self.crops = torch.empty(n, I.cache_row_bytes(S), dtype=torch.uint8, device=self.device)
        self.input_ids, self.input_mask, self.segment_ids = (torch.empty(n, max_seq, dtype=torch.int64, device=self.device)
                                                             for _ in range(3))
        self.labels = torch.empty(n, dtype=torch.int64, device=self.device)
        self.norm = norm
        self.lut = I._device_table(str(self.device), norm)
        self.img_mask = None      # the constant row, [ntok] on the device, from the first batch
        self._h_img_mask = None
        self.filled = torch.zeros(n, dtype=torch.bool)
        self.fallbacks = 0
        self.decode_log = DecodeLog(logger or _logger)

    @classmethod
    def for_loader(cls, loader, device, split: str = "data", logger=None):
        """An empty cache for `loader`'s dataset: max_seq from the dataset, crop size and normalisation from its ClipCollate."""
        collate, ds = loader.collate_fn, loader.dataset
        if not all(hasattr(collate, a) for a in ("S", "mean", "std", "rescale")) or not hasattr(ds, "max_seq"):
            raise ValueError("--cache_dataset needs a loader over an MSDDataset with a ClipCollate (real data)")
        norm = (tuple(float(v) for v in collate.mean), tuple(float(v) for v in collate.std), float(collate.rescale))
        return cls(len(ds), ds.max_seq, collate.S, norm, device, split, logger)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.crops, self.input_ids, self.input_mask, self.segment_ids, self.labels))

    def fill(self, batch) -> None:
        ids, mask, seg, img_mask, labels, images = batch
        h_slots = images.indices
        if self._h_img_mask is None:
            self._h_img_mask = img_mask[0].clone()
            self.img_mask = self._h_img_mask.to(self.device)
        if not bool((img_mask == self._h_img_mask).all()):
            raise ValueError(f"the {self.split} split's img_mask is not one constant row: it cannot be cached as one")
        if int(h_slots.min()) < 0 or int(h_slots.max()) >= self.n or bool(self.filled[h_slots].any()):
            raise ValueError(f"the {self.split} split's prefill named a sample twice or outside the {self.n} samples")
        slots = h_slots.to(self.device)
        for dst, src in ((self.input_ids, ids), (self.input_mask, mask), (self.segment_ids, seg), (self.labels, labels)):
            dst.index_copy_(0, slots, src.to(self.device, non_blocking=True))
        images.packed.to_cache(self.device, self.crops, h_slots)
        self.filled[h_slots] = True
        self.fallbacks += images.fallbacks
        if isinstance(images.packed, PackedJpegImages):
            self.decode_log.note((images.packed,))  # keeps the status tensor: read once, in finish()
        else:
            self.decode_log.host += len(images)

    def finish(self) -> None:
        """After the last fill: every sample present, the device work done, the JPEG status words read (the one read-back)."""
        if not bool(self.filled.all()):
            raise ValueError(f"the {self.split} split's prefill left {int((~self.filled).sum())} of {self.n} samples out")
        torch.cuda.synchronize(self.device)
        self.decode_log.end_pass(f"{self.split} split prefill")

    def gather(self, h_idx: torch.Tensor, idx: torch.Tensor, augmenter=None, text_augmenter=None):
        """The trainer's 6-tuple of the samples idx (int64 [B] on the device, h_idx its host copy), on the device.  With an
        `augmenter` (d2r_amd.augment.Augmenter) the pixel values are its augmented view of the crops; with a `text_augmenter`
        (d2r_amd.text_augment.TokenAugmenter) the three token tensors are its augmented view of the rows, from one launch."""
        if augmenter is None:
            images = I.clip_cache_gather(self.crops, h_idx, idx, self.S, self.lut)
        else:
            if augmenter.photometric and augmenter.norm != self.norm:  # the photometric kernel normalises by value, not by the table
                raise ValueError(f"the {self.split} cache is normalised with {self.norm}, the augmenter was built with {augmenter.norm}")
            images = augmenter.apply(self.crops, h_idx, idx, self.lut)
        if text_augmenter is None:
            tokens = (I.gather_rows(self.input_ids, h_idx, idx), I.gather_rows(self.input_mask, h_idx, idx),
                      I.gather_rows(self.segment_ids, h_idx, idx))
        else:
            tokens = text_augmenter.apply(self.input_ids, self.input_mask, self.segment_ids, h_idx, idx)
        batch = CachedBatch((*tokens, self.img_mask.expand(h_idx.numel(), -1), I.gather_rows(self.labels, h_idx, idx), images))
        batch.cached_images = int(h_idx.numel())
        return batch


class CachedBatch(tuple):
    """A batch served from the device cache: the usual 6-tuple, every element on the device; ``cached_images`` is what
    DecodeLog.note counts."""
    cached_images = 0


def release_workers(loader) -> None:
    """Shuts down the worker processes a DataLoader keeps between epochs (persistent_workers); it starts new ones if iterated again."""
    it = getattr(loader, "_iterator", None)
    if it is not None:
        if hasattr(it, "_shutdown_workers"):
            it._shutdown_workers()
        loader._iterator = None


def prefill(loader, cache, logger=None, split: str = "data") -> float:
    """One sequential, unshuffled, drop_last=False pass over `loader`'s dataset into `cache` (fill per batch, finish at the end),
    through the loader's workers' settings and collate function.  The workers are gone afterwards, `loader`'s own included, and
    torch's default generator is as it was.  -> seconds."""
    logger = logger or _logger
    state = torch.get_rng_state()
    t0 = time.time()
    it = None
    try:
        nw = loader.num_workers
        dl = DataLoader(_IndexedSamples(loader.dataset), batch_size=loader.batch_size or 1, shuffle=False, drop_last=False,
                        num_workers=nw, pin_memory=loader.pin_memory, persistent_workers=False,
                        collate_fn=_IndexedCollate(loader.collate_fn), prefetch_factor=loader.prefetch_factor if nw > 0 else None)
        it = iter(dl)
        for batch in it:
            cache.fill(batch)
        cache.finish()
    finally:
        if it is not None and hasattr(it, "_shutdown_workers"):
            it._shutdown_workers()
        release_workers(loader)
        torch.set_rng_state(state)
    seconds = time.time() - t0
    logger.info("%s split cached on the device: %d images, %d inf.png fallback(s), %d bytes held, prefill %.1f s", split,
                getattr(cache, "n", 0), getattr(cache, "fallbacks", 0), getattr(cache, "nbytes", 0), seconds)
    return seconds


class CachedLoader:
    """Stands in for `loader` wherever the trainer looks (__len__, dataset, sampler with set_epoch, batch_sampler, batch_size) and
    yields CachedBatch tuples from `cache` for the index batches of loader.batch_sampler.

    Generator fidelity: a DataLoader draws one int64 from its generator (the default one here) whenever it builds an iterator -
    every epoch, or once when it keeps persistent workers - and the samplers draw theirs as they are iterated.  The same draws are
    made here, in the same order, so the state of the default generator after an epoch equals the plain loader's.

    `augmenter` (training loader only): every batch's images are drawn through it, one draw per batch in batch order.
    `text_augmenter` (training loader only): likewise every batch's token tensors."""

    def __init__(self, loader, cache, augmenter=None, *, text_augmenter=None):
        self.loader, self.cache, self.augmenter, self.text_augmenter = loader, cache, augmenter, text_augmenter
        self._persistent = bool(loader.persistent_workers and loader.num_workers > 0)
        self._started = False

    dataset = property(lambda self: self.loader.dataset)
    sampler = property(lambda self: self.loader.sampler)
    batch_sampler = property(lambda self: self.loader.batch_sampler)
    batch_size = property(lambda self: self.loader.batch_size)
    drop_last = property(lambda self: self.loader.drop_last)

    def __len__(self):
        return len(self.loader)

    def index_batches(self):
        """The host int64 index batches of one epoch (what the plain loader would hand to its dataset), with the loader's draws."""
        if not (self._persistent and self._started):
            torch.empty((), dtype=torch.int64).random_(generator=self.loader.generator)  # the DataLoader iterator's base seed
            self._started = True
        return (torch.tensor(b, dtype=torch.int64) for b in self.loader.batch_sampler)

    def __iter__(self):
        batches = self.index_batches()  # the base-seed draw happens here, as in DataLoader.__iter__, not at the first batch
        return self._batches(batches)

    def _batches(self, batches):
        pin = self.cache.device.type == "cuda"
        for h_idx in batches:
            if pin:
                h_idx = h_idx.pin_memory()
            idx = h_idx.to(self.cache.device, non_blocking=True)
            if self.text_augmenter is not None:
                yield self.cache.gather(h_idx, idx, self.augmenter, text_augmenter=self.text_augmenter)
            else:
                yield self.cache.gather(h_idx, idx) if self.augmenter is None else self.cache.gather(h_idx, idx, self.augmenter)


def cache_loaders(loaders: dict, device, logger=None, augmenters: dict = None, *, text_augmenters: dict = None) -> dict:
    """{split: DataLoader} -> {split: CachedLoader}: every split's cache is sized and checked against the free device memory
    before anything is decoded, then allocated and prefilled in turn.  augmenters: {split: Augmenter} for the splits whose batches
    are augmented (the training split, if any); text_augmenters: {split: TokenAugmenter} likewise for the token tensors."""
    logger = logger or _logger
    needs = []
    for split, dl in loaders.items():
        collate, ds = dl.collate_fn, dl.dataset
        if not hasattr(collate, "S") or not hasattr(ds, "max_seq"):
            raise ValueError("--cache_dataset needs loaders over an MSDDataset with a ClipCollate (real data)")
        needs.append((split, cache_bytes(len(ds), ds.max_seq, collate.S)))
    free, _ = torch.cuda.mem_get_info(torch.device(device))
    check_fit(needs, free)
    caches = {split: DeviceDatasetCache.for_loader(dl, device, split, logger) for split, dl in loaders.items()}
    for split, dl in loaders.items():
        prefill(dl, caches[split], logger, split)
    return {split: CachedLoader(dl, caches[split], (augmenters or {}).get(split), text_augmenter=(text_augmenters or {}).get(split))
            for split, dl in loaders.items()}
