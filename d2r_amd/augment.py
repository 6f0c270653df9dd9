"""--aug_crop_scale / --aug_flip: random resized crop and horizontal flip of the training images, on the device.

Every training image reaches the model through a uint8 crop, planar [3, S, S]: a row of the device cache (d2r_amd.cache), or - without
the cache - a row of a scratch buffer that ``PackedImages.to_cache`` / ``PackedJpegImages.to_cache`` fill for the batch.  One kernel
(d2r_clip_cache_augment, csrc/image.hip) turns such rows into pixel values while it cuts a box per sample out of the normalised
image, resizes it bilinearly to S x S and mirrors it; it moves the bytes of the plain gather.  The boxes are drawn on the host, one
vectorised draw per batch, from a generator of the augmenter's own: torch's default generator (the samplers, the dropout seeds) is
never touched, so every other random choice of a run stays what it was.  The reference has no augmentation; this is an extension,
off by default, and only the training split is ever augmented.
"""
from __future__ import annotations

import math

import torch

from . import image as I

RATIO = (3.0 / 4.0, 4.0 / 3.0)  # aspect ratios of the box, log-uniform (torchvision's RandomResizedCrop default)
_TAG = 0x6175676D656E74        # "augment": keeps the stream apart from a default generator seeded with the same number


def stream_seed(seed: int, rank: int = 0) -> int:
    """The seed of rank `rank`'s augmentation generator in a run seeded `seed`: ``(((seed mod 2^32) << 24) | rank) ^ 0x6175676D656E74``
    with 0 <= rank < 2^24.  Distinct (seed mod 2^32, rank) pairs give distinct seeds (the shift keeps the fields apart, the xor is a
    bijection), so the ranks of one run augment their shards with different streams."""
    if not 0 <= int(rank) < (1 << 24):
        raise ValueError(f"rank must be in [0, 2^24), got {rank}")
    return (((int(seed) & 0xFFFFFFFF) << 24) | int(rank)) ^ _TAG


class Augmenter:
    """Random resized crop (area fraction in [crop_scale, 1], aspect ratio in [3/4, 4/3]) and horizontal flip (probability flip_p) of
    S x S crops.  crop_scale = 1 turns the crop off (every box is the whole image) and flip_p = 0 the flip; with both, ``apply`` is
    bit for bit the plain gather.  The draws happen all the same, so the stream does not depend on the settings."""

    def __init__(self, S: int, crop_scale: float = 1.0, flip_p: float = 0.0, seed: int = 0, rank: int = 0):
        if not (isinstance(S, int) and 1 <= S <= 4096):
            raise ValueError(f"S must be an integer in [1, 4096], got {S}")
        if not 0.0 < crop_scale <= 1.0:
            raise ValueError(f"crop_scale must be in (0, 1], got {crop_scale}")
        if not 0.0 <= flip_p <= 1.0:
            raise ValueError(f"flip_p must be in [0, 1], got {flip_p}")
        self.S, self.crop_scale, self.flip_p = S, float(crop_scale), float(flip_p)
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(stream_seed(seed, rank))
        self._slots = {}     # B -> (host arange, device arange) of the uncached path
        self._scratch = None  # uint8 [B, cache_row_bytes(S)] of the uncached path, reused across steps

    def describe(self) -> str:
        crop = f"scale [{self.crop_scale:g}, 1], ratio [{RATIO[0]:.4g}, {RATIO[1]:.4g}]" if self.crop_scale < 1 else "off"
        return f"random resized crop {crop}; horizontal flip with probability {self.flip_p:g}"

    def draw(self, B: int) -> torch.Tensor:
        """Descriptors of one batch, host int32 [B, 8] (x0, y0, w, h, flip, 0, 0, 0: d2r_clip_augment_desc), from ONE
        torch.rand(B, 5, float64) of the augmenter's generator.  Per sample, with u0..u4 its row:
            area = (crop_scale + u0 * (1 - crop_scale)) * S^2,  log r = log(3/4) + u1 * (log(4/3) - log(3/4)),
            w = clamp(round(sqrt(area * r)), 1, S),  h = clamp(round(sqrt(area / r)), 1, S),
            x0 = min(floor(u2 * (S - w + 1)), S - w),  y0 = min(floor(u3 * (S - h + 1)), S - h),  flip = u4 < flip_p.
        This is torchvision's RandomResizedCrop with a side that comes out longer than the image clamped to it, where torchvision
        draws again (up to ten times, then takes a central crop).  The source is square and the ratios are mild, so that only
        happens for areas above 3/4 of the image, and the clamped box still covers at least 3/4 of it.  crop_scale = 1 is "off":
        the box is the whole image (what torchvision arrives at there, through its fallback)."""
        S = self.S
        u = torch.rand(B, 5, dtype=torch.float64, generator=self.generator)
        out = torch.zeros(B, I.AUG_FIELDS, dtype=torch.int32)
        if self.crop_scale < 1.0:
            area = (self.crop_scale + u[:, 0] * (1.0 - self.crop_scale)) * float(S * S)
            lo, hi = math.log(RATIO[0]), math.log(RATIO[1])
            r = torch.exp(lo + u[:, 1] * (hi - lo))
            w = torch.round(torch.sqrt(area * r)).clamp(1, S).to(torch.int64)
            h = torch.round(torch.sqrt(area / r)).clamp(1, S).to(torch.int64)
            x0 = torch.minimum(torch.floor(u[:, 2] * (S - w + 1).double()).to(torch.int64), S - w)
            y0 = torch.minimum(torch.floor(u[:, 3] * (S - h + 1).double()).to(torch.int64), S - h)
            out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x0, y0, w, h
        else:
            out[:, 2] = out[:, 3] = S
        out[:, 4] = u[:, 4] < self.flip_p
        return out

    def apply(self, crops: torch.Tensor, h_idx: torch.Tensor, idx: torch.Tensor, lut: torch.Tensor = None) -> torch.Tensor:
        """Draws one batch of boxes, uploads them (one non-blocking copy from pinned memory) and launches d2r_clip_cache_augment on
        the current stream: fp32 [B, 3, S, S] pixel values of the rows idx of `crops` (uint8 [rows, cache_row_bytes(S)] on the
        device; h_idx is the host copy of idx).  lut: the device's [3, 256] table (CLIP's when None)."""
        h_aug = self.draw(h_idx.numel())
        if crops.is_cuda:
            h_aug = h_aug.pin_memory()
        if lut is None:
            lut = I._device_table(str(crops.device), (I.CLIP_MEAN, I.CLIP_STD, I.RESCALE))
        return I.clip_cache_augment(crops, h_idx, idx, h_aug, h_aug.to(crops.device, non_blocking=True), self.S, lut)

    def apply_packed(self, packed, device) -> torch.Tensor:
        """The uncached path: a collated image batch (PackedImages / PackedJpegImages) becomes uint8 crops in rows 0..B-1 of a
        scratch buffer that is reused across steps (``to_cache``), and ``apply`` reads them from there."""
        B = len(packed)
        if packed.S != self.S:
            raise ValueError(f"the batch holds {packed.S} x {packed.S} crops, the augmenter was built for {self.S}")
        device = torch.device(device)
        if self._scratch is None or self._scratch.shape[0] < B or self._scratch.device != device:
            self._scratch = torch.empty(B, I.cache_row_bytes(self.S), dtype=torch.uint8, device=device)
        if B not in self._slots:
            h = torch.arange(B, dtype=torch.int64)
            h = h.pin_memory() if device.type == "cuda" else h
            self._slots[B] = (h, h.to(device))
        h_slots, slots = self._slots[B]
        packed.to_cache(device, self._scratch, h_slots)
        return self.apply(self._scratch, h_slots, slots, I._device_table(str(self._scratch.device), packed.norm))
