"""--aug_crop_scale / --aug_flip: random resized crop and horizontal flip of the training images, on the device.

Every training image reaches the model through a uint8 crop, planar [3, S, S]: a row of the device cache (d2r_amd.cache), or - without
the cache - a row of a scratch buffer that ``PackedImages.to_cache`` / ``PackedJpegImages.to_cache`` fill for the batch.  One kernel
(d2r_clip_cache_augment, csrc/image.hip) turns such rows into pixel values while it cuts a box per sample out of the normalised
image, resizes it bilinearly to S x S and mirrors it; it moves the bytes of the plain gather.  The boxes are drawn on the host, one
vectorised draw per batch, from a generator of the augmenter's own: torch's default generator (the samplers, the dropout seeds) is
never touched, so every other random choice of a run stays what it was.  The reference has no augmentation; this is an extension,
off by default, and only the training split is ever augmented.

--aug_brightness / --aug_contrast / --aug_saturation / --aug_hue / --aug_grayscale / --aug_erase: the photometric half (colour
jitter, random grayscale, random erasing).  With any of them on, the same launch slot is taken by
d2r_clip_cache_augment_photo, which resamples the raw values and applies brightness, contrast, saturation, hue (in this fixed
order: the random permutation torchvision's ColorJitter draws is not built), grayscale, the normalisation and an erase box per
sample.  Their draws come from a second generator, so the crop / flip stream is the same with and without them.
"""
from __future__ import annotations

import math

import torch

from . import image as I

RATIO = (3.0 / 4.0, 4.0 / 3.0)  # aspect ratios of the box, log-uniform (torchvision's RandomResizedCrop default)
_TAG = 0x6175676D656E74        # "augment": keeps the stream apart from a default generator seeded with the same number
_PHOTO_TAG = 0x70686F746F6D6574  # "photomet": the photometric draws' stream, apart from the boxes', DropPath's and a default generator's
ERASE_AREA = (0.02, 0.33)      # erased fraction of the image, uniform (torchvision's RandomErasing defaults)
ERASE_RATIO = (0.3, 3.3)       # aspect ratio (height / width) of the erase box, log-uniform


def stream_seed(seed: int, rank: int = 0) -> int:
    """The seed of rank `rank`'s augmentation generator in a run seeded `seed`: ``(((seed mod 2^32) << 24) | rank) ^ 0x6175676D656E74``
    with 0 <= rank < 2^24.  Distinct (seed mod 2^32, rank) pairs give distinct seeds (the shift keeps the fields apart, the xor is a
    bijection), so the ranks of one run augment their shards with different streams."""
    if not 0 <= int(rank) < (1 << 24):
        raise ValueError(f"rank must be in [0, 2^24), got {rank}")
    return (((int(seed) & 0xFFFFFFFF) << 24) | int(rank)) ^ _TAG


def photo_stream_seed(seed: int, rank: int = 0) -> int:
    """The seed of rank `rank`'s photometric generator: stream_seed's construction with a tag of its own,
    ``((((seed mod 2^32) << 24) | rank) ^ 0x70686F746F6D6574) mod 2^64`` (as functional.drop_path_stream_seed)."""
    if not 0 <= int(rank) < (1 << 24):
        raise ValueError(f"rank must be in [0, 2^24), got {rank}")
    return ((((int(seed) & 0xFFFFFFFF) << 24) | int(rank)) ^ _PHOTO_TAG) & 0xFFFFFFFFFFFFFFFF


class Augmenter:
    """Random resized crop (area fraction in [crop_scale, 1], aspect ratio in [3/4, 4/3]) and horizontal flip (probability flip_p) of
    S x S crops.  crop_scale = 1 turns the crop off (every box is the whole image) and flip_p = 0 the flip; with both, ``apply`` is
    bit for bit the plain gather.  The draws happen all the same, so the stream does not depend on the settings.

    Keyword-only, all off at 0: brightness / contrast / saturation J (a factor uniform in [max(0, 1 - J), 1 + J] per sample), hue H
    (a shift uniform in [-H, H] turns, H <= 0.5), grayscale_p and erase_p (probabilities); norm = (mean, std, rescale) of the
    normalisation, which the photometric kernel applies itself (rescale must be 1/255).  With any of the six on, ``photometric`` is
    true, a second generator exists (``photo_generator``) and apply / apply_packed launch d2r_clip_cache_augment_photo."""

    def __init__(self, S: int, crop_scale: float = 1.0, flip_p: float = 0.0, seed: int = 0, rank: int = 0, *, brightness: float = 0.0,
                 contrast: float = 0.0, saturation: float = 0.0, hue: float = 0.0, grayscale_p: float = 0.0, erase_p: float = 0.0,
                 norm=(I.CLIP_MEAN, I.CLIP_STD, I.RESCALE)):
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
        for name, v in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        if not 0.0 <= hue <= 0.5:
            raise ValueError(f"hue must be in [0, 0.5], got {hue}")
        for name, v in (("grayscale_p", grayscale_p), ("erase_p", erase_p)):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must be in [0, 1], got {v}")
        self.brightness, self.contrast, self.saturation, self.hue = float(brightness), float(contrast), float(saturation), float(hue)
        self.grayscale_p, self.erase_p = float(grayscale_p), float(erase_p)
        self.photometric = any(v != 0.0 for v in (self.brightness, self.contrast, self.saturation, self.hue, self.grayscale_p,
                                                  self.erase_p))
        self.norm = (tuple(float(v) for v in norm[0]), tuple(float(v) for v in norm[1]), float(norm[2]))
        self.photo_generator = None
        self._ws = None  # fp32 workspace of the contrast mean, reused across steps
        if self.photometric:
            if self.norm[2] != I.RESCALE:
                raise ValueError(f"the photometric options need rescale == 1/255 (pixel values in [0, 1]), got rescale = {self.norm[2]!r}")
            self.photo_generator = torch.Generator(device="cpu")
            self.photo_generator.manual_seed(photo_stream_seed(seed, rank))

    def describe(self) -> str:
        crop = f"scale [{self.crop_scale:g}, 1], ratio [{RATIO[0]:.4g}, {RATIO[1]:.4g}]" if self.crop_scale < 1 else "off"
        text = f"random resized crop {crop}; horizontal flip with probability {self.flip_p:g}"
        if self.photometric:
            text += (f"; brightness {self.brightness:g}, contrast {self.contrast:g}, saturation {self.saturation:g}, hue {self.hue:g} "
                     f"(in this order); grayscale with probability {self.grayscale_p:g}; erasing with probability {self.erase_p:g}")
        return text

    def draw_photo(self, B: int) -> torch.Tensor:
        """Photometric descriptors of one batch, host int32 [B, 12] (d2r_clip_photo_desc: the fp32 bits of brightness, contrast,
        saturation, hue; gray, ex0, ey0, ew, eh; three zeros), from ONE torch.rand(B, 12, float64) of the second generator, whatever
        the settings.  Per sample, with u0..u11 its row and J the setting of a factor:
            factor = lo + u * (1 + J - lo) with lo = max(0, 1 - J) (u0 brightness, u1 contrast, u2 saturation; exactly 1 at J = 0),
            hue = (2 * u3 - 1) * H,  gray = u4 < grayscale_p,
            erase = u5 < erase_p:  area = (0.02 + u6 * 0.31) * S^2,  log r = log 0.3 + u7 * (log 3.3 - log 0.3),
            eh = clamp(round(sqrt(area * r)), 1, S),  ew = clamp(round(sqrt(area / r)), 1, S),
            ex0 = min(floor(u8 * (S - ew + 1)), S - ew),  ey0 = min(floor(u9 * (S - eh + 1)), S - eh);  u10, u11 are spare.
        This is torchvision's ColorJitter (without its random order), RandomGrayscale and RandomErasing(value=0) with their default
        ranges; a side of the erase box that comes out longer than the image is clamped where torchvision draws again."""
        if not self.photometric:
            raise RuntimeError("no photometric option is on: there is no second generator to draw from")
        S = self.S
        u = torch.rand(B, I.PHOTO_FIELDS, dtype=torch.float64, generator=self.photo_generator)
        fac = torch.ones(B, 4, dtype=torch.float64)
        for k, J in enumerate((self.brightness, self.contrast, self.saturation)):
            if J != 0.0:
                lo = max(0.0, 1.0 - J)
                fac[:, k] = lo + u[:, k] * (1.0 + J - lo)
        fac[:, 3] = (2.0 * u[:, 3] - 1.0) * self.hue if self.hue != 0.0 else 0.0
        out = torch.zeros(B, I.PHOTO_FIELDS, dtype=torch.int32)
        out[:, :4] = fac.to(torch.float32).view(torch.int32)  # rounding is monotone: the factors stay >= 0 and |hue| <= 0.5
        out[:, 4] = u[:, 4] < self.grayscale_p
        on = u[:, 5] < self.erase_p
        if bool(on.any()):
            area = (ERASE_AREA[0] + u[:, 6] * (ERASE_AREA[1] - ERASE_AREA[0])) * float(S * S)
            lo, hi = math.log(ERASE_RATIO[0]), math.log(ERASE_RATIO[1])
            r = torch.exp(lo + u[:, 7] * (hi - lo))
            eh = torch.round(torch.sqrt(area * r)).clamp(1, S).to(torch.int64)
            ew = torch.round(torch.sqrt(area / r)).clamp(1, S).to(torch.int64)
            ex0 = torch.minimum(torch.floor(u[:, 8] * (S - ew + 1).double()).to(torch.int64), S - ew)
            ey0 = torch.minimum(torch.floor(u[:, 9] * (S - eh + 1).double()).to(torch.int64), S - eh)
            zero = torch.zeros_like(ew)
            out[:, 5], out[:, 6] = torch.where(on, ex0, zero), torch.where(on, ey0, zero)
            out[:, 7], out[:, 8] = torch.where(on, ew, zero), torch.where(on, eh, zero)
        return out

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
        if self.photometric:  # the normalisation is self.norm's, applied by the kernel: no table
            B = h_idx.numel()
            h_photo = self.draw_photo(B)
            if crops.is_cuda:
                h_photo = h_photo.pin_memory()
            need = I.clip_cache_augment_photo_ws_bytes(B, self.S) // 4
            if self._ws is None or self._ws.numel() < need or self._ws.device != crops.device:
                self._ws = torch.empty(max(need, 1), dtype=torch.float32, device=crops.device)
            return I.clip_cache_augment_photo(crops, h_idx, idx, h_aug, h_aug.to(crops.device, non_blocking=True), h_photo,
                                              h_photo.to(crops.device, non_blocking=True), self.S, self.norm, ws=self._ws)
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
        if self.photometric and packed.norm != self.norm:
            raise ValueError(f"the batch is normalised with {packed.norm}, the augmenter was built with {self.norm}")
        return self.apply(self._scratch, h_slots, slots, I._device_table(str(self._scratch.device), packed.norm))
