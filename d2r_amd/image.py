"""CLIP image preprocessing on the device: what ``CLIPProcessor(images=img)`` does per sample in the reference's loader
workers (processor/dataset.py:87-95), bit-identical, as one batched launch pair (``d2r_clip_preprocess``, csrc/image.hip).

The processor (transformers' CLIPImageProcessor, PIL backend, with the CLIP defaults) does four things to a uint8 RGB image:
  1. output size: the short side becomes R (``size["shortest_edge"]``), the long side ``int(R * long / short)``;
  2. ``PIL.Image.resize(..., BICUBIC)``: Pillow's separable antialiased resampler in 22-bit fixed point, horizontal pass first
     into a uint8 image, vertical pass from it;
  3. center crop S x S at ``((rh - S) // 2, (rw - S) // 2)``;
  4. rescale and normalise: ``(float32(float64(v) * rescale) - float32(mean_c)) / float32(std_c)`` in fp32, a function of the
     uint8 value and the channel alone (a [3, 256] table).
The device computes only the cropped pixels (every output pixel depends on its own weights alone), in integer arithmetic.  The
weights themselves are computed here in float64, in Pillow's operation order (a sequential sum for the normalisation, no fused
multiply-add): a pairwise sum, or the same arithmetic contracted to FMA on the device, can flip an integer weight.

The loader side (``ClipCollate``) packs a batch of decoded images into ``PackedImages``: one uint8 buffer of the pixels and one
buffer of descriptors + weight tables; ``PackedImages.to_pixel_values(device)`` copies both (non-blocking from pinned memory) and
launches the kernels on the current stream.  ``reference_preprocess`` is the same computation in numpy (tests, CPU checks).
``to_cache`` stops one step earlier: the uint8 crop goes into rows of a device-resident cache (``d2r_clip_preprocess_u8``), from
which ``clip_cache_gather`` later builds the same pixel values by index (d2r_amd.cache, --cache_dataset device).
``clip_cache_augment`` is that gather with a box per sample resized bilinearly to S x S and an optional mirror (d2r_amd.augment);
``reference_augment`` restates it in numpy float64.  ``clip_cache_augment_photo`` adds the photometric half (brightness, contrast,
saturation, hue, grayscale, erase box: DESIGN.md K22) to the same resample of the raw values; ``reference_photo`` restates that.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import math
import os

import numpy as np
import torch

from . import _lib

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)  # OpenAI CLIP (CLIPImageProcessor defaults)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
RESCALE = 1 / 255
PRECISION_BITS = 22  # Pillow's fixed-point weights (libImaging/Resample.c)

DESC_DTYPE = np.dtype([("src_offset", "<i8")] + [(n, "<i4") for n in ("H", "W", "rh", "rw", "top", "left", "kx", "ky", "bx", "cx",
                                                                      "by", "cy", "row0", "nrows")] + [("ws_offset", "<i8")])
assert DESC_DTYPE.itemsize == C.sizeof(_lib.ClipImageDesc)


def resize_shape(H: int, W: int, R: int):
    """(rh, rw) of the resize to shortest edge R: Python float division, then truncation (transformers'
    get_resize_output_image_size with default_to_square=False)."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(R * long / short)
    return (new_long, R) if W <= H else (R, new_long)


def crop_origin(rh: int, rw: int, S: int):
    if S > rh or S > rw:
        raise ValueError(f"a {S} x {S} crop of a {rh} x {rw} image needs padding, which is not supported")
    return (rh - S) // 2, (rw - S) // 2


def _bicubic(x):
    """Pillow's bicubic filter (a = -0.5), elementwise in float64 with the same operations as the C code."""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


@functools.lru_cache(maxsize=4096)
def bicubic_weights(in_size: int, out_size: int, lo: int, count: int):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for output indices [lo, lo + count) of an in_size -> out_size
    resize: (bounds int32 [count, 2] = (xmin, n), weights int32 [count, k]); weights past n are 0."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(lo, lo + count, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    n = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)
    w = _bicubic(((x[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(x[None, :] < n[:, None], w, 0.0)
    total = np.add.accumulate(w, axis=1)[:, -1]  # left-to-right, as the C loop (np.sum would be pairwise)
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one)).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    bounds.flags.writeable = False
    k.flags.writeable = False
    return bounds, k


def _clip8(acc):
    return np.where(acc >= (1 << PRECISION_BITS << 8), 255, np.where(acc <= 0, 0, acc >> PRECISION_BITS)).astype(np.uint8)


def _apply(src, bounds, k, axis):
    """One fixed-point pass along `axis` (1 = columns, 0 = rows) of a uint8 [rows, cols, 3] array."""
    src = src.astype(np.int64)
    size = src.shape[axis]
    acc = np.full((src.shape[0], len(bounds), 3) if axis == 1 else (len(bounds), src.shape[1], 3), 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(k.shape[1]):
        idx = np.minimum(bounds[:, 0] + t, size - 1)  # weights past n are 0: the clamped index adds nothing
        if axis == 1:
            acc += src[:, idx, :] * k[None, :, t, None]
        else:
            acc += src[idx, :, :] * k[:, t, None, None]
    return _clip8(acc)


def resample(img: np.ndarray, rh: int, rw: int, top: int = 0, left: int = 0, h: int = None, w: int = None) -> np.ndarray:
    """Rows [top, top + h) x columns [left, left + w) of Pillow's BICUBIC resize of uint8 HWC RGB `img` to rh x rw (numpy)."""
    H, W, _ = img.shape
    h, w = rh if h is None else h, rw if w is None else w
    bx, kx = bicubic_weights(W, rw, left, w)
    by, ky = bicubic_weights(H, rh, top, h)
    row0, row1 = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
    mid = _apply(img[row0:row1], bx, kx, axis=1)
    return _apply(mid, np.stack([by[:, 0] - row0, by[:, 1]], 1), ky, axis=0)


def normalize_table(mean=CLIP_MEAN, std=CLIP_STD, rescale=RESCALE) -> np.ndarray:
    """fp32 [3, 256]: the normalised value of every (channel, uint8) pair, in the processor's exact arithmetic."""
    r = (np.arange(256, dtype=np.float64) * float(rescale)).astype(np.float32)
    m = np.asarray(mean, np.float64).astype(np.float32)[:, None]
    s = np.asarray(std, np.float64).astype(np.float32)[:, None]
    return ((r[None, :] - m) / s).astype(np.float32)


def reference_preprocess(img: np.ndarray, R: int, S: int, table: np.ndarray = None):
    """CPU restatement of the whole pipeline: (uint8 crop [S, S, 3], fp32 pixel values [3, S, S])."""
    rh, rw = resize_shape(img.shape[0], img.shape[1], R)
    top, left = crop_origin(rh, rw, S)
    crop = resample(np.ascontiguousarray(img), rh, rw, top, left, S, S)
    table = normalize_table() if table is None else table
    return crop, np.stack([table[c][crop[:, :, c]] for c in range(3)])


def as_rgb_array(img) -> np.ndarray:
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected a uint8 [H, W, 3] RGB image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def plan_batch(images, R: int, S: int):
    """Packs decoded images for d2r_clip_preprocess: (pixels uint8 [N], descriptors DESC_DTYPE [B], table int32 [T])."""
    images = [as_rgb_array(im) for im in images]
    if not images:
        raise ValueError("empty batch")
    offsets = np.cumsum([0] + [im.size for im in images[:-1]])
    desc, tab = plan_layout([im.shape[:2] for im in images], offsets, R, S)
    return np.concatenate([im.reshape(-1) for im in images]), desc, tab


def plan_layout(shapes, offsets, R: int, S: int):
    """Descriptors DESC_DTYPE [B] and the int32 table for images of `shapes` (H, W) whose pixels sit at byte `offsets` of the
    source buffer (the images need not be decoded yet)."""
    B = len(shapes)
    if B == 0:
        raise ValueError("empty batch")
    desc = np.zeros(B, DESC_DTYPE)
    tab, tlen, ws = [], 0, 0
    for b, (H, W) in enumerate(shapes):
        rh, rw = resize_shape(H, W, R)
        top, left = crop_origin(rh, rw, S)
        bx, kx = bicubic_weights(W, rw, left, S)
        by, ky = bicubic_weights(H, rh, top, S)
        row0, row1 = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
        d = desc[b]
        d["src_offset"], d["H"], d["W"], d["rh"], d["rw"], d["top"], d["left"] = int(offsets[b]), H, W, rh, rw, top, left
        d["kx"], d["ky"], d["row0"], d["nrows"], d["ws_offset"] = kx.shape[1], ky.shape[1], row0, row1 - row0, ws
        for name, arr in (("bx", bx), ("cx", kx), ("by", by), ("cy", ky)):
            d[name] = tlen
            tab.append(arr.reshape(-1))
            tlen += arr.size
        ws += -(-(row1 - row0) * S * 3 // 16) * 16  # 16-byte aligned regions
    return desc, np.concatenate(tab).astype(np.int32)


@functools.lru_cache(maxsize=16)
def _device_table(device: str, norm: tuple):
    return torch.from_numpy(normalize_table(*norm)).to(device)


def clip_preprocess(pixels: torch.Tensor, h_desc: np.ndarray, desc: torch.Tensor, h_tab: torch.Tensor, tab: torch.Tensor, S: int,
                    lut: torch.Tensor, out: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """d2r_clip_preprocess on the current stream.  pixels / desc / tab / lut live on the device, h_desc / h_tab are their host
    copies (the library checks every bound on them before it enqueues anything).  Returns out, fp32 [B, 3, S, S]."""
    B = len(h_desc)
    dev = pixels.device
    if not (pixels.dtype == torch.uint8 and desc.dtype == torch.uint8 and tab.dtype == torch.int32 and lut.dtype == torch.float32):
        raise TypeError("pixels / desc uint8, tab int32, lut float32 expected")
    if h_desc.dtype != DESC_DTYPE or desc.numel() != B * DESC_DTYPE.itemsize or h_tab.numel() != tab.numel() or lut.numel() != 768:
        raise ValueError("descriptor / table / lut sizes disagree")
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() for t in (desc, tab, lut)) or h_tab.is_cuda or not h_tab.is_contiguous():
        raise ValueError("device tensors must be contiguous on one GPU, h_tab on the host")
    hd = C.cast(h_desc.ctypes.data, C.POINTER(_lib.ClipImageDesc))
    need = int(_lib.load().d2r_clip_preprocess_ws_bytes(hd, B, S))
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * 3 * S * S:
        raise ValueError("out must be a contiguous fp32 [B, 3, S, S] tensor")
    from .functional import _stream
    _lib.call("d2r_clip_preprocess", pixels.data_ptr(), pixels.numel(), hd, desc.data_ptr(), B, S, h_tab.data_ptr(), tab.data_ptr(),
              tab.numel(), lut.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out


def cache_row_bytes(S: int) -> int:
    """Bytes of one row of a crop cache: the planar uint8 [3, S, S] crop, padded to a multiple of 16."""
    return int(_lib.load().d2r_clip_cache_row_bytes(S))


def clip_preprocess_u8(pixels: torch.Tensor, h_desc: np.ndarray, desc: torch.Tensor, h_tab: torch.Tensor, tab: torch.Tensor, S: int,
                       cache: torch.Tensor, h_slots: torch.Tensor, slots: torch.Tensor, ws: torch.Tensor = None) -> None:
    """d2r_clip_preprocess_u8 on the current stream: image b's uint8 crop, planar [3, S, S], into row slots[b] of `cache` (uint8
    [rows, cache_row_bytes(S)] on the device).  h_slots (host) and slots (device) are int64 [B]; the library checks every bound on
    the host copies before it enqueues anything."""
    B = len(h_desc)
    dev = pixels.device
    if not (pixels.dtype == torch.uint8 and desc.dtype == torch.uint8 and tab.dtype == torch.int32 and cache.dtype == torch.uint8 and
            h_slots.dtype == torch.int64 and slots.dtype == torch.int64):
        raise TypeError("pixels / desc / cache uint8, tab int32, slots int64 expected")
    if h_desc.dtype != DESC_DTYPE or desc.numel() != B * DESC_DTYPE.itemsize or h_tab.numel() != tab.numel() or \
            h_slots.numel() != B or slots.numel() != B or cache.dim() != 2 or cache.shape[1] != cache_row_bytes(S):
        raise ValueError("descriptor / table / slot / cache sizes disagree")
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() for t in (desc, tab, cache, slots)) or h_tab.is_cuda or \
            not h_tab.is_contiguous() or h_slots.is_cuda or not h_slots.is_contiguous():
        raise ValueError("device tensors must be contiguous on one GPU, h_tab / h_slots on the host")
    hd = C.cast(h_desc.ctypes.data, C.POINTER(_lib.ClipImageDesc))
    if ws is None:
        ws = torch.empty(max(int(_lib.load().d2r_clip_preprocess_ws_bytes(hd, B, S)), 1), dtype=torch.uint8, device=dev)
    from .functional import _stream
    _lib.call("d2r_clip_preprocess_u8", pixels.data_ptr(), pixels.numel(), hd, desc.data_ptr(), B, S, h_tab.data_ptr(), tab.data_ptr(),
              tab.numel(), cache.data_ptr(), cache.shape[0], h_slots.data_ptr(), slots.data_ptr(), ws.data_ptr(), ws.numel(), _stream())


def clip_cache_gather(cache: torch.Tensor, h_idx: torch.Tensor, idx: torch.Tensor, S: int, lut: torch.Tensor,
                      out: torch.Tensor = None) -> torch.Tensor:
    """d2r_clip_cache_gather on the current stream: fp32 [B, 3, S, S] pixel values of the cache rows idx (int64 [B] on the device,
    h_idx its host copy; repeats allowed)."""
    B = h_idx.numel()
    dev = cache.device
    if not (cache.dtype == torch.uint8 and h_idx.dtype == torch.int64 and idx.dtype == torch.int64 and lut.dtype == torch.float32):
        raise TypeError("cache uint8, idx int64, lut float32 expected")
    if cache.dim() != 2 or cache.shape[1] != cache_row_bytes(S) or idx.numel() != B or lut.numel() != 768:
        raise ValueError("cache / index / lut sizes disagree")
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() for t in (cache, idx, lut)) or h_idx.is_cuda or not h_idx.is_contiguous():
        raise ValueError("device tensors must be contiguous on one GPU, h_idx on the host")
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * 3 * S * S or out.device != dev:
        raise ValueError("out must be a contiguous fp32 [B, 3, S, S] tensor on the cache's device")
    from .functional import _stream
    _lib.call("d2r_clip_cache_gather", cache.data_ptr(), cache.shape[0], h_idx.data_ptr(), idx.data_ptr(), B, S, lut.data_ptr(),
              out.data_ptr(), _stream())
    return out


AUG_FIELDS = 8  # int32 per d2r_clip_augment_desc: x0, y0, w, h, flip, three reserved zeros
assert 4 * AUG_FIELDS == C.sizeof(_lib.ClipAugmentDesc)


def clip_cache_augment(cache: torch.Tensor, h_idx: torch.Tensor, idx: torch.Tensor, h_aug: torch.Tensor, aug: torch.Tensor, S: int,
                       lut: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """d2r_clip_cache_augment on the current stream: clip_cache_gather with one box per output sample, resized bilinearly to S x S
    and mirrored when its flip is set.  aug is int32 [B, 8] on the device (x0, y0, w, h, flip, 0, 0, 0 per sample), h_aug its host
    copy; the library checks indices and boxes on the host copies before it enqueues anything."""
    B = h_idx.numel()
    dev = cache.device
    if not (cache.dtype == torch.uint8 and h_idx.dtype == torch.int64 and idx.dtype == torch.int64 and lut.dtype == torch.float32 and
            h_aug.dtype == torch.int32 and aug.dtype == torch.int32):
        raise TypeError("cache uint8, idx int64, aug int32, lut float32 expected")
    if cache.dim() != 2 or cache.shape[1] != cache_row_bytes(S) or idx.numel() != B or lut.numel() != 768 or \
            tuple(h_aug.shape) != (B, AUG_FIELDS) or tuple(aug.shape) != (B, AUG_FIELDS):
        raise ValueError("cache / index / descriptor / lut sizes disagree")
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() for t in (cache, idx, aug, lut)) or \
            any(t.is_cuda or not t.is_contiguous() for t in (h_idx, h_aug)):
        raise ValueError("device tensors must be contiguous on one GPU, h_idx / h_aug on the host")
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * 3 * S * S or out.device != dev:
        raise ValueError("out must be a contiguous fp32 [B, 3, S, S] tensor on the cache's device")
    from .functional import _stream
    _lib.call("d2r_clip_cache_augment", cache.data_ptr(), cache.shape[0], h_idx.data_ptr(), idx.data_ptr(),
              C.cast(h_aug.data_ptr(), C.POINTER(_lib.ClipAugmentDesc)), aug.data_ptr(), B, S, lut.data_ptr(), out.data_ptr(), _stream())
    return out


def reference_augment(crop: np.ndarray, box, S: int, table: np.ndarray = None) -> np.ndarray:
    """CPU restatement of d2r_clip_cache_augment for one sample, in float64: `crop` uint8 planar [3, S, S] (a cache row), `box` =
    (x0, y0, w, h, flip), `table` fp32 [3, 256] -> float64 [3, S, S].  The coordinates are computed in integers exactly as the kernel
    does; only the blend is carried out in float64 instead of fp32."""
    x0, y0, w, h, flip = (int(v) for v in box)
    crop = np.asarray(crop)
    if crop.dtype != np.uint8 or crop.shape != (3, S, S):
        raise ValueError(f"expected a uint8 [3, {S}, {S}] crop, got {crop.dtype} {crop.shape}")
    if not (x0 >= 0 and y0 >= 0 and w >= 1 and h >= 1 and x0 + w <= S and y0 + h <= S and flip in (0, 1)):
        raise ValueError(f"box {tuple(box)} does not lie inside the {S} x {S} crop")
    table = normalize_table() if table is None else table

    def axis(o, n):
        nx = np.maximum((2 * o + 1) * n - S, 0)
        lo = nx // (2 * S)
        return lo, np.minimum(lo + 1, n - 1), (nx % (2 * S)).astype(np.float64) / float(2 * S)

    pos = np.arange(S, dtype=np.int64)
    ix0, ix1, fx = axis(S - 1 - pos if flip else pos, w)
    iy0, iy1, fy = axis(pos, h)
    fx, fy = fx[None, :], fy[:, None]
    out = np.empty((3, S, S), np.float64)
    for c in range(3):
        T = np.asarray(table[c], np.float64)[crop[c]]
        a, b = T[np.ix_(y0 + iy0, x0 + ix0)], T[np.ix_(y0 + iy0, x0 + ix1)]
        c_, d = T[np.ix_(y0 + iy1, x0 + ix0)], T[np.ix_(y0 + iy1, x0 + ix1)]
        out[c] = (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c_ + fx * d)
    return out


PHOTO_FIELDS = 12  # 32-bit words per d2r_clip_photo_desc: fp32 brightness, contrast, saturation, hue; int32 gray, ex0, ey0, ew, eh, 3 x 0
assert 4 * PHOTO_FIELDS == C.sizeof(_lib.ClipPhotoDesc)
GRAY_WEIGHTS = (0.299, 0.587, 0.114)  # g(x) of K22 (ITU-R 601 luma: torchvision's rgb_to_grayscale, Pillow's "L")


def photo_desc(rows) -> torch.Tensor:
    """Host int32 [B, 12] descriptors (the four factors as their fp32 bits) from rows (brightness, contrast, saturation, hue, gray,
    ex0, ey0, ew, eh)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 9)
    d = np.zeros((len(rows), PHOTO_FIELDS), np.int32)
    d[:, :4] = rows[:, :4].astype(np.float32).view(np.int32)
    d[:, 4:9] = rows[:, 4:].astype(np.int32)
    return torch.from_numpy(d)


def clip_cache_augment_photo_ws_bytes(B: int, S: int) -> int:
    return int(_lib.load().d2r_clip_cache_augment_photo_ws_bytes(B, S))


def clip_cache_augment_photo(cache: torch.Tensor, h_idx: torch.Tensor, idx: torch.Tensor, h_aug: torch.Tensor, aug: torch.Tensor,
                             h_photo: torch.Tensor, photo: torch.Tensor, S: int, norm=(CLIP_MEAN, CLIP_STD, RESCALE),
                             out: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """d2r_clip_cache_augment_photo on the current stream: clip_cache_augment on the raw values (no table) followed per sample by
    brightness, contrast, saturation, hue, grayscale, the normalisation with norm = (mean, std, rescale) and an erase box (K22).
    photo is int32 [B, 12] on the device (``photo_desc``), h_photo its host copy; ws a float32 workspace of at least
    clip_cache_augment_photo_ws_bytes(B, S) bytes on the device (allocated when None).  The library checks indices, boxes and
    descriptors on the host copies before it enqueues anything."""
    B = h_idx.numel()
    dev = cache.device
    if not (cache.dtype == torch.uint8 and h_idx.dtype == torch.int64 and idx.dtype == torch.int64 and h_aug.dtype == torch.int32 and
            aug.dtype == torch.int32 and h_photo.dtype == torch.int32 and photo.dtype == torch.int32):
        raise TypeError("cache uint8, idx int64, aug / photo int32 expected")
    if cache.dim() != 2 or cache.shape[1] != cache_row_bytes(S) or idx.numel() != B or tuple(h_aug.shape) != (B, AUG_FIELDS) or \
            tuple(aug.shape) != (B, AUG_FIELDS) or tuple(h_photo.shape) != (B, PHOTO_FIELDS) or tuple(photo.shape) != (B, PHOTO_FIELDS):
        raise ValueError("cache / index / descriptor sizes disagree")
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() for t in (cache, idx, aug, photo)) or \
            any(t.is_cuda or not t.is_contiguous() for t in (h_idx, h_aug, h_photo)):
        raise ValueError("device tensors must be contiguous on one GPU, h_idx / h_aug / h_photo on the host")
    mean, std, rescale = norm
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("norm must be (mean[3], std[3], rescale)")
    need = clip_cache_augment_photo_ws_bytes(B, S)
    if ws is None:
        ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
    elif ws.dtype != torch.float32 or not ws.is_contiguous() or ws.device != dev:
        raise ValueError("ws must be a contiguous fp32 tensor on the cache's device")
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * 3 * S * S or out.device != dev:
        raise ValueError("out must be a contiguous fp32 [B, 3, S, S] tensor on the cache's device")
    h_norm = (C.c_float * 6)(*[float(v) for v in mean], *[float(v) for v in std])
    from .functional import _stream
    _lib.call("d2r_clip_cache_augment_photo", cache.data_ptr(), cache.shape[0], h_idx.data_ptr(), idx.data_ptr(),
              C.cast(h_aug.data_ptr(), C.POINTER(_lib.ClipAugmentDesc)), aug.data_ptr(),
              C.cast(h_photo.data_ptr(), C.POINTER(_lib.ClipPhotoDesc)), photo.data_ptr(), B, S, h_norm, float(rescale), out.data_ptr(),
              ws.data_ptr(), ws.numel() * 4, _stream())
    return out


def _gray64(x):
    return GRAY_WEIGHTS[0] * x[0] + GRAY_WEIGHTS[1] * x[1] + GRAY_WEIGHTS[2] * x[2]


def reference_hue(x: np.ndarray, delta: float) -> np.ndarray:
    """Step 4 of K22 in float64 on x [3, ...] in [0, 1]: RGB -> HSV (hexcone), h <- frac(h + delta), HSV -> RGB."""
    r, g, b = x[0], x[1], x[2]
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    cr = mx - mn
    grey = cr == 0
    s = cr / np.where(grey, 1.0, mx)
    dv = np.where(grey, 1.0, cr)
    rc, gc, bc = (mx - r) / dv, (mx - g) / dv, (mx - b) / dv
    h6 = np.where(mx == r, bc - gc, np.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = h6 / 6.0 + delta
    h = h - np.floor(h)
    hs = h * 6.0
    fl = np.floor(hs)
    f = hs - fl
    sec = fl.astype(np.int64) % 6
    p, q, t = mx * (1.0 - s), mx * (1.0 - s * f), mx * (1.0 - s * (1.0 - f))
    p, q, t = (np.clip(v, 0.0, 1.0) for v in (p, q, t))
    pick = lambda table: np.choose(sec, table)  # noqa: E731
    return np.stack([pick([mx, q, p, p, t, mx]), pick([t, mx, mx, q, p, p]), pick([p, p, t, mx, mx, q])])


def reference_photo(crop: np.ndarray, box, photo, S: int, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """CPU restatement of d2r_clip_cache_augment_photo for one sample, in float64 (K22): `crop` uint8 planar [3, S, S], `box` =
    (x0, y0, w, h, flip), `photo` = (brightness, contrast, saturation, hue, gray, ex0, ey0, ew, eh) -> float64 [3, S, S].  The
    resample is reference_augment's, of the raw values crop / 255."""
    beta, kappa, sigma, delta = (float(v) for v in photo[:4])
    gray, ex0, ey0, ew, eh = (int(v) for v in photo[4:9])
    if not all(math.isfinite(v) and v >= 0 for v in (beta, kappa, sigma)) or not abs(delta) <= 0.5 or gray not in (0, 1):
        raise ValueError(f"bad photometric settings {tuple(photo)}")
    if ew != 0 and not (ex0 >= 0 and ey0 >= 0 and ew >= 1 and eh >= 1 and ex0 + ew <= S and ey0 + eh <= S):
        raise ValueError(f"erase box {(ex0, ey0, ew, eh)} is neither empty nor inside the {S} x {S} output")
    raw = np.tile(np.arange(256, dtype=np.float64) / 255.0, (3, 1))
    x = reference_augment(crop, box, S, raw)
    if beta != 1.0:
        x = np.clip(beta * x, 0.0, 1.0)
    if kappa != 1.0:
        x = np.clip(kappa * x + (1.0 - kappa) * _gray64(x).mean(), 0.0, 1.0)
    if sigma != 1.0:
        x = np.clip(sigma * x + (1.0 - sigma) * _gray64(x)[None], 0.0, 1.0)
    if delta != 0.0:
        x = reference_hue(x, delta)
    if gray:
        x = np.repeat(_gray64(x)[None], 3, axis=0)
    x = (x - np.asarray(mean, np.float64)[:, None, None]) / np.asarray(std, np.float64)[:, None, None]
    if ew != 0:
        x[:, ey0:ey0 + eh, ex0:ex0 + ew] = 0.0
    return x


def gather_rows(src: torch.Tensor, h_idx: torch.Tensor, idx: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """d2r_gather_rows on the current stream: out[b] = src[idx[b]] for a contiguous device tensor src [N, ...] (idx int64 [B] on
    the device, h_idx its host copy)."""
    B = h_idx.numel()
    if not (src.is_cuda and src.is_contiguous() and src.dim() >= 1 and src.shape[0] >= 1):
        raise ValueError("src must be a contiguous device tensor with at least one row")
    if not (h_idx.dtype == torch.int64 and idx.dtype == torch.int64 and idx.numel() == B and idx.is_cuda and idx.device == src.device and
            idx.is_contiguous() and not h_idx.is_cuda and h_idx.is_contiguous()):
        raise ValueError("idx must be a contiguous int64 tensor on src's device, h_idx its host copy")
    if out is None:
        out = torch.empty((B,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    elif out.dtype != src.dtype or not out.is_contiguous() or out.device != src.device or out.numel() * src.shape[0] != B * src.numel():
        raise ValueError("out must be a contiguous [B, ...] tensor of src's dtype on its device")
    row_bytes = src.numel() // src.shape[0] * src.element_size()
    from .functional import _stream
    _lib.call("d2r_gather_rows", out.data_ptr(), src.data_ptr(), src.shape[0], row_bytes, h_idx.data_ptr(), idx.data_ptr(), B, _stream())
    return out


def _crops_to_cache(pixels, clip_meta, batch, S, cache, h_slots):
    """Shared tail of PackedImages.to_cache / PackedJpegImages.to_cache: `pixels` are the batch's source pixels on the device."""
    nd = batch * DESC_DTYPE.itemsize
    meta = clip_meta.to(pixels.device, non_blocking=True)
    h_desc = clip_meta.numpy()[:nd].view(DESC_DTYPE)
    clip_preprocess_u8(pixels, h_desc, meta[:nd], clip_meta[nd:].view(torch.int32), meta[nd:].view(torch.int32), S, cache, h_slots,
                       h_slots.to(pixels.device, non_blocking=True))


class PackedImages:
    """A collated batch of decoded images: the loader element the trainer turns into pixel values on the device.
    ``pixels`` uint8 [N] (HWC RGB images back to back), ``meta`` uint8 [B * 72 + 4 * T] (descriptors, then the int32 table)."""

    def __init__(self, pixels: torch.Tensor, meta: torch.Tensor, batch: int, S: int, norm: tuple):
        self.pixels, self.meta, self.batch, self.S, self.norm = pixels, meta, batch, S, norm

    @classmethod
    def from_images(cls, images, R: int, S: int, mean=CLIP_MEAN, std=CLIP_STD, rescale=RESCALE):
        pixels, desc, tab = plan_batch(images, R, S)
        meta = np.concatenate([desc.view(np.uint8), tab.view(np.uint8)])
        return cls(torch.from_numpy(pixels), torch.from_numpy(meta), len(desc),
                   S, (tuple(float(v) for v in mean), tuple(float(v) for v in std), float(rescale)))

    def __len__(self):
        return self.batch

    def pin_memory(self, device=None):  # DataLoader(pin_memory=True) calls this in its pinning thread
        return PackedImages(self.pixels.pin_memory(), self.meta.pin_memory(), self.batch, self.S, self.norm)

    def host_parts(self):
        nd = self.batch * DESC_DTYPE.itemsize
        h = self.meta.numpy()
        return h[:nd].view(DESC_DTYPE), self.meta[nd:].view(torch.int32)

    def to_pixel_values(self, device) -> torch.Tensor:
        """fp32 [B, 3, S, S] on `device`: the two host-to-device copies (non-blocking; from pinned memory they overlap what the
        stream is doing) and the two kernels, all on the current stream."""
        h_desc, h_tab = self.host_parts()
        pixels = self.pixels.to(device, non_blocking=True)
        meta = self.meta.to(device, non_blocking=True)
        nd = self.batch * DESC_DTYPE.itemsize
        return clip_preprocess(pixels, h_desc, meta[:nd], h_tab, meta[nd:].view(torch.int32), self.S,
                               _device_table(str(pixels.device), self.norm))

    def to_cache(self, device, cache: torch.Tensor, h_slots: torch.Tensor) -> None:
        """The batch's uint8 crops into rows h_slots (host int64 [B]) of the crop cache on `device`: the copies of
        to_pixel_values, then d2r_clip_preprocess_u8."""
        _crops_to_cache(self.pixels.to(device, non_blocking=True), self.meta, self.batch, self.S, cache, h_slots)

    def to_pixel_values_cpu(self) -> torch.Tensor:
        """The same batch through the numpy restatement (reference_preprocess): fp32 [B, 3, S, S] on the host."""
        h_desc, _ = self.host_parts()
        px = self.pixels.numpy()
        table = normalize_table(*self.norm)
        out = []
        for d in h_desc:
            img = px[int(d["src_offset"]):int(d["src_offset"]) + int(d["H"]) * int(d["W"]) * 3].reshape(int(d["H"]), int(d["W"]), 3)
            crop = resample(img, int(d["rh"]), int(d["rw"]), int(d["top"]), int(d["left"]), self.S, self.S)
            out.append(np.stack([table[c][crop[:, :, c]] for c in range(3)]))
        return torch.from_numpy(np.stack(out))


class ClipCollate:
    """collate_fn for MSDDataset samples (ids, mask, segments, img_mask, label, uint8 image): the five tensors stacked, the
    images packed into one PackedImages.  Runs in the loader workers (picklable).  With ``image_decode="device"`` (for
    MSDDataset(image_decode="device")), or when some images are parsed JPEG files, the batch becomes a
    d2r_amd.jpeg.PackedJpegImages, which decodes those on the device."""

    def __init__(self, R: int = 224, S: int = 224, mean=CLIP_MEAN, std=CLIP_STD, rescale=RESCALE, image_decode: str = "host"):
        self.R, self.S, self.mean, self.std, self.rescale = R, S, tuple(mean), tuple(std), rescale
        self.image_decode = image_decode

    def __call__(self, samples):
        cols = list(zip(*samples))
        head = [torch.stack(list(c)) for c in cols[:5]]
        from .jpeg import JpegInfo, PackedJpegImages
        if self.image_decode == "device" or any(isinstance(im, JpegInfo) for im in cols[5]):
            # MSDDataset(image_decode="device"): parsed JPEG files for the device, any others decoded; every such batch is a
            # PackedJpegImages, so that the trainer counts its host-decoded images too
            return (*head, PackedJpegImages.from_items(cols[5], self.R, self.S, self.mean, self.std, self.rescale))
        return (*head, PackedImages.from_images(cols[5], self.R, self.S, self.mean, self.std, self.rescale))


def processor_settings(directory: str):
    """(R, S, mean, std, rescale) from a CLIP checkpoint's preprocessor_config.json.  Only what the device path reproduces
    exactly is accepted: bicubic resample, resize to a shortest edge, center crop, rescale, normalise, convert to RGB."""
    path = os.path.join(directory, "preprocessor_config.json")
    with open(path) as f:
        cfg = json.load(f)
    expect = {"do_resize": True, "do_center_crop": True, "do_rescale": True, "do_normalize": True, "do_convert_rgb": True,
              "resample": 3}
    for key, want in expect.items():
        if key in cfg and cfg[key] != want:
            raise ValueError(f"{path}: {key} = {cfg[key]!r} is not supported (only {want!r}: bicubic CLIP preprocessing)")
    size, crop = cfg.get("size", 224), cfg.get("crop_size", 224)
    if isinstance(size, dict):
        if set(k for k, v in size.items() if v is not None) != {"shortest_edge"}:
            raise ValueError(f"{path}: size {size} is not supported (only a shortest_edge resize)")
        size = size["shortest_edge"]
    if isinstance(crop, dict):
        if crop.get("height") != crop.get("width"):
            raise ValueError(f"{path}: only square crops are supported, got {crop}")
        crop = crop["height"]
    R, S = int(size), int(crop)
    if S > R:
        raise ValueError(f"{path}: a crop of {S} from a shortest edge of {R} needs padding, which is not supported")
    return (R, S, tuple(cfg.get("image_mean", CLIP_MEAN)), tuple(cfg.get("image_std", CLIP_STD)),
            float(cfg.get("rescale_factor", RESCALE)))
