"""Writes tests/golden/clip_preprocess.npz: what transformers' CLIPImageProcessor (PIL backend, CLIP defaults: bicubic resize to
the shortest edge S, S x S center crop, rescale 1/255, OpenAI mean / std) makes of a dozen synthetic images.

The input images are not stored: ``fixture_image`` regenerates them from integer seeds with numpy's PCG64 and integer arithmetic
only, identically on every machine.  Stored per case: the uint8 crop after Pillow's resize (``crop_<name>``, [S, S, 3], row-delta
coded: read it with ``expected_crop``); for the cases in PIXEL_VALUE_CASES also the processor's fp32 ``pixel_values`` ([3, S, S]),
which pin the normalisation formula.  Before writing, every case's crop mapped through d2r_amd.image.normalize_table must equal
the processor's pixel_values bit for bit.

    python tests/make_clip_golden.py          (needs Pillow and transformers; the tests that read the file need neither)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "clip_preprocess.npz")

# name: (H, W, S, seed)
CASES = {
    "landscape": (480, 640, 224, 1),
    "portrait": (640, 480, 224, 2),
    "upscale": (80, 100, 224, 3),
    "identity": (224, 224, 224, 4),
    "one_taller": (225, 224, 224, 5),     # S x (S + 1)
    "width_kept": (300, 224, 224, 6),     # the horizontal pass keeps the width
    "extreme": (160, 1200, 224, 7),
    "heavy": (1500, 2000, 224, 8),
    "odd": (517, 333, 224, 9),
    "c4_odd": (999, 1601, 384, 11),
    "c4_upscale": (333, 517, 384, 12),
    "c4_one_wider": (384, 385, 384, 13),
}
PIXEL_VALUE_CASES = ("identity", "extreme")


def fixture_image(seed: int, H: int, W: int) -> np.ndarray:
    """uint8 [H, W, 3]: a diagonal gradient, a blocky texture (cells of min(H, W) / 32 pixels), single-pixel speckles and two
    saturated blocks (0 / 255 edges make the bicubic ringing clip).  Low entropy on purpose: the crops stay small in git."""
    rng = np.random.default_rng(seed)
    yy = np.arange(H, dtype=np.int64)[:, None, None]
    xx = np.arange(W, dtype=np.int64)[None, :, None]
    cc = np.arange(3, dtype=np.int64)[None, None, :]
    grad = (yy * 255 // H + xx * 255 // W + cc * 85) % 256
    c = max(4, min(H, W) // 32)
    coarse = rng.integers(0, 8, size=(H // c + 1, W // c + 1, 1), dtype=np.int64)
    img = (7 * grad) // 8 + np.repeat(np.repeat(coarse, c, 0), c, 1)[:H, :W]
    n = H * W // 2000
    img[rng.integers(0, H, n), rng.integers(0, W, n)] = rng.integers(0, 256, (n, 3))
    img[H // 4:H // 2, W // 4:W // 2] = 255
    img[H // 2:3 * H // 4, W // 2:3 * W // 4] = 0
    return img.astype(np.uint8)


def encode_crop(crop: np.ndarray) -> np.ndarray:
    """Stored form of a crop: every pixel minus its left neighbour (mod 256), which compresses far better than the pixels."""
    d = crop.copy()
    d[:, 1:] = crop[:, 1:] - crop[:, :-1]
    return d


def expected_crop(g, name: str) -> np.ndarray:
    """The uint8 crop [S, S, 3] of case `name` from the loaded fixture (inverse of encode_crop)."""
    return np.cumsum(g["crop_" + name], axis=1, dtype=np.uint8)


def main():
    from PIL import Image
    from transformers import CLIPImageProcessor
    sys.path.insert(0, ROOT)
    from d2r_amd.image import crop_origin, normalize_table, resize_shape
    table = normalize_table()
    out = {}
    for name, (H, W, S, seed) in CASES.items():
        img = fixture_image(seed, H, W)
        proc = CLIPImageProcessor(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
        pv = proc(images=Image.fromarray(img), return_tensors="np")["pixel_values"][0]
        rh, rw = resize_shape(H, W, S)
        top, left = crop_origin(rh, rw, S)
        crop = np.asarray(Image.fromarray(img).resize((rw, rh), Image.BICUBIC))[top:top + S, left:left + S]
        mine = np.stack([table[c][crop[:, :, c]] for c in range(3)])
        assert pv.dtype == np.float32 and np.array_equal(mine, pv), f"{name}: crop + table differ from the processor"
        out["crop_" + name] = encode_crop(crop)
        assert np.array_equal(expected_crop(out, name), crop)
        if name in PIXEL_VALUE_CASES:
            out["pixel_values_" + name] = pv
        print(f"{name:14s} {H:5d} x {W:5d} -> {rh} x {rw}, crop {S} at ({top}, {left})")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
