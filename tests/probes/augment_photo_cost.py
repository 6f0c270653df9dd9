"""Cost of the photometric augmentation next to the geometric one: d2r_clip_cache_augment (K21, unchanged) and
d2r_clip_cache_augment_photo (K22) at B = 32, S = 224 on the same cache, indices, boxes and output buffer, each launch between two
HIP events of its own on the launching stream, the three variants alternating launch by launch so that drift hits all alike:

    augment        d2r_clip_cache_augment
    photo          d2r_clip_cache_augment_photo with every option on (brightness, contrast, saturation 0.4, hue 0.1, grayscale 0.1,
                   erase 0.25): the statistics pass and the apply kernel
    photo_no_stats the same descriptors with every contrast factor set to 1: the apply kernel alone

The boxes are Augmenter(224, 0.5, 0.5) draws and the descriptors its draw_photo's, new ones per launch; the indices are random rows of
a cache larger than the Infinity Cache, new ones per launch too.  After a warm-up it prints the median, the minimum and the 90th
percentile of N launches per variant and their ratios to `augment` (an interval between two events holds the launch's own overhead
too - twice for the two launches of `photo` - so these are upper bounds of the kernels' times); the last line is JSON.

    python tests/probes/augment_photo_cost.py > profiles/augment_photo_cost.log
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from d2r_amd import image as I
from d2r_amd.augment import Augmenter

B = int(os.environ.get("D2R_PROBE_BATCH", "32"))
S = int(os.environ.get("D2R_PROBE_CROP", "224"))
ROWS = int(os.environ.get("D2R_PROBE_ROWS", "2048"))     # 308 MB of crops at S = 224
LAUNCHES = int(os.environ.get("D2R_PROBE_LAUNCHES", "300"))
WARMUP = 20
assert LAUNCHES >= 100
SETTINGS = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, grayscale_p=0.1, erase_p=0.25)

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
cache = torch.randint(0, 256, (ROWS, I.cache_row_bytes(S)), dtype=torch.uint8, generator=g).to(dev)
lut = torch.from_numpy(I.normalize_table()).to(dev)
out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
ws = torch.empty(I.clip_cache_augment_photo_ws_bytes(B, S) // 4, dtype=torch.float32, device=dev)
aug = Augmenter(S, 0.5, 0.5, seed=0, **SETTINGS)
sets = []
for _ in range(WARMUP + LAUNCHES):
    h_idx = torch.randint(0, ROWS, (B,), generator=g).pin_memory()
    h_aug = aug.draw(B).pin_memory()
    h_photo = aug.draw_photo(B)
    h_flat = h_photo.clone()
    h_flat[:, 1] = torch.ones(B, dtype=torch.float32).view(torch.int32)  # contrast 1: no statistics pass
    h_photo, h_flat = h_photo.pin_memory(), h_flat.pin_memory()
    sets.append((h_idx, h_idx.to(dev), h_aug, h_aug.to(dev), h_photo, h_photo.to(dev), h_flat, h_flat.to(dev)))
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


events = {"augment": [], "photo": [], "photo_no_stats": []}
for k, (h_idx, idx, h_aug, d_aug, h_photo, d_photo, h_flat, d_flat) in enumerate(sets):
    trio = [("augment", lambda: I.clip_cache_augment(cache, h_idx, idx, h_aug, d_aug, S, lut, out=out)),
            ("photo", lambda: I.clip_cache_augment_photo(cache, h_idx, idx, h_aug, d_aug, h_photo, d_photo, S, out=out, ws=ws)),
            ("photo_no_stats", lambda: I.clip_cache_augment_photo(cache, h_idx, idx, h_aug, d_aug, h_flat, d_flat, S, out=out, ws=ws))]
    for name, fn in trio[k % 3:] + trio[:k % 3]:
        ev = timed(fn)
        torch.cuda.synchronize()  # one variant in flight at a time: an interval never holds another kernel's tail
        if k >= WARMUP:
            events[name].append(ev)

res = {"B": B, "S": S, "cache_rows": ROWS, "launches": LAUNCHES, "crop_scale": 0.5, "flip_p": 0.5, **SETTINGS,
       "bytes_read": B * 3 * S * S, "bytes_written": 4 * B * 3 * S * S}
for name, evs in events.items():
    us = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
    med = statistics.median(us)
    res[name] = {"median_us": round(med, 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2)}
    print(f"{name}: median {med:.2f} us, min {us[0]:.2f} us, p90 {us[int(0.9 * len(us))]:.2f} us over {len(us)} launches")
for name in ("photo", "photo_no_stats"):
    res[name + "_over_augment"] = round(res[name]["median_us"] / res["augment"]["median_us"], 3)
    print(f"{name} / augment = {res[name + '_over_augment']:.3f} (medians)")
res["below_200_us"] = res["photo"]["median_us"] < 200.0
print(f"photo median below 0.2 ms (1 % of a 20 ms step): {res['below_200_us']}")
print(json.dumps(res))
