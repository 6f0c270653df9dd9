"""Cost of the augmenting gather next to the plain one: d2r_clip_cache_gather and d2r_clip_cache_augment at B = 32, S = 224 on the
same cache, indices and output buffer, each launch between two HIP events of its own on the launching stream, the two kernels
alternating launch by launch so that drift hits both alike.  The boxes are Augmenter(224, 0.5, 0.5) draws, new ones per launch; the
indices are random rows of a cache larger than the Infinity Cache, new ones per launch too.  After a warm-up it prints the median,
the minimum and the 90th percentile of N launches per kernel, their ratio and the bytes per second that the medians amount to (an
interval between two events holds the launch's own overhead too, so these are upper bounds of the kernels' times); the last line
is JSON.  The kernels' own durations come from a run under rocprofv3 of its own:

    python tests/probes/augment_cost.py > profiles/augment_cost.log
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o augment -- python tests/probes/augment_cost.py
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

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
cache = torch.randint(0, 256, (ROWS, I.cache_row_bytes(S)), dtype=torch.uint8, generator=g).to(dev)
lut = torch.from_numpy(I.normalize_table()).to(dev)
out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
aug = Augmenter(S, 0.5, 0.5, seed=0)
sets = []
for _ in range(WARMUP + LAUNCHES):
    h_idx = torch.randint(0, ROWS, (B,), generator=g).pin_memory()
    h_aug = aug.draw(B).pin_memory()
    sets.append((h_idx, h_idx.to(dev), h_aug, h_aug.to(dev)))
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


events = {"gather": [], "augment": []}
for k, (h_idx, idx, h_aug, d_aug) in enumerate(sets):
    pair = (("gather", lambda: I.clip_cache_gather(cache, h_idx, idx, S, lut, out=out)),
            ("augment", lambda: I.clip_cache_augment(cache, h_idx, idx, h_aug, d_aug, S, lut, out=out)))
    for name, fn in (pair if k % 2 == 0 else pair[::-1]):
        ev = timed(fn)
        if k >= WARMUP:
            events[name].append(ev)
    torch.cuda.synchronize()  # one launch in flight at a time: an interval never holds another kernel's tail

res = {"B": B, "S": S, "cache_rows": ROWS, "launches": LAUNCHES, "crop_scale": 0.5, "flip_p": 0.5,
       "bytes_read": B * 3 * S * S, "bytes_written": 4 * B * 3 * S * S}
for name, evs in events.items():
    us = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
    med = statistics.median(us)
    res[name] = {"median_us": round(med, 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2),
                 "GBps_at_median": round((res["bytes_read"] + res["bytes_written"]) / med / 1e3, 1)}
    print(f"{name}: median {med:.2f} us, min {us[0]:.2f} us, p90 {us[int(0.9 * len(us))]:.2f} us over {len(us)} launches; "
          f"{res[name]['GBps_at_median']} GB/s at the median ({res['bytes_read'] / 1e6:.1f} MB read, {res['bytes_written'] / 1e6:.1f} MB written)")
res["augment_over_gather"] = round(res["augment"]["median_us"] / res["gather"]["median_us"], 3)
print(f"augment / gather = {res['augment_over_gather']:.3f} (medians)")
print(json.dumps(res))
