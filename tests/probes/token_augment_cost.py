"""Cost of d2r_token_augment next to the three d2r_gather_rows launches it replaces: B = 32, L = 128 on a cache of a few thousand
token rows, the same indices and output buffers.  Three ways to build a batch's token tensors alternate launch by launch so that
drift hits all alike - the three gathers (ids, mask, seg), one d2r_token_augment without a continuation table and one with - each
between two HIP events of its own on the launching stream (the three gathers between ONE pair: what the call replaces).  The plans
are TokenAugmenter(0.1, 0.1, 0.05) draws, new ones per launch, uploaded before the clock; the indices are random rows, new ones per
launch too.  After a warm-up it prints the median, the minimum and the 90th percentile of N launches per way and their ratios (an
interval between two events holds the launches' own overhead too, so these are upper bounds of the kernels' times); the last line is
JSON.  The kernels' own durations come from a run under rocprofv3 of its own:

    python tests/probes/token_augment_cost.py > profiles/token_augment_cost.log
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o token_augment -- python tests/probes/token_augment_cost.py
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from d2r_amd import image as I
from d2r_amd import text_augment as T

B = int(os.environ.get("D2R_PROBE_BATCH", "32"))
L = int(os.environ.get("D2R_PROBE_SEQ", "128"))
ROWS = int(os.environ.get("D2R_PROBE_ROWS", "4511"))     # MVSA-single's posts: 3 x 4.6 MB of token rows
LAUNCHES = int(os.environ.get("D2R_PROBE_LAUNCHES", "300"))
VOCAB, MASK_ID, PAD_ID = 30522, 103, 0
WARMUP = 20
assert LAUNCHES >= 100

dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
n = rng.integers(L // 4, L + 1, ROWS)  # ragged lengths, as the synthetic set's
real = np.arange(L)[None, :] < n[:, None]
ids = np.where(real, rng.integers(1000, 30000, (ROWS, L)), PAD_ID)
ids[:, 0] = 101
ids[np.arange(ROWS), n - 1] = 102
src = [torch.from_numpy(t.astype(np.int64)).to(dev) for t in (ids, real, np.zeros((ROWS, L)))]
cont = torch.from_numpy((rng.random(VOCAB) < 0.2).astype(np.uint8)).to(dev)  # about the share of ## pieces in bert-base-uncased
out = torch.empty(3, B, L, dtype=torch.int64, device=dev)
aug = T.TokenAugmenter(0.1, 0.1, 0.05, MASK_ID, PAD_ID, VOCAB, replace_range=(1000, 30000), cont=cont.cpu().numpy(), seed=0)
g = torch.Generator().manual_seed(0)
sets = []
for _ in range(WARMUP + LAUNCHES):
    h_idx = torch.randint(0, ROWS, (B,), generator=g).pin_memory()
    h_plan = aug.draw(B, L).view(torch.int32).pin_memory()
    sets.append((h_idx, h_idx.to(dev), h_plan, h_plan.to(dev)))
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def gathers(h_idx, idx):
    for k in range(3):
        I.gather_rows(src[k], h_idx, idx, out=out[k])


events = {"three gathers": [], "token_augment": [], "token_augment, cont": []}
for k, (h_idx, idx, h_plan, plan) in enumerate(sets):
    ways = [("three gathers", lambda: gathers(h_idx, idx)),
            ("token_augment", lambda: T.token_augment(*src, h_idx, idx, h_plan, plan, None, VOCAB, MASK_ID, PAD_ID, out=out)),
            ("token_augment, cont", lambda: T.token_augment(*src, h_idx, idx, h_plan, plan, cont, VOCAB, MASK_ID, PAD_ID, out=out))]
    for name, fn in ways[k % 3:] + ways[:k % 3]:
        ev = timed(fn)
        if k >= WARMUP:
            events[name].append(ev)
        torch.cuda.synchronize()  # one way in flight at a time: an interval never holds another kernel's tail

res = {"B": B, "L": L, "cache_rows": ROWS, "launches": LAUNCHES, "delete_p": 0.1, "mask_p": 0.1, "replace_p": 0.05,
       "bytes_read": 3 * 8 * B * L, "bytes_written": 3 * 8 * B * L, "plan_bytes": 4 * B * L}
for name, evs in events.items():
    us = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
    med = statistics.median(us)
    res[name] = {"median_us": round(med, 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2)}
    print(f"{name}: median {med:.2f} us, min {us[0]:.2f} us, p90 {us[int(0.9 * len(us))]:.2f} us over {len(us)} launches "
          f"({res['bytes_read'] / 1e3:.1f} KB read, {res['bytes_written'] / 1e3:.1f} KB written)")
for name in ("token_augment", "token_augment, cont"):
    res[name + " over three gathers"] = round(res[name]["median_us"] / res["three gathers"]["median_us"], 3)
    print(f"{name} / three gathers = {res[name + ' over three gathers']:.3f} (medians)")
print(json.dumps(res))
