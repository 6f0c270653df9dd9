"""Cost of MixUp / CutMix (K24).  Two measurements at one commit:

  1. d2r_image_mix alone at B = 32, S = 224: each launch between two HIP events of its own on the launching stream, new descriptors
     per launch (Mixer(224, 0.8, 1.0) draws, uploaded beforehand), three variants alternating launch by launch so that drift hits
     all alike:
         mixed     every sample mixed (MixUp or CutMix, 0.5 each): two reads where the partner is needed, one write
         identity  prob = 0: every sample a copy (one read, one write) - the floor of a kernel that runs after the batch is built
         copy      torch's out.copy_(in) on the same buffers, for scale
     The median, the minimum and the 90th percentile of N launches per variant (an interval between two events holds the launch's
     own overhead too, so these are upper bounds of the kernel's time).
  2. the C2 training step of bench.py (batch 32, text length 128, 224 x 224 images, 12 + 12 layers, fp16, eager), with and without
     Mixer.apply in front of it and labels_b / mix_lam through the head, the two variants alternating step by step: wall-clock time
     per step between two device synchronisations, median and minimum.  `with` holds everything the flags add to a step: the draw on
     the host, the pinned upload, d2r_image_mix, the index_select and the mixed-label loss kernels in place of the plain ones.

The last line is JSON.

    python tests/probes/mix_cost.py > profiles/mix_cost.log
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from d2r_amd import functional as F
from d2r_amd.mix import Mixer

B = int(os.environ.get("D2R_PROBE_BATCH", "32"))
S = int(os.environ.get("D2R_PROBE_CROP", "224"))
LAUNCHES = int(os.environ.get("D2R_PROBE_LAUNCHES", "300"))
STEPS = int(os.environ.get("D2R_PROBE_STEPS", "40"))
WARMUP = 20
ALPHAS = (0.8, 1.0)

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
res = {"B": B, "S": S, "launches": LAUNCHES, "steps": STEPS, "mixup_alpha": ALPHAS[0], "cutmix_alpha": ALPHAS[1],
       "bytes_per_tensor": 4 * B * 3 * S * S}

# ---- 1. the kernel alone --------------------------------------------------------------------------------
pixels = torch.randn(B, 3, S, S, generator=g).to(dev)
out = torch.empty_like(pixels)
lib = F._lib.load()
on, off = Mixer(S, *ALPHAS, 1.0, seed=0), Mixer(S, *ALPHAS, 0.0, seed=0)
sets = []
for _ in range(WARMUP + LAUNCHES):
    h_on, h_off = on.draw(B)[0], off.draw(B)[0]
    sets.append((h_on, h_on.to(dev), h_off, h_off.to(dev)))
torch.cuda.synchronize()


def mix(h, d):
    F._lib.call("d2r_image_mix", pixels.data_ptr(), out.data_ptr(), B, S, h.data_ptr(), d.data_ptr(), F._stream())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


events = {"mixed": [], "identity": [], "copy": []}
for k, (h_on, d_on, h_off, d_off) in enumerate(sets):
    trio = [("mixed", lambda: mix(h_on, d_on)), ("identity", lambda: mix(h_off, d_off)), ("copy", lambda: out.copy_(pixels))]
    for name, fn in trio[k % 3:] + trio[:k % 3]:
        ev = timed(fn)
        torch.cuda.synchronize()  # one variant in flight at a time
        if k >= WARMUP:
            events[name].append(ev)
for name, evs in events.items():
    us = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
    med = statistics.median(us)
    res[name] = {"median_us": round(med, 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2)}
    print(f"d2r_image_mix {name}: median {med:.2f} us, min {us[0]:.2f} us, p90 {us[int(0.9 * len(us))]:.2f} us over {len(us)} launches")
del sets, events

# ---- 2. the C2 step with and without the mixer --------------------------------------------------------------
sys.argv = [sys.argv[0]]
import bench
from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.params import FusedAdamW, LinearWarmupSchedule, ParamStore

import d2r_amd
d2r_amd.configure_runtime()
a = bench.parse()
dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}[a.dtype]
torch.manual_seed(2023)
model = M.UnimoModelF(default_args(DR_step=a.dr_step, num_cells=a.num_cells),
                      VisionConfig(num_hidden_layers=a.layers, image_size=S, patch_size=a.patch),
                      TextConfig(num_hidden_layers=a.layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), num_classes=a.classes)
model.to(dev).set_compute_dtype(dtype).train()
store = ParamStore(model, dtype)
opt = FusedAdamW(store, lr=3e-5)
if dtype == torch.float16:
    opt.enable_loss_scaling()
total = 2 * (WARMUP + STEPS) + 8
sched = LinearWarmupSchedule(opt, 0.01 * total, total)
ids, mask, seg, labels, images = bench.synthetic_batch(B, a.seq, S, dev, seed=0, classes=a.classes)
mixer = Mixer(S, *ALPHAS, 1.0, seed=0)


def step(mixed):
    if mixed:
        px, y, y2, lam = mixer.apply(images, labels)
        loss, _ = model(ids, mask, seg, y, px, labels_b=y2, mix_lam=lam)
    else:
        loss, _ = model(ids, mask, seg, labels, images)
    opt.backward(loss)
    opt.step()
    sched.step()
    opt.zero_grad()


times = {False: [], True: []}
for k in range(WARMUP + STEPS):
    for mixed in ((False, True) if k % 2 == 0 else (True, False)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(mixed)
        torch.cuda.synchronize()
        if k >= WARMUP:
            times[mixed].append(1e3 * (time.perf_counter() - t0))
for mixed, name in ((False, "step_without"), (True, "step_with")):
    ms = sorted(times[mixed])
    res[name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3)}
    print(f"C2 step {name[5:]} the mixer ({a.dtype}, eager): median {statistics.median(ms):.3f} ms, min {ms[0]:.3f} ms over {len(ms)} steps")
res["step_added_ms_median"] = round(res["step_with"]["median_ms"] - res["step_without"]["median_ms"], 3)
res["step_added_percent_median"] = round(100.0 * res["step_added_ms_median"] / res["step_without"]["median_ms"], 2)
print(f"the flags add {res['step_added_ms_median']:.3f} ms to the median step ({res['step_added_percent_median']:.2f} %)")
print(json.dumps(res))
