"""Cost of the focal loss (K13, --focal_gamma).  Two measurements at one commit:

  1. d2r_ce_focal_fwd / d2r_ce_focal_bwd (gamma = 2) next to d2r_ce_mix_fwd / d2r_ce_mix_bwd at B = 32, C = 3 on the same inputs (two
     labels per row, class weights, label smoothing 0.1): each launch between two HIP events of its own on the launching stream, the
     four variants alternating launch by launch so that drift hits all alike.  The median, the minimum and the 90th percentile of N
     launches per variant (an interval between two events holds the launch's own overhead too, so these are upper bounds of the
     kernels' times; all four are single-workgroup latency kernels).
  2. the C2 training step of bench.py (batch 32, text length 128, 224 x 224 images, 12 + 12 layers, fp16, eager) with focal_gamma = 2
     and with focal_gamma = 0 - the calls of a build without the option - on one model, the two alternating step by step: wall-clock
     time per step between two device synchronisations, median and minimum.

The last line is JSON.

    python tests/probes/focal_cost.py > profiles/focal_cost.log
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

B = int(os.environ.get("D2R_PROBE_BATCH", "32"))
C = int(os.environ.get("D2R_PROBE_CLASSES", "3"))
LAUNCHES = int(os.environ.get("D2R_PROBE_LAUNCHES", "300"))
STEPS = int(os.environ.get("D2R_PROBE_STEPS", "40"))
WARMUP = 20
GAMMA, EPS = 2.0, 0.1

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
res = {"B": B, "C": C, "launches": LAUNCHES, "steps": STEPS, "focal_gamma": GAMMA, "label_smoothing": EPS}

# ---- 1. the kernels alone -------------------------------------------------------------------------------
logits = (4.0 * torch.randn(B, C, generator=g)).to(dev)
y, y2 = torch.randint(0, C, (B,), generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)
lam = torch.rand(B, generator=g).to(dev)
w = (0.25 + 2.0 * torch.rand(C, generator=g)).to(dev)
loss, dloss, dlogits = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty(B, C, device=dev)
head = (logits.data_ptr(), y.data_ptr(), y2.data_ptr(), lam.data_ptr(), w.data_ptr(), EPS)
variants = [
    ("d2r_ce_mix_fwd", lambda: F._lib.call("d2r_ce_mix_fwd", *head, B, C, loss.data_ptr(), F._stream())),
    ("d2r_ce_focal_fwd", lambda: F._lib.call("d2r_ce_focal_fwd", *head, GAMMA, B, C, loss.data_ptr(), F._stream())),
    ("d2r_ce_mix_bwd", lambda: F._lib.call("d2r_ce_mix_bwd", *head, B, C, dloss.data_ptr(), dlogits.data_ptr(), F._stream())),
    ("d2r_ce_focal_bwd", lambda: F._lib.call("d2r_ce_focal_bwd", *head, GAMMA, B, C, dloss.data_ptr(), dlogits.data_ptr(), F._stream())),
]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


events = {name: [] for name, _ in variants}
for k in range(WARMUP + LAUNCHES):
    n = k % len(variants)
    for name, fn in variants[n:] + variants[:n]:
        ev = timed(fn)
        torch.cuda.synchronize()  # one variant in flight at a time
        if k >= WARMUP:
            events[name].append(ev)
for name, evs in events.items():
    us = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
    med = statistics.median(us)
    res[name] = {"median_us": round(med, 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2)}
    print(f"{name} (B = {B}, C = {C}): median {med:.2f} us, min {us[0]:.2f} us, p90 {us[int(0.9 * len(us))]:.2f} us over {len(us)} launches")
del events

# ---- 2. the C2 step with and without the focal term ---------------------------------------------------------
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
                      VisionConfig(num_hidden_layers=a.layers, image_size=a.image_size, patch_size=a.patch),
                      TextConfig(num_hidden_layers=a.layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), num_classes=a.classes)
model.to(dev).set_compute_dtype(dtype).train()
store = ParamStore(model, dtype)
opt = FusedAdamW(store, lr=3e-5)
if dtype == torch.float16:
    opt.enable_loss_scaling()
total = 2 * (WARMUP + STEPS) + 8
sched = LinearWarmupSchedule(opt, 0.01 * total, total)
ids, mask, seg, labels, images = bench.synthetic_batch(B, a.seq, a.image_size, dev, seed=0, classes=a.classes)


def step(gamma):
    model.focal_gamma = gamma  # what UnimoModelF reads from args.focal_gamma; 0: the calls of a build without the option
    loss, _ = model(ids, mask, seg, labels, images)
    opt.backward(loss)
    opt.step()
    sched.step()
    opt.zero_grad()


times = {0.0: [], GAMMA: []}
for k in range(WARMUP + STEPS):
    for gamma in ((0.0, GAMMA) if k % 2 == 0 else (GAMMA, 0.0)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(gamma)
        torch.cuda.synchronize()
        if k >= WARMUP:
            times[gamma].append(1e3 * (time.perf_counter() - t0))
for gamma, name in ((0.0, "step_without"), (GAMMA, "step_with")):
    ms = sorted(times[gamma])
    res[name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3)}
    print(f"C2 step with focal_gamma = {gamma:g} ({a.dtype}, eager): median {statistics.median(ms):.3f} ms, min {ms[0]:.3f} ms over {len(ms)} steps")
res["step_added_ms_median"] = round(res["step_with"]["median_ms"] - res["step_without"]["median_ms"], 3)
res["step_added_percent_median"] = round(100.0 * res["step_added_ms_median"] / res["step_without"]["median_ms"], 2)
print(f"focal_gamma = {GAMMA:g} adds {res['step_added_ms_median']:.3f} ms to the median step ({res['step_added_percent_median']:.2f} %)")
print(json.dumps(res))
