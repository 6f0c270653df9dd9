"""Cost of per-parameter AdamW hyper-parameters (d2r_adamw_step_table) at the C2 parameter count, bf16 shadow: the optimiser
launches alone over the flat buffers of the C2 model (12 + 12 encoder layers, 224 px images in 16 px patches), in ONE process on
the SAME weight, gradient, moment and shadow buffers:

    a   the launch per group of the plain step (4 launches)
    a2  the same again, an optimiser object of its own: the run-to-run spread of (a)
    b   the table launch with one segment per group, scale 1 (the same arithmetic as a, the lookup always on its uniform path)
    c   the table launch with the real table of --layer_lr_decay 0.8 --wd_exempt_1d

Blocks of STEPS steps between two device events, the four variants in the order a, b, c, a2 in even blocks and reversed in odd
ones, so that drift and whatever a predecessor leaves in the caches hit all alike.  Prints the median and the range of the per-block
mean step time of each, the ratios to (a) and the achieved bytes per second (30 bytes per element); the last line is JSON."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.params import FusedAdamW, ParamStore

STEPS = int(os.environ.get("D2R_PROBE_STEPS", "50"))    # steps per block
BLOCKS = int(os.environ.get("D2R_PROBE_BLOCKS", "12"))  # blocks per variant
LAYERS = int(os.environ.get("D2R_PROBE_LAYERS", "12"))
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = M.UnimoModelF(default_args(DR_step=3), VisionConfig(num_hidden_layers=LAYERS, image_size=224, patch_size=16),
                      TextConfig(num_hidden_layers=LAYERS)).to(dev)
model.set_compute_dtype(torch.bfloat16).train()
store = ParamStore(model, torch.bfloat16)
store.flat_g.copy_(torch.randn(store.n, device=dev) * 1e-3)
opts = dict(a=FusedAdamW(store, lr=1e-5), a2=FusedAdamW(store, lr=1e-5), b=FusedAdamW(store, lr=1e-5),
            c=FusedAdamW(store, lr=1e-5, layer_lr_decay=0.8, decay_exempt_1d=True))
opts["b"]._set_table([(pg["range"][1], 1.0, pg["weight_decay"], i) for i, pg in enumerate(opts["b"].param_groups)])
for o in opts.values():  # the same buffers: the only difference is the launch
    o.m, o.v = opts["a"].m, opts["a"].v
order = ["a", "b", "c", "a2"]
times = {k: [] for k in order}
for k in order:
    for _ in range(5):
        opts[k].step()
torch.cuda.synchronize()
for blk in range(BLOCKS):
    for k in (order if blk % 2 == 0 else order[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            opts[k].step()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / STEPS)
med = {k: statistics.median(v) for k, v in times.items()}
print(f"bf16: {store.n / 1e6:.1f} M elements ({store.live_numel() / 1e6:.1f} M live); segments: b {len(opts['b'].table)}, "
      f"c {len(opts['c'].table)}; {STEPS} steps x {BLOCKS} blocks per variant, order reversed every other block", flush=True)
for k in order:
    print(f"  {k:2s}: {med[k]:.4f} ms [{min(times[k]):.4f}, {max(times[k]):.4f}]  x{med[k] / med['a']:.4f} of a  "
          f"{30.0 * store.n / med[k] / 1e9:.2f} TB/s", flush=True)
print(json.dumps(dict(elements=store.n, live=store.live_numel(), segments_b=len(opts["b"].table), segments_c=len(opts["c"].table),
                      steps=STEPS, blocks=BLOCKS, median_ms=med, min_max_ms={k: [min(v), max(v)] for k, v in times.items()})))
