"""Cost of the weight EMA (FusedAdamW(ema_decay=...)) at the C2 parameter count: the optimiser launches alone, over the flat buffers
of the C2 model (12 + 12 encoder layers, 224 px images in 16 px patches), with EMA off and on in ONE process on the SAME weight,
gradient, moment and shadow buffers, alternating off / on block by block so that drift hits both alike.  Gradients are random,
written straight into the flat buffer.  Per dtype it prints the median and the spread of the per-block mean step time of both,
their ratio next to the byte ratio 38 / 30, and the achieved bytes per second; the last line is JSON.  The per-kernel times come
from a run under rocprofv3 of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ema -- python tests/probes/ema_cost.py
"""
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
BLOCKS = int(os.environ.get("D2R_PROBE_BLOCKS", "12"))  # blocks per variant, alternating
LAYERS = int(os.environ.get("D2R_PROBE_LAYERS", "12"))
dev = torch.device("cuda:0")
out = {}
for dtype in (torch.bfloat16, torch.float16):
    torch.manual_seed(0)
    model = M.UnimoModelF(default_args(DR_step=3), VisionConfig(num_hidden_layers=LAYERS, image_size=224, patch_size=16),
                          TextConfig(num_hidden_layers=LAYERS)).to(dev)
    model.set_compute_dtype(dtype).train()
    store = ParamStore(model, dtype)
    store.flat_g.copy_(torch.randn(store.n, device=dev) * 1e-3)
    off = FusedAdamW(store, lr=1e-5)
    on = FusedAdamW(store, lr=1e-5, ema_decay=0.999)
    on.m, on.v = off.m, off.v  # the same buffers: the only difference between the two is the ema stream
    times = {"off": [], "on": []}
    for name, opt in (("off", off), ("on", on)):
        for _ in range(5):
            opt.step()
    torch.cuda.synchronize()
    for _ in range(BLOCKS):
        for name, opt in (("off", off), ("on", on)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(STEPS):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / STEPS)
    med = {k: statistics.median(v) for k, v in times.items()}
    ratio = med["on"] / med["off"]
    tag = str(dtype)[6:]
    out[tag] = dict(elements=store.n, launches_per_step=len(off.param_groups), steps=STEPS, blocks=BLOCKS,
                    off_ms=med["off"], on_ms=med["on"], off_min_max=[min(times["off"]), max(times["off"])],
                    on_min_max=[min(times["on"]), max(times["on"])], ratio=ratio, byte_ratio=38.0 / 30.0,
                    off_TBps=30.0 * store.n / med["off"] / 1e9, on_TBps=38.0 * store.n / med["on"] / 1e9)
    print(f"{tag}: {store.n / 1e6:.1f} M elements, {len(off.param_groups)} launches per step; optimiser step off "
          f"{med['off']:.4f} ms [{min(times['off']):.4f}, {max(times['off']):.4f}], on {med['on']:.4f} ms "
          f"[{min(times['on']):.4f}, {max(times['on']):.4f}]; on / off = {ratio:.3f} (bytes: 38 / 30 = 1.267); "
          f"{out[tag]['off_TBps']:.2f} -> {out[tag]['on_TBps']:.2f} TB/s", flush=True)
    del model, store, off, on
    torch.cuda.empty_cache()
print(json.dumps(out))
