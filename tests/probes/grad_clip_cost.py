"""Cost of gradient clipping (FusedAdamW(max_grad_norm=...)) at the C2 parameter count: the optimiser step alone, over the flat
buffers of the C2 model (12 + 12 encoder layers, 224 px images in 16 px patches), with clipping off and on, in the bf16 mode
(clipping adds the norm pass) and the fp16 mode (the norm pass replaces the overflow scan).  Gradients are random, written
straight into the flat buffer.  Prints the mean step time from events per configuration; the per-kernel times come from a run
under rocprofv3 of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o clip -- python tests/probes/grad_clip_cost.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.params import FusedAdamW, ParamStore

STEPS = int(os.environ.get("D2R_PROBE_STEPS", "20"))
dev = torch.device("cuda:0")
for dtype in (torch.bfloat16, torch.float16):
    torch.manual_seed(0)
    model = M.UnimoModelF(default_args(DR_step=3), VisionConfig(num_hidden_layers=12, image_size=224, patch_size=16),
                          TextConfig(num_hidden_layers=12)).to(dev)
    model.set_compute_dtype(dtype).train()
    store = ParamStore(model, dtype)
    g = torch.randn(store.n, device=dev) * 1e-3
    for clip in (None, 1.0, None):  # off again at the end: the two "off" rows bracket the "on" row against drift
        opt = FusedAdamW(store, lr=1e-5, max_grad_norm=clip)
        if dtype == torch.float16:
            opt.enable_loss_scaling()
        store.flat_g.copy_(g * opt.loss_scale)
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            opt.step()
        e1.record()
        torch.cuda.synchronize()
        norm = float(opt.last_grad_norm) if clip else float("nan")
        print(f"{str(dtype)[6:]} clip={clip}: {store.n / 1e6:.1f} M elements, optimiser step {e0.elapsed_time(e1) / STEPS:.3f} ms, "
              f"grad_norm {norm:.4f}", flush=True)
    del model, store, opt, g
    torch.cuda.empty_cache()
