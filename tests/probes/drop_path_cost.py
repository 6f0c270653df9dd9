"""Cost of stochastic depth (--drop_path) on a whole training step at C2 (batch 32, 128 text tokens, 224 px images in 16 px patches:
197 image tokens, 12 + 12 encoder layers): forward + backward + AdamW of ONE model in ONE process, with

    off   set_drop_path(0): the step as it is without the flag
    on    set_drop_path(D2R_PROBE_DROP_PATH, default 0.1): layers 1..11 of each tower run the d2r_drop_path pass
    off2  set_drop_path(0) again: the run-to-run spread of (off)

Blocks of STEPS steps between two device events, the three variants in the order off, on, off2 in even blocks and reversed in odd
ones, so that drift hits all alike.  BERT dropout is D2R_PROBE_BERT_DROPOUT (default 0.1, run.py's default: the text layers then
already make the elementwise pass and only swap its kernel; with 0 they gain the pass as the vision layers do).  Prints the median
and the range of the per-block mean step time of each and the difference to (off); the last line is JSON."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import d2r_amd
from d2r_amd import functional as F
from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.params import FusedAdamW, ParamStore

STEPS = int(os.environ.get("D2R_PROBE_STEPS", "10"))   # steps per block
BLOCKS = int(os.environ.get("D2R_PROBE_BLOCKS", "8"))  # blocks per variant
RATE = float(os.environ.get("D2R_PROBE_DROP_PATH", "0.1"))
BERT_DROPOUT = float(os.environ.get("D2R_PROBE_BERT_DROPOUT", "0.1"))
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}[os.environ.get("D2R_PROBE_DTYPE", "fp16")]
B, L, S = 32, 128, 224
d2r_amd.configure_runtime()
dev = torch.device("cuda:0")
torch.manual_seed(2023)
model = M.UnimoModelF(default_args(DR_step=3), VisionConfig(num_hidden_layers=12, image_size=S, patch_size=16),
                      TextConfig(num_hidden_layers=12, hidden_dropout_prob=BERT_DROPOUT, attention_probs_dropout_prob=BERT_DROPOUT))
model.to(dev).set_compute_dtype(DTYPE).train()
store = ParamStore(model, DTYPE)
opt = FusedAdamW(store, lr=3e-5)
if DTYPE == torch.float16:
    opt.enable_loss_scaling()
F.seed_drop_path(2023, 0)
g = torch.Generator().manual_seed(0)
ids = torch.randint(1000, 30000, (B, L), generator=g)
ids[:, 0] = 101
batch = tuple(t.to(dev) for t in (ids, torch.ones(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long),
                                  torch.randint(0, 3, (B,), generator=g), torch.randn(B, 3, S, S, generator=g)))


def step():
    loss, _ = model(*batch)
    opt.backward(loss)
    opt.step()
    opt.zero_grad()
    return loss


rates = dict(off=0.0, on=RATE, off2=0.0)
order = ["off", "on", "off2"]
times = {k: [] for k in order}
for k in order:
    model.model.set_drop_path(rates[k])
    for _ in range(3):
        step()
torch.cuda.synchronize()
for blk in range(BLOCKS):
    for k in (order if blk % 2 == 0 else order[::-1]):
        model.model.set_drop_path(rates[k])
        step()  # the first step after a switch is not timed
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            loss = step()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / STEPS)
assert bool(torch.isfinite(loss))
med = {k: statistics.median(v) for k, v in times.items()}
print(f"{str(DTYPE)[6:]} C2 step (batch {B}, {L} text tokens, 197 image tokens), BERT dropout {BERT_DROPOUT:g}, drop_path {RATE:g}: "
      f"{STEPS} steps x {BLOCKS} blocks per variant, order reversed every other block", flush=True)
for k in order:
    print(f"  {k:4s}: {med[k]:.3f} ms [{min(times[k]):.3f}, {max(times[k]):.3f}]  {med[k] - med['off']:+.3f} ms against off", flush=True)
print(json.dumps(dict(dtype=str(DTYPE)[6:], bert_dropout=BERT_DROPOUT, drop_path=RATE, steps=STEPS, blocks=BLOCKS, median_ms=med,
                      min_max_ms={k: [min(v), max(v)] for k, v in times.items()})))
