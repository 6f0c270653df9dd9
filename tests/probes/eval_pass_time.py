"""Time MSDTrainer.evaluate() over the synthetic dev split (2048 samples, batch 32, the default 12+12-layer bf16 model) with the
batches materialised on the host beforehand, so the pass measures the evaluation loop and not the synthetic-data generator.
Two warm-up passes, then five timed ones; the last line is JSON.  Compare two builds by alternating fresh processes:

    python tests/probes/eval_pass_time.py <tag>
"""
import json
import logging
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.data import SyntheticMSDDataset, make_loader
from d2r_amd.train import MSDTrainer

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
torch.manual_seed(0)
args = default_args(compute_dtype=torch.bfloat16, device="cuda:0", num_epochs=1, batch_size=32, save_path=None)
model = M.UnimoModelF(args, VisionConfig(num_hidden_layers=12, image_size=224, patch_size=32),
                      TextConfig(num_hidden_layers=12, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
ds = SyntheticMSDDataset(2048, 128, 224, 3, seed=2, num_image_tokens=50)
batches = [tuple(t.pin_memory() for t in b) for b in make_loader(ds, 32, False, 8)]
logger = logging.getLogger("eval-time")
logger.setLevel(logging.WARNING)
tr = MSDTrainer(dev_data=batches, model=model, args=args, logger=logger, writer=None)
times = []
for i in range(7):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = tr.evaluate(1)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
timed = times[2:]  # two warm-up passes
print(json.dumps({"tag": tag, "passes_s": [round(t, 4) for t in times], "median_s": round(statistics.median(timed), 4),
                  "min_s": round(min(timed), 4), "max_s": round(max(timed), 4), "f_score": res["f_score"], "loss": res["loss"]}))
