"""CLIP preprocessing on the device vs in the loader workers.

  --kernel-only : d2r_clip_preprocess on one batch of 32 mixed 0.3-2 MP images, 50 times (run it under
                  `rocprofv3 --kernel-trace --stats` for the kernel times)
  (default)     : event-timed kernel pair and host-to-device copy of the packed bytes for that batch, then loader samples/s over a
                  directory of JPEGs of the same sizes: MSDDataset + ClipCollate + the device preprocessing (the trainer's
                  path) vs the reference's recipe (CLIPImageProcessor per sample in the workers), at 4 / 8 / 15 workers.

    python tests/probes/clip_preprocess_probe.py [--kernel-only] [--images 480] [--workers 4,8,15]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from d2r_amd import image as I  # noqa: E402
from d2r_amd.data import MSDDataset  # noqa: E402
from make_clip_golden import fixture_image  # noqa: E402


def sizes(n, seed=0):
    """n (H, W) pairs of 0.3-2 MP, aspect 3:4 .. 16:9 either way."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        mp = rng.uniform(0.3e6, 2.0e6)
        aspect = rng.uniform(0.75, 16 / 9)
        h = int(np.sqrt(mp / aspect))
        w = int(mp / h)
        out.append((h, w) if rng.integers(2) else (w, h))
    return out


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


class ProcessorDataset(MSDDataset):
    """The reference's recipe (processor/dataset.py:87-95): CLIPImageProcessor on every sample in the worker."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        from transformers import CLIPImageProcessor
        self.proc = CLIPImageProcessor()

    def __getitem__(self, idx):
        from PIL import Image
        ids, mask, seg = self.encode(self.texts[idx])
        with Image.open(os.path.join(self.img_path, self.imgs[idx])) as im:
            pv = self.proc(images=im.convert("RGB"), return_tensors="pt")["pixel_values"].squeeze(0)
        return ids, mask, seg, torch.ones(50, dtype=torch.long), torch.tensor(self.labels[idx]), pv


class _Tok:  # whitespace tokenizer: the probe measures images, not text
    def tokenize(self, t):
        return t.split()

    def convert_tokens_to_ids(self, toks):
        return [1] * len(toks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--images", type=int, default=480)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", default="4,8,15")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    imgs = [fixture_image(1000 + i, h, w) for i, (h, w) in enumerate(sizes(a.batch))]
    packed = I.PackedImages.from_images(imgs, 224, 224).pin_memory()
    mb = packed.pixels.numel() / 1e6
    if a.kernel_only:
        for _ in range(50):
            packed.to_pixel_values(dev)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "batch": a.batch, "packed_MB": round(mb, 1)}))
        return
    h_desc, h_tab = packed.host_parts()
    pixels, meta = packed.pixels.to(dev), packed.meta.to(dev)
    nd = a.batch * I.DESC_DTYPE.itemsize
    lut = torch.from_numpy(I.normalize_table()).to(dev)
    out = torch.empty(a.batch, 3, 224, 224, device=dev)
    kern = event_ms(lambda: I.clip_preprocess(pixels, h_desc, meta[:nd], h_tab, meta[nd:].view(torch.int32), 224, lut, out=out), 50)
    dst = torch.empty_like(packed.pixels, device=dev)
    h2d = event_ms(lambda: dst.copy_(packed.pixels, non_blocking=True), 20)
    t = time.perf_counter()
    for _ in range(5):
        I.PackedImages.from_images(imgs, 224, 224)
    collate_ms = (time.perf_counter() - t) / 5 * 1e3
    res = {"batch": a.batch, "packed_MB": round(mb, 1), "kernel_pair_ms_events": round(kern, 4), "h2d_ms": round(h2d, 3),
           "h2d_GBps": round(mb / h2d, 1), "collate_pack_ms": round(collate_ms, 1)}
    print(json.dumps(res), flush=True)

    from PIL import Image
    with tempfile.TemporaryDirectory() as d:
        samples = []
        for i, (h, w) in enumerate(sizes(a.images, seed=1)):
            Image.fromarray(fixture_image(2000 + i, h, w)).save(os.path.join(d, f"p{i}.jpg"), quality=90)
            samples.append({"id": f"p{i}", "text": "a b c", "emotion_label": i % 3})
        with open(os.path.join(d, "all.json"), "w") as f:
            json.dump(samples, f)
        for nw in [int(x) for x in a.workers.split(",")]:
            for kind in ("gpu", "cpu"):
                if kind == "gpu":
                    ds = MSDDataset(os.path.join(d, "all.json"), d, _Tok(), max_seq=64)
                    dl = DataLoader(ds, batch_size=a.batch, num_workers=nw, pin_memory=True, collate_fn=I.ClipCollate(224, 224),
                                    persistent_workers=True, prefetch_factor=4)
                else:
                    ds = ProcessorDataset(os.path.join(d, "all.json"), d, _Tok(), max_seq=64)
                    dl = DataLoader(ds, batch_size=a.batch, num_workers=nw, pin_memory=True, persistent_workers=True, prefetch_factor=4)
                for epoch in range(2):  # epoch 0 starts the workers
                    t = time.perf_counter()
                    n = 0
                    for batch in dl:
                        x = batch[5].to_pixel_values(dev) if kind == "gpu" else batch[5].to(dev, non_blocking=True)
                        n += x.shape[0]
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t
                print(json.dumps({"loader": kind, "workers": nw, "samples_per_s": round(n / dt, 1)}), flush=True)
                del dl


if __name__ == "__main__":
    main()
