"""--cache_dataset device: what the loader delivers with and without the device cache.

Generates a directory of JPEGs of 0.3-2 MP (MVSA-style JSON splits, a tiny BERT vocabulary) and reports, one JSON line each:
  1. samples/s of the plain loader (MSDDataset + ClipCollate + the device preprocessing: the trainer's path), in both
     --image_decode modes at 4 and 8 workers, second epoch (the first starts the workers);
  2. the prefill time of the device cache, per decode mode;
  3. samples/s of CachedLoader alone (index batches -> gather kernels), synchronised at the end of each epoch;
  4. training samples/s of `python -m d2r_amd.run` over epochs >= 2 with and without --cache_dataset device, and on synthetic data
     of the same shape (the default model, batch 32; an epoch is 5 steps, the trainer's clock starts after 5 warm-up steps, i.e. with
     epoch 2, and stops across evaluation).

    python tests/probes/cache_loader_rate.py [--images 320] [--workers 4,8] [--epochs 30] [--skip-loaders] [--skip-training]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from clip_preprocess_probe import sizes  # noqa: E402
from d2r_amd import image as I  # noqa: E402
from d2r_amd.cache import CachedLoader, DeviceDatasetCache, prefill, release_workers  # noqa: E402
from d2r_amd.data import MSDDataset, make_loader  # noqa: E402
from make_clip_golden import fixture_image  # noqa: E402
from test_clip_data import TEXTS, VOCAB  # noqa: E402


def make_dir(root, n_train, n_eval):
    from PIL import Image
    os.makedirs(os.path.join(root, "img"))
    os.makedirs(os.path.join(root, "bert"))
    with open(os.path.join(root, "bert", "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    samples = []
    for i, (h, w) in enumerate(sizes(n_train + 2 * n_eval, seed=1)):
        Image.fromarray(fixture_image(2000 + i, h, w)).save(os.path.join(root, "img", f"p{i}.jpg"), quality=90)
        samples.append({"id": f"p{i}", "text": TEXTS[i % len(TEXTS)], "emotion_label": i % 3})
    Image.fromarray(fixture_image(99, 250, 260)).save(os.path.join(root, "img", "inf.png"))
    parts = (("train.json", samples[:n_train]), ("dev.json", samples[n_train:n_train + n_eval]), ("test.json", samples[n_train + n_eval:]))
    for name, part in parts:
        with open(os.path.join(root, name), "w") as f:
            json.dump(part, f)
    return root, os.path.join(root, "img"), os.path.join(root, "bert")


def epoch_rate(loader, dev, epochs):
    """samples/s of every epoch: each ends in a device synchronise."""
    rates = []
    for _ in range(epochs):
        t, n = time.perf_counter(), 0
        for batch in loader:
            x = batch[5] if isinstance(batch[5], torch.Tensor) else batch[5].to_pixel_values(dev)
            n += x.shape[0]
        torch.cuda.synchronize()
        rates.append(round(n / (time.perf_counter() - t), 1))
    return rates


def training_rate(out, epochs, extra):
    cmd = [sys.executable, "-m", "d2r_amd.run", "--num_epochs", str(epochs), "--batch_size", "32", "--num_workers", "4",
           "--save_path", out + "/", *extra]
    t = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))
    log = r.stdout + r.stderr
    if r.returncode != 0:
        raise RuntimeError(log[-3000:])
    m = re.search(r"training throughput: ([0-9.]+) samples/s", log)
    prefills = [float(x) for x in re.findall(r"prefill ([0-9.]+) s", log)]
    return {"samples_per_s": float(m.group(1)), "wall_s": round(time.perf_counter() - t, 1), "prefill_s": prefills}


def loader_rates(a, loader, dev):
    for decode in ("host", "device"):
        for nw in [int(x) for x in a.workers.split(",")]:
            dl = loader(decode, nw)
            rates = epoch_rate(dl, dev, 3)
            release_workers(dl)
            print(json.dumps({"what": "plain loader", "image_decode": decode, "workers": nw, "images": a.images,
                              "samples_per_s_epochs": rates}), flush=True)
    for decode in ("host", "device"):
        dl = loader(decode, 4)
        cache = DeviceDatasetCache.for_loader(dl, dev, "train")
        seconds = prefill(dl, cache, split="train")
        print(json.dumps({"what": "prefill", "image_decode": decode, "workers": 4, "images": a.images, "seconds": round(seconds, 2),
                          "samples_per_s": round(a.images / seconds, 1), "bytes_held": cache.nbytes}), flush=True)
    cached = CachedLoader(dl, cache)
    rates = epoch_rate(cached, dev, 30)
    print(json.dumps({"what": "CachedLoader alone", "batch": a.batch, "images_per_epoch": len(cached) * a.batch,
                      "samples_per_s_epochs_first3": rates[:3], "samples_per_s_median_of_30": sorted(rates)[len(rates) // 2]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=320)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", default="4,8")
    ap.add_argument("--epochs", type=int, default=30, help="of the training runs: 5 * (epochs - 1) timed steps")
    ap.add_argument("--skip-loaders", action="store_true")
    ap.add_argument("--skip-training", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from transformers import BertTokenizer
    with tempfile.TemporaryDirectory() as d:
        data, img, vocab = make_dir(os.path.join(d, "ds"), a.images, 32)
        tok = BertTokenizer.from_pretrained(vocab, do_lower_case=True)

        def loader(decode, nw, split="train", shuffle=True):
            ds = MSDDataset(os.path.join(data, split + ".json"), img, tok, max_seq=128, image_decode=decode)
            return make_loader(ds, a.batch, shuffle, nw, drop_last=shuffle, collate_fn=I.ClipCollate(224, 224, image_decode=decode))

        if not a.skip_loaders:
            loader_rates(a, loader, dev)
        if a.skip_training:
            return
        # an epoch of 5 steps: the trainer's clock starts after 5 warm-up steps, i.e. it covers epochs >= 2 only
        with open(os.path.join(data, "train.json")) as f:
            samples = json.load(f)
        with open(os.path.join(data, "train.json"), "w") as f:
            json.dump(samples[:5 * a.batch], f)
        real = ["--data_path", data, "--img_path", img, "--bert_name", vocab]
        for name, extra in (("plain loader, host decode", real), ("device cache", real + ["--cache_dataset", "device"]),
                            ("plain loader, device decode", real + ["--image_decode", "device"]),
                            ("synthetic data", ["--train_samples", str(5 * a.batch), "--eval_samples", "32"])):
            res = training_rate(os.path.join(d, "out"), a.epochs, extra)
            print(json.dumps({"what": "training, epochs >= 2", "loader": name, "workers": 4, "epochs": a.epochs, **res}), flush=True)


if __name__ == "__main__":
    main()
