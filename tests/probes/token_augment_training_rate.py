"""Training samples/s of `python -m d2r_amd.run --cache_dataset device` with and without --aug_token_delete 0.1 --aug_token_mask 0.1,
on augment_training_rate.py's image set, window and command (the default model, batch 32, 4 workers, an epoch of 5 steps; the
trainer's clock covers epochs >= 2 and stops across evaluation).  The runs alternate, `--repeats` of each; one JSON line per run, then
one line with the median per configuration.  With --baseline_tree DIR (a built checkout of another commit, the parent's for instance)
that tree's cached run on the same files alternates with the two.

    python tests/probes/token_augment_training_rate.py [--epochs 6] [--repeats 3] [--baseline_tree DIR] >> profiles/token_augment_cost.log
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cache_loader_rate as R  # noqa: E402
from augment_training_rate import rate_in  # noqa: E402

FLAGS = ["--aug_token_delete", "0.1", "--aug_token_mask", "0.1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=320, help="generated training images; the first 5 * batch are trained on")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=6, help="5 * (epochs - 1) timed steps")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline_tree", default=None, help="a built checkout of another commit: its cached run is measured too")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        data, img, vocab = R.make_dir(os.path.join(d, "ds"), a.images, 32)
        with open(os.path.join(data, "train.json")) as f:
            samples = json.load(f)
        with open(os.path.join(data, "train.json"), "w") as f:
            json.dump(samples[:5 * a.batch], f)
        cached = ["--data_path", data, "--img_path", img, "--bert_name", vocab, "--cache_dataset", "device"]
        runs = [("device cache", R.ROOT, cached), ("device cache, " + " ".join(FLAGS), R.ROOT, cached + FLAGS)]
        if a.baseline_tree:
            runs.insert(0, ("device cache, baseline tree", os.path.abspath(a.baseline_tree), cached))
        rates = {name: [] for name, _, _ in runs}
        for rep in range(a.repeats):
            for name, tree, extra in runs:
                res = rate_in(tree, os.path.join(d, "out"), a.epochs, extra)
                rates[name].append(res["samples_per_s"])
                print(json.dumps({"what": "training, epochs >= 2", "loader": name, "repeat": rep, "epochs": a.epochs, **res}), flush=True)
        print(json.dumps({"what": "training, epochs >= 2, median samples/s of the repeats",
                          **{name: statistics.median(v) for name, v in rates.items()}}), flush=True)


if __name__ == "__main__":
    main()
