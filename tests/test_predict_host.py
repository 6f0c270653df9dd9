"""Host side of prediction from a checkpoint (no GPU): MSDDataset's optional labels and ids, the --only_test / --write_path
argument checks of d2r_amd.run, and the JSON Lines writer of MSDTrainer.predict."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataset_dir(tmp_path, labelled):
    from test_clip_data import make_msd_dir
    data, img, vocab = make_msd_dir(str(tmp_path / "ds"), n=6)
    path = os.path.join(data, "test.json")
    with open(path) as f:
        samples = json.load(f)
    for i, s in enumerate(samples):
        if i not in labelled:
            del s["emotion_label"]
    with open(path, "w") as f:
        json.dump(samples, f)
    return path, img, vocab, samples


def test_dataset_optional_labels_and_ids(tmp_path):
    pytest.importorskip("transformers")
    from d2r_amd.data import MSDDataset
    path, img, vocab, samples = _dataset_dir(tmp_path, labelled={1})
    ds = MSDDataset(path, img, vocab, 16, labels_optional=True)
    assert ds.ids == [str(s["id"]) for s in samples]
    assert ds.labels == [-1, samples[1]["emotion_label"], -1]
    assert [int(ds[i][4]) for i in range(len(ds))] == ds.labels
    with pytest.raises(KeyError):  # the default still insists on a label
        MSDDataset(path, img, vocab, 16)


def test_dataset_labelled_json_unchanged_by_labels_optional(tmp_path):
    pytest.importorskip("transformers")
    from d2r_amd.data import MSDDataset
    path, img, vocab, samples = _dataset_dir(tmp_path, labelled={0, 1, 2})
    a, b = MSDDataset(path, img, vocab, 16), MSDDataset(path, img, vocab, 16, labels_optional=True)
    assert a.labels == b.labels == [s["emotion_label"] for s in samples]
    assert a.ids == b.ids and a.imgs == [i + ".jpg" for i in a.ids]


def _run(args, env_extra=None):
    env = dict(os.environ, PYTHONPATH=ROOT, **(env_extra or {}))
    env.pop("LOCAL_RANK", None)
    return subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "d2r_amd.run", *args], cwd=ROOT, env=env,
                          capture_output=True, text=True)


def test_only_test_needs_load_path():
    r = _run(["--only_test"])
    assert r.returncode != 0 and "--only_test needs --load_path" in r.stderr


@pytest.mark.parametrize("flags", [["--only_test", "--load_path", "x.pth"], ["--write_path", "p.jsonl"]], ids=["only_test", "write_path"])
def test_prediction_flags_are_single_process(monkeypatch, flags):
    from d2r_amd import dp, run
    called = []
    orig = dp.init_process_group_from_env
    monkeypatch.setattr(dp, "init_process_group_from_env", lambda *a, **k: called.append(1) or orig(*a, **k))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        run.main(flags)
    assert not called  # refused before any process group / device work


def test_prediction_flags_refused_under_world_size_2_in_a_subprocess():
    r = _run(["--write_path", "p.jsonl"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "single process" in r.stderr


def test_jsonl_writer_round_trips_fp32(tmp_path):
    from d2r_amd.train import write_predictions
    g = torch.Generator().manual_seed(0)
    n = 7
    probs = torch.softmax(torch.randn(n, 3, generator=g), -1)
    probs[0] = torch.tensor([1e-45, 3.4028235e38, float.fromhex("0x1.fffffep-1")])  # subnormal, fp32 max, just below 1
    pt = torch.rand(n, 78, generator=g)
    pt[1, :5] = 0.0
    pi = torch.rand(n, 78, generator=g) * 1e-30
    preds = torch.argmax(probs, -1)
    ids = [f"id{i}" for i in range(n)]
    labels = [None, 2, 0, 1, None, 1, 0]
    path = str(tmp_path / "p.jsonl")
    write_predictions(path, ids, labels, preds, probs, pt, pi)
    with open(path) as f:
        lines = f.read().splitlines()
    assert len(lines) == n
    for i, line in enumerate(lines):
        r = json.loads(line)
        assert list(r) == ["index", "id", "label", "pred", "probs", "paths_text", "paths_image"]
        assert r["index"] == i and r["id"] == ids[i] and r["label"] == labels[i] and r["pred"] == int(preds[i])
        for key, t in (("probs", probs), ("paths_text", pt), ("paths_image", pi)):
            back = torch.tensor(r[key], dtype=torch.float32)
            assert torch.equal(back, t[i]), key
            assert all(isinstance(v, float) for v in r[key])
