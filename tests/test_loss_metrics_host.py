"""Class-weighted / label-smoothed loss and per-class metrics on the host: metrics_from_confusion against get_four_metrics
(sklearn; bit-equal), the balanced class weights, the refusals of the two CLI flags (before anything touches a GPU), the three new
C-ABI symbols in the header, the library and d2r_amd._lib, and the checkpoint key set with both options on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW = ("d2r_ce_fwd_ex", "d2r_ce_bwd_ex", "d2r_confusion_add")


# ------------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------------
def _confusion(labels, preds, C):
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (np.asarray(labels), np.asarray(preds)), 1)
    return cm


def _label_sets():
    """(name, C, labels, predictions): seeded random sets for C in {2, 3, 7} x N in {1, 17, 500}, plus a class that is never
    predicted, a class absent from the labels, a class absent from both, and the all-correct case."""
    out = []
    for C in (2, 3, 7):
        for N in (1, 17, 500):
            rng = np.random.RandomState(1000 * C + N)
            out.append((f"random-C{C}-N{N}", C, rng.randint(0, C, N), rng.randint(0, C, N)))
            y, p = rng.randint(0, C, N), rng.randint(0, C, N)
            p[p == C - 1] = 0
            out.append((f"never-predicted-C{C}-N{N}", C, y, p))
            y, p = rng.randint(0, C, N), rng.randint(0, C, N)
            y[y == 0] = C - 1
            out.append((f"absent-label-C{C}-N{N}", C, y, p))
            y = rng.randint(0, C, N)
            out.append((f"all-correct-C{C}-N{N}", C, y, y.copy()))
            y, p = rng.randint(0, C - 1, N), rng.randint(0, C - 1, N)  # class C - 1 in neither: sklearn never sees it
            out.append((f"absent-class-C{C}-N{N}", C, y, p))
    return out


SETS = _label_sets()


@pytest.mark.filterwarnings("ignore::sklearn.exceptions.UndefinedMetricWarning")
@pytest.mark.parametrize("name,C,labels,preds", SETS, ids=[s[0] for s in SETS])
def test_metrics_from_confusion_is_bit_equal_to_get_four_metrics(name, C, labels, preds):
    from sklearn.metrics import precision_recall_fscore_support
    from d2r_amd.train import get_four_metrics, metrics_from_confusion
    cm = _confusion(labels, preds, C)
    got = metrics_from_confusion(cm)
    acc, recall, precision, f1 = get_four_metrics(labels.tolist(), preds.tolist(), type="weighted")
    for key, ref in (("eval_accuracy", acc), ("recall", recall), ("precision", precision), ("f_score", f1)):
        assert isinstance(got[key], float) and got[key] == float(ref), (name, key, got[key], float(ref))
    assert got["confusion"] == cm.tolist() and sum(map(sum, got["confusion"])) == len(labels)
    # per class: sklearn's per-label view over all C classes
    p, r, f, s = precision_recall_fscore_support(labels, preds, labels=list(range(C)), average=None, zero_division=0)
    assert [pc["class"] for pc in got["per_class"]] == list(range(C))
    for c, pc in enumerate(got["per_class"]):
        assert (pc["precision"], pc["recall"], pc["f1"], pc["support"]) == (float(p[c]), float(r[c]), float(f[c]), int(s[c])), (name, c)


def test_metrics_from_confusion_accepts_lists_and_tensors_and_refuses_nonsense():
    from d2r_amd.train import metrics_from_confusion
    cm = [[3, 1], [0, 2]]
    a, b = metrics_from_confusion(cm), metrics_from_confusion(torch.tensor(cm))
    assert a == b and a["eval_accuracy"] == 5 / 6
    for bad in ([[0, 0], [0, 0]], [[1, 2, 3]], [[1, -1], [0, 1]]):
        with pytest.raises(ValueError):
            metrics_from_confusion(bad)


# ------------------------------------------------------------------------------------------------------
# balanced weights, flags
# ------------------------------------------------------------------------------------------------------
def test_balanced_class_weights():
    from d2r_amd.run import balanced_class_weights
    counts = [470, 1398, 2743]  # an MVSA-like split: neutral is the minority
    N, C = sum(counts), len(counts)
    assert balanced_class_weights(counts) == [N / (C * n) for n in counts]
    assert balanced_class_weights([5, 5]) == [1.0, 1.0]
    with pytest.raises(ValueError, match=r"class\(es\) 1 "):
        balanced_class_weights([4, 0, 9])


def test_balanced_weights_come_from_the_whole_training_split(tmp_path):
    import json
    from d2r_amd.data import SyntheticMSDDataset
    from d2r_amd.run import build_parser, train_label_counts
    args = build_parser().parse_args(["--train_samples", "40", "--max_seq", "16", "--image_size", "64"])
    ds = SyntheticMSDDataset(40, 16, 64, 3, seed=1)
    labels = [int(ds[i][4]) for i in range(40)]
    assert ds.labels == labels
    assert train_label_counts(args) == np.bincount(labels, minlength=3).tolist()
    path = str(tmp_path / "train.json")
    for ys, want in (([0, 1, 1, 2, 2, 2], [1, 2, 3]), ([0, 0, 2], [2, 0, 1])):
        with open(path, "w") as f:
            json.dump([{"id": i, "text": "t", "emotion_label": y} for i, y in enumerate(ys)], f)
        assert train_label_counts(args, path) == want
    with open(path, "w") as f:
        json.dump([{"id": 0, "text": "t", "emotion_label": 5}], f)
    with pytest.raises(ValueError, match="outside"):  # a label outside [0, num_classes) is named, not counted
        train_label_counts(args, path)


def test_parse_class_weights():
    from d2r_amd.run import parse_class_weights
    assert parse_class_weights("none", 3) is None and parse_class_weights("balanced", 3) == "balanced"
    assert parse_class_weights("1,0,2.5", 3) == [1.0, 0.0, 2.5]
    for bad in ("1,2", "1,2,3,4", "1,-1,2", "0,0,0", "1,nan,1", "1,inf,1", "a,b,c", ""):
        with pytest.raises(ValueError):
            parse_class_weights(bad, 3)


@pytest.mark.parametrize("argv", [["--label_smoothing", "-0.1"], ["--label_smoothing", "1.0"], ["--class_weights", "1,2"],
                                  ["--class_weights", "1,-2,3"], ["--class_weights", "0,0,0"],
                                  ["--dp_exact", "--class_weights", "1,2,3"], ["--dp_exact", "--class_weights", "balanced"]],
                         ids=["eps-negative", "eps-one", "wrong-length", "negative-entry", "all-zero", "dp-exact-list", "dp-exact-balanced"])
def test_cli_refusals(argv, monkeypatch):
    """Refused at startup: main() exits before it initialises a process group, a device or a dataset."""
    from d2r_amd import dp, run
    monkeypatch.setattr(dp, "init_process_group_from_env", lambda: pytest.fail("the refusal must come before any set-up"))
    with pytest.raises(SystemExit) as e:
        run.main(argv + ["--device", "cpu", "--save_path", "/nonexistent/"])
    assert e.value.code not in (0, None)


def test_cli_accepts_the_flags():
    from d2r_amd.run import build_parser
    a = build_parser().parse_args([])
    assert a.label_smoothing == 0.0 and a.class_weights == "none"
    a = build_parser().parse_args(["--label_smoothing", "0.1", "--class_weights", "balanced", "--only_test", "--load_path", "x"])
    assert a.label_smoothing == 0.1 and a.class_weights == "balanced"
    a = build_parser().parse_args(["--dp_exact", "--label_smoothing", "0.2"])  # smoothing alone is fine with --dp_exact
    assert a.dp_exact and a.label_smoothing == 0.2


# ------------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_documented_exported_and_typed():
    from d2r_amd import _lib
    text = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "libd2r_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    kinds = {_lib.i32: "int", _lib.i64: "int64_t", _lib.f32: "float", _lib.vp: "pointer"}
    for name in NEW:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/d2r_hip.h"
        assert name in comments, f"{name} has no comment in the header"
        assert hasattr(lib, name), f"{name} declared but not exported"
        res, argtypes = _lib.SIGNATURES[name]
        want = ["pointer" if "*" in a else a.split()[-2] for a in (x.strip() for x in m.group(2).split(","))]
        assert kinds[res] == m.group(1) and [kinds[t] for t in argtypes] == want, (name, want)
    # the descriptor's two new fields come last, after d_pooled, in the header and in the ctypes mirror
    body = re.search(r"typedef struct \{([^}]*)\} d2r_head_desc;", hdr).group(1)
    assert re.search(r"d_pooled;\s*const float\* class_weight; float label_smoothing;\s*$", body), body[-200:]
    assert [f[0] for f in _lib.HeadDesc._fields_][-3:] == ["d_pooled", "class_weight", "label_smoothing"]
    assert _lib.HeadDesc._fields_[-1][1] is _lib.f32 and _lib.HeadDesc._fields_[-2][1] is _lib.vp


def test_host_side_refusals_need_no_gpu():
    """label_smoothing outside [0, 1) and bad confusion shapes are refused before any launch (null pointers never dereferenced)."""
    from d2r_amd import _lib
    lib = _lib.load()
    for eps in (-0.1, 1.0, float("nan")):
        assert lib.d2r_ce_fwd_ex(None, None, None, eps, 4, 3, None, None) != 0
        assert b"label_smoothing" in lib.d2r_last_error()
        assert lib.d2r_ce_bwd_ex(None, None, None, eps, 4, 3, None, None, None) != 0
    for ld, rows, C in ((3, 0, 3), (3, 4, 0), (2, 4, 3), (3, -1, 3)):
        assert lib.d2r_confusion_add(None, ld, None, rows, C, None, None) != 0
        assert b"bad shape" in lib.d2r_last_error()
    assert lib.d2r_confusion_add(None, 3, None, 4, 3, None, None) != 0 and b"null pointer" in lib.d2r_last_error()


# ------------------------------------------------------------------------------------------------------
# model
# ------------------------------------------------------------------------------------------------------
def _model(**kw):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    return M.UnimoModelF(default_args(**kw), VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                         TextConfig(num_hidden_layers=1))


def test_checkpoint_keys_do_not_change_with_the_options():
    plain, both = _model(), _model(label_smoothing=0.1, class_weights=[2.0, 1.0, 0.5])
    assert plain.class_weight is None and plain.label_smoothing == 0.0
    assert both.label_smoothing == 0.1 and both.class_weight.dtype == torch.float32 and both.class_weight.tolist() == [2.0, 1.0, 0.5]
    assert list(plain.state_dict()) == list(both.state_dict())
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in both.named_buffers()]
    both.load_state_dict(plain.state_dict(), strict=True)


@pytest.mark.parametrize("kw", [dict(label_smoothing=1.0), dict(label_smoothing=-0.5), dict(class_weights=[1.0, 2.0]),
                                dict(class_weights=[1.0, -1.0, 1.0]), dict(class_weights=[0.0, 0.0, 0.0]),
                                dict(class_weights=[1.0, float("nan"), 1.0])])
def test_model_refuses_bad_options(kw):
    with pytest.raises(ValueError):
        _model(**kw)
