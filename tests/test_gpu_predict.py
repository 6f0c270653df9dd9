"""GPU: prediction from a checkpoint - d2r_argmax_rows against torch.argmax, the label-free d2r_head_fwd, the label-free
UnimoModelF forward (logits bit-identical to the labelled call's), the per-sample router outputs aux["paths_text" / "paths_image"]
against the live fp64 oracle, MSDTrainer.predict, and --only_test / --write_path end to end."""
import json
import logging
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import golden_batch, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "fp16"]
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------
# d2r_argmax_rows
# ------------------------------------------------------------------------------------------------------
CRAFTED = [  # (row, torch.argmax's answer)
    ([1.0, 3.0, 3.0, 2.0, 0.0], 1),          # tie: lowest index
    ([2.0, 2.0, 2.0, 2.0, 2.0], 0),          # all equal
    ([-INF, -INF, -INF, -INF, -INF], 0),
    ([-INF, 2.0, INF, INF, 1.0], 2),
    ([INF, INF, INF, INF, INF], 0),
    ([NAN, 1.0, 2.0, INF, NAN], 0),          # a NaN is the maximum, the first one wins
    ([1.0, NAN, 5.0, NAN, INF], 1),
    ([-INF, -INF, 3.0, -INF, NAN], 4),
    ([-0.0, 0.0, -1.0, -0.0, -2.0], 0),      # -0 == +0
    ([-5.0, -3.0, -4.0, -3.0, -9.0], 1),
    ([NAN, NAN, NAN, NAN, NAN], 0),
    ([1e-45, 0.0, -1e-45, 1e-45, 0.0], 0),   # subnormals
]


def test_argmax_rows_crafted(gpu):
    from d2r_amd import functional as F
    x = torch.tensor([r for r, _ in CRAFTED], dtype=torch.float32, device=gpu)
    got = F.argmax_rows(x)
    assert got.dtype == torch.int64 and got.shape == (len(CRAFTED),)
    assert got.cpu().tolist() == [i for _, i in CRAFTED]
    assert torch.equal(got, torch.argmax(x, dim=-1))


def _random_rows(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (rows, cols), generator=g).float()  # small integers: many ties
    x += torch.randn(rows, cols, generator=g) * (torch.rand(rows, 1, generator=g) < 0.5)
    special = torch.rand(rows, cols, generator=g)
    x[special < 0.02] = NAN
    x[(special >= 0.02) & (special < 0.05)] = INF
    x[(special >= 0.05) & (special < 0.09)] = -INF
    return x


@pytest.mark.parametrize("cols", [1, 2, 3, 7, 33])
@pytest.mark.parametrize("rows", [0, 1, 5, 100_000])
def test_argmax_rows_matches_torch(gpu, rows, cols):
    from d2r_amd import functional as F
    x = _random_rows(rows, cols, seed=rows * 131 + cols).to(gpu)
    got = F.argmax_rows(x)
    assert got.shape == (rows,)
    if rows:
        assert torch.equal(got, torch.argmax(x, dim=-1))
    # a row stride larger than cols: a column slice of a wider matrix
    wide = _random_rows(rows, cols + 5, seed=rows * 17 + cols).to(gpu)
    view = wide[:, 2:2 + cols]
    assert view.stride(0) == cols + 5 or rows == 0
    got = F.argmax_rows(view)
    torch.cuda.synchronize()
    assert got.shape == (rows,)
    if rows:
        assert torch.equal(got, torch.argmax(view, dim=-1))


def test_argmax_rows_refuses_bad_arguments(gpu):
    from d2r_amd import _lib
    x = torch.zeros(4, 3, device=gpu)
    idx = torch.empty(4, dtype=torch.int64, device=gpu)
    lib = _lib.load()
    for args, what in [((x.data_ptr(), 3, 4, 0, idx.data_ptr(), None), "bad shape"),     # cols 0
                       ((x.data_ptr(), 2, 4, 3, idx.data_ptr(), None), "bad shape"),     # ld < cols
                       ((x.data_ptr(), 3, -1, 3, idx.data_ptr(), None), "bad shape"),    # rows < 0
                       ((None, 3, 4, 3, idx.data_ptr(), None), "null pointer"),
                       ((x.data_ptr(), 3, 4, 3, None, None), "null pointer")]:
        assert lib.d2r_argmax_rows(*args) != 0
        assert what in lib.d2r_last_error().decode()
    assert lib.d2r_argmax_rows(None, 3, 0, 3, None, None) == 0  # rows == 0: nothing to do, nothing launched


def test_argmax_rows_refuses_overlapping_views(gpu):
    from d2r_amd import _lib
    from d2r_amd import functional as F
    row = torch.randn(1, 3, device=gpu)
    with pytest.raises(_lib.D2RError, match="not overlap"):
        F.argmax_rows(row.expand(4, 3))  # stride(0) == 0: row r would be read at r * 3, past the storage
    with pytest.raises(_lib.D2RError, match="unit-stride"):
        F.argmax_rows(torch.randn(3, 4, device=gpu).t())  # column stride 4
    assert F.argmax_rows(row.expand(1, 3)).tolist() == [int(torch.argmax(row))]  # one row: its stride is never used
    col = torch.randn(4, 6, device=gpu)[:, 2:3]  # one column, row stride 6
    assert F.argmax_rows(col).tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------
# the label-free head
# ------------------------------------------------------------------------------------------------------
def _tiny_model(gpu, dtype, dr=3, num_cells=6, layers=1, image=64, seed=3, router_bias="normal"):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.params import ParamStore
    from oracle import d2r_oracle as O
    cfg = O.OracleConfig(text_layers=layers, vision_layers=layers, image_size=image, patch_size=32, DR_step=dr, num_cells=num_cells)
    sd = O.seeded_state_dict(cfg, seed=seed, router_bias=router_bias)
    tc = TextConfig(num_hidden_layers=layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=layers, image_size=image, patch_size=32)
    model = M.UnimoModelF(default_args(DR_step=dr, num_cells=num_cells), vc, tc)
    model.load_state_dict(sd, strict=True)
    model.to(gpu).set_compute_dtype(dtype).eval()
    store = ParamStore(model, dtype)
    return model, store, sd, cfg


def test_head_fwd_without_labels(gpu):
    from d2r_amd import _lib
    from d2r_amd import functional as F
    from oracle import d2r_oracle as O
    model, _, _, cfg = _tiny_model(gpu, torch.float32)
    batch = [t.to(gpu) for t in O.synthetic_batch(cfg, 5, 12, seed=4)]
    hb = model.model._head_bundle(model.fc)
    assert hb is not None, "the one-call head does not apply"
    with torch.no_grad():
        model(*batch)
        aux = model.last_aux
        tp, vp, js = aux["text_pooled"], aux["vision_pooled"], aux["js_loss"]
        loss, logits, pooled = F.head(tp, vp, js, batch[3], hb)
        none, logits2, pooled2 = F.head(tp, vp, js, None, hb)  # d2r_head_fwd with labels, loss and js NULL
    torch.cuda.synchronize()
    assert none is None and loss is not None
    assert torch.equal(logits, logits2) and torch.equal(pooled, pooled2)
    with pytest.raises(_lib.D2RError, match="no loss"):
        F.head(tp.detach().requires_grad_(True), vp, js, None, hb)
    # d2r_head_bwd without labels is refused on the host (nothing launched)
    d = _lib.HeadDesc()
    d.B, d.E, d.mm, d.chunks, d.rank, d.classes = 5, hb.E, hb.mm, hb.chunks, hb.rank, hb.classes
    d.lin0, d.lin1, d.merge0, d.merge1, d.lin_out, d.fc = hb.lp
    d.x0, d.x1, d.logits, d.pooled = tp.data_ptr(), vp.data_ptr(), logits.data_ptr(), pooled.data_ptr()
    lib = _lib.load()
    assert lib.d2r_head_bwd(d, None) != 0
    assert "labels are required" in lib.d2r_last_error().decode()


def _golden_model(gpu, case_name, dtype):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.params import ParamStore
    from oracle import d2r_oracle as O
    from oracle import golden_cases as GC
    case = [c for c in GC.MODEL_CASES if c.name == case_name][0]
    g = load_golden(case.name)
    tc = TextConfig(num_hidden_layers=case.layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=case.layers, image_size=case.image_size, patch_size=case.patch)
    model = M.UnimoModelF(default_args(DR_step=case.DR_step), vc, tc)
    model.load_state_dict(O.seeded_state_dict(case.cfg(), seed=case.seed, router_bias=case.router_bias), strict=True)
    model.to(gpu).set_compute_dtype(dtype).eval()
    ParamStore(model, dtype)
    return model, [t.to(gpu) for t in golden_batch(case, g)]


@pytest.mark.parametrize("composite", [True, False], ids=["one_call_head", "op_by_op_head"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case_name", ["m_l2_eval", "m_l2_dr4"])
def test_label_free_forward_is_bit_identical(gpu, case_name, dtype, composite):
    from d2r_amd import modules as M
    M.COMPOSITE_HEAD = composite
    try:
        model, (ids, mask, tt, labels, images) = _golden_model(gpu, case_name, dtype)
        assert (model.model._head_bundle(model.fc) is not None) == composite
        with torch.no_grad():
            loss, logits = model(ids, mask, tt, labels, images)
            aux1 = model.last_aux
            none, logits2 = model(ids, mask, tt, None, images)
            aux2 = model.last_aux
        torch.cuda.synchronize()
        assert loss is not None and none is None
        assert logits2.dtype == torch.float32 and torch.equal(logits, logits2), float((logits - logits2).abs().max())
        assert torch.equal(aux1["paths_text"], aux2["paths_text"]) and torch.equal(aux1["paths_image"], aux2["paths_image"])
        with pytest.raises(RuntimeError, match="no loss"):
            model(ids, mask, tt, None, images)  # under grad: nothing to differentiate
    finally:
        M.COMPOSITE_HEAD = True


# ------------------------------------------------------------------------------------------------------
# aux["paths_text"] / aux["paths_image"] against the fp64 oracle
# ------------------------------------------------------------------------------------------------------
PATH_BOUND = {torch.float32: 1e-5, torch.float16: 8e-3, torch.bfloat16: 6e-2}  # fp16 / bf16: test_full_model_vs_reference_golden's sim_paths


def _oracle_paths(trace, prefix, dr, B):
    keys = [f"{prefix}.dynamic_itr_l0.probs"] + [f"{prefix}.dynamic_itr_l1.{i}.probs" for i in range(dr - 2)] + [f"{prefix}.dynamic_itr_l2.probs"]
    return torch.cat([trace[k].reshape(B, -1) for k in keys], dim=-1)


PATH_CONFIGS = [(2, 6), (3, 6), (8, 6), (3, 4)]  # (DR_step, num_cells)
PATH_MODES = [(torch.float32, False), (torch.bfloat16, True), (torch.bfloat16, False), (torch.float16, True), (torch.float16, False)]


@pytest.mark.parametrize("mode", PATH_MODES, ids=["f32", "bf16_whole", "bf16_op_by_op", "fp16_whole", "fp16_op_by_op"])
@pytest.mark.parametrize("dr,nc", PATH_CONFIGS, ids=["dr2", "dr3", "dr8", "dr3_cells4"])
def test_paths_vs_fp64_oracle(gpu, monkeypatch, dr, nc, mode):
    from d2r_amd import functional as F
    from d2r_amd import modules as M
    from oracle import d2r_oracle as O
    dtype, whole = mode
    monkeypatch.setattr(M, "COMPOSITE_ROUTING", whole)
    calls = []
    real = F.interaction
    monkeypatch.setattr(F, "interaction", lambda *a, **k: calls.append(1) or real(*a, **k))
    model, _, sd, cfg = _tiny_model(gpu, dtype, dr=dr, num_cells=nc, seed=7 + dr)
    B = 4
    ids, mask, tt, labels, images = O.synthetic_batch(cfg, B, 12, seed=dr)
    with torch.no_grad():
        _, _ = model(ids.to(gpu), mask.to(gpu), tt.to(gpu), None, images.to(gpu))
    torch.cuda.synchronize()
    assert len(calls) == (2 if whole else 0), "the module path under test was not the one taken"
    aux = model.last_aux
    trace = {}
    osd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        O.forward(osd, cfg, ids, mask, tt, labels, images.double(), train=False, trace=trace)
    total = nc * nc * (dr - 1) + nc
    for key, prefix in (("paths_text", "model.itr_module"), ("paths_image", "model.Reversed_itr_module")):
        got = aux[key]
        assert got.dtype == torch.float32 and got.shape == (B, total), (key, got.shape)
        ref = _oracle_paths(trace, prefix, dr, B)
        assert ref.shape == (B, total)
        got = got.double().cpu()
        err = float((got - ref).abs().max())
        assert err <= PATH_BOUND[dtype], f"{key}: err {err:.3e}"
        assert torch.equal(got == 0, ref == 0), f"{key}: open / closed paths differ from the oracle"
        # the [B,B] Gram matrix the JS term reads
        sim = aux["sim_paths" if key == "paths_text" else "rev_sim_paths"].double().cpu()
        gram = got @ got.t()
        assert float((gram - sim).abs().max()) <= 1e-5 * max(float(gram.abs().max()), 1.0)
    print(f"[dr{dr} cells{nc} {str(dtype)[6:]} {'whole' if whole else 'op-by-op'}] open paths text "
          f"{int((aux['paths_text'] != 0).sum())}/{aux['paths_text'].numel()}")


# ------------------------------------------------------------------------------------------------------
# MSDTrainer.predict
# ------------------------------------------------------------------------------------------------------
def test_trainer_predict_synthetic(gpu, tmp_path):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.train import MSDTrainer, get_four_metrics
    torch.manual_seed(0)
    tc = TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)
    args = default_args(compute_dtype=torch.bfloat16, device="cuda:0", num_epochs=1, batch_size=4, save_path=None)
    model = M.UnimoModelF(args, vc, tc)
    data = make_loader(SyntheticMSDDataset(10, 16, 64, 3, seed=3, num_image_tokens=5), 4, False, 0)
    logger = logging.getLogger("predict-test")
    tr = MSDTrainer(test_data=data, model=model, args=args, logger=logger, writer=None)
    out_path = str(tmp_path / "sub" / "pred.jsonl")
    res = tr.predict(data, write_path=out_path)
    assert model.training  # back in training mode, like test()
    logits, probs, preds = res["logits"], res["probs"], res["preds"]
    assert logits.shape == (10, 3) and probs.shape == (10, 3) and preds.dtype == torch.int64 and preds.shape == (10,)
    assert not logits.is_cuda and not probs.is_cuda
    assert torch.equal(preds, torch.argmax(logits, dim=-1))
    ref = torch.softmax(logits.double(), dim=-1)
    assert float((probs.double() - ref).abs().max()) <= 1e-6
    # the label-free logits equal the labelled eval forward's, batch by batch
    model.eval()
    with torch.no_grad():
        lab = torch.cat([tr._step(tr._to_device(b), mode="test")[0][1].cpu() for b in data])
    assert torch.equal(lab, logits)
    labels = [int(y) for b in data for y in b[4]]
    assert res["labels"] == labels and res["ids"] == [None] * 10
    tres = tr.test(1)
    for k in ("eval_accuracy", "precision", "recall", "f_score"):
        assert res["metrics"][k] == tres[k], k
    acc = get_four_metrics(labels, preds.tolist())[0]
    assert res["metrics"]["eval_accuracy"] == acc
    assert res["samples_per_sec"] > 0
    with open(out_path) as f:
        recs = [json.loads(line) for line in f]
    assert [r["index"] for r in recs] == list(range(10))
    for i, r in enumerate(recs):
        assert r["id"] is None and r["label"] == labels[i] and r["pred"] == int(preds[i])
        assert torch.equal(torch.tensor(r["probs"], dtype=torch.float32), probs[i])
        assert torch.equal(torch.tensor(r["paths_text"], dtype=torch.float32), res["paths_text"][i])
        assert torch.equal(torch.tensor(r["paths_image"], dtype=torch.float32), res["paths_image"][i])
        assert len(r["paths_text"]) == 6 * 6 * 2 + 6


def test_predict_reports_corrupt_device_decodes(gpu, tmp_path):
    """--image_decode device: predict() counts the device decodes and reports one whose entropy data is corrupt, as train() does."""
    pytest.importorskip("transformers")
    from test_clip_data import make_msd_dir
    from test_gpu_clip_preprocess import _model
    from test_gpu_jpeg_decode import _corrupt
    from test_jpeg_host import encode
    from d2r_amd.config import default_args
    from d2r_amd.data import MSDDataset, make_loader
    from d2r_amd.image import ClipCollate
    from d2r_amd.train import MSDTrainer
    data, img, vocab = make_msd_dir(str(tmp_path), n=8)  # test.json: s4 .. s7
    with open(os.path.join(img, "s5.jpg"), "wb") as f:
        f.write(_corrupt(encode(50, 640, 480, quality=95)))
    dl = make_loader(MSDDataset(os.path.join(data, "test.json"), img, vocab, max_seq=32, image_decode="device"), 4, False, 0,
                     collate_fn=ClipCollate(224, 224))
    msgs = []

    class Catch(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.getMessage())

    logger = logging.getLogger("predict-decode-test")
    logger.addHandler(Catch())
    logger.setLevel(logging.INFO)
    tr = MSDTrainer(test_data=dl, model=_model(gpu), args=default_args(device=str(gpu), save_path=None), logger=logger, writer=None)
    res = tr.predict(dl)
    assert res["ids"] == ["s4", "s5", "s6", "s7"] and res["metrics"] is not None
    assert any(m.startswith("1 JPEG image(s) had corrupt entropy data") for m in msgs), msgs
    assert "prediction images: 4 decoded on the device, 0 on the host, 1 device decode(s) with corrupt data" in msgs, msgs


# ------------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------------
def _cli(args, cwd, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "d2r_amd.run", *args], cwd=str(cwd), env=env,
                       capture_output=True, text=True)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


def _results(log, header):
    """The `key = value` lines logged under the last `header` line."""
    lines = log.splitlines()
    start = max(i for i, line in enumerate(lines) if header in line)
    out = {}
    for line in lines[start + 1:]:
        msg = line.split(" -   ", 1)[-1]
        if not msg.startswith("  ") or " = " not in msg:
            break
        k, v = msg.strip().split(" = ", 1)
        out[k] = v
    return out


def _read(path):
    with open(path) as f:
        return [json.loads(line) for line in f]


TINY = ["--eval_samples", "8", "--batch_size", "4", "--encoder_layers", "1", "--image_size", "64", "--max_seq", "16",
        "--num_workers", "0", "--dtype", "bf16"]


def test_cli_only_test_reproduces_the_training_runs_predictions(gpu, tmp_path):
    save = str(tmp_path / "out") + "/"
    log = _cli(["--num_epochs", "1", "--train_samples", "16", "--save_path", save, "--write_path", str(tmp_path / "train_pred.jsonl"),
                *TINY], tmp_path)
    ck = os.path.join(save, "best_model.pth")
    assert os.path.exists(ck) and os.path.exists(tmp_path / "train_pred.jsonl")
    test_metrics = _results(log, "***** Test Eval results *****")
    log2 = _cli(["--only_test", "--load_path", ck, "--save_path", save, "--write_path", str(tmp_path / "only.jsonl"), *TINY], tmp_path)
    assert "Running training" not in log2 and not re.search(r"step \d+ loss:", log2) and "Running evaluate" not in log2
    assert re.search(r"step \d+ loss:", log)
    a, b = _read(tmp_path / "train_pred.jsonl"), _read(tmp_path / "only.jsonl")
    assert len(a) == len(b) == 8
    assert a == b
    pm = _results(log2, "***** Prediction results *****")
    for k in ("eval_accuracy", "precision", "recall", "f_score"):
        assert pm[k] == test_metrics[k], (k, pm[k], test_metrics[k])


def test_cli_only_test_on_unlabelled_posts(gpu, tmp_path):
    pytest.importorskip("transformers")
    from test_clip_data import make_msd_dir
    data, img, vocab = make_msd_dir(str(tmp_path / "ds"), n=8)
    with open(os.path.join(data, "test.json")) as f:
        test = json.load(f)
    for s in test:
        del s["emotion_label"]
    with open(os.path.join(data, "test.json"), "w") as f:
        json.dump(test, f)
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    torch.manual_seed(1)
    model = M.UnimoModelF(default_args(), VisionConfig(num_hidden_layers=1, image_size=224, patch_size=32),
                          TextConfig(num_hidden_layers=1))
    ck = str(tmp_path / "ck.pth")
    torch.save(model.state_dict(), ck)
    out = str(tmp_path / "pred.jsonl")
    log = _cli(["--only_test", "--load_path", ck, "--data_path", data, "--img_path", img, "--bert_name", vocab, "--encoder_layers", "1",
                "--batch_size", "4", "--num_workers", "0", "--max_seq", "32", "--save_path", str(tmp_path / "o") + "/",
                "--write_path", out], tmp_path)
    assert "no metrics computed" in log and "f_score" not in log
    recs = _read(out)
    assert [r["id"] for r in recs] == [str(s["id"]) for s in test]
    assert all(r["label"] is None and 0 <= r["pred"] < 3 and math.isclose(sum(r["probs"]), 1.0, rel_tol=1e-5) for r in recs)
