"""GPU: the class-weighted, label-smoothed cross entropy (d2r_ce_fwd_ex / d2r_ce_bwd_ex) against fp64 torch through the C ABI, its
plain path against d2r_ce_fwd / d2r_ce_bwd bit for bit, the two options inside the one-call head, d2r_confusion_add against numpy,
and the trainer with --label_smoothing / --class_weights: dev metrics from the on-device confusion matrix, dev loss, checkpoint.

Branch                                                          Test
--------------------------------------------------------------  ------------------------------------------------------------
ce_ex thread loop (B > 256), multi-block bwd, grid edges,       test_cross_entropy_ex[*]
  weights / smoothing / both / a zero weight; C = 1 with its
  only weight zero: 0 / 0 = NaN, as torch
plain path = the plain kernels                                  test_cross_entropy_ex_plain_path_is_bit_identical[*]
label_smoothing outside [0, 1): nothing launched                test_cross_entropy_ex_refuses_bad_smoothing
head descriptor fields, d_logits still adds                     test_head_one_call_with_loss_options
confusion: ld > C, ties, labels -1 and C, repeated calls        test_confusion_add[*], test_confusion_add_functional
trainer: eval loop, per-class lines, loss, checkpoint, CLI      test_trainer_*"""
import logging
import os

import numpy as np
import pytest
import torch

from test_gpu_kernel_edges import Guarded, _st, call, check

pytestmark = pytest.mark.gpu

BS, CS = (1, 2, 255, 256, 257, 600), (1, 2, 3, 7)  # block-stride and grid-edge sizes of the two kernels
SHAPES = [(B, C) for B in BS for C in CS]
OPTIONS = ["plain", "w", "eps", "w+eps", "w0+eps"]  # (None, 0), (w, 0), (None, 0.1), (w, 0.1), (w with one zero entry, 0.3)
DLOSS = -1.7


def _case(B, C, option):
    """logits (+-80, as test_cross_entropy), labels, weights (or None), eps.  In the zero-weight case the seed is advanced until
    one label carries a non-zero weight (B = 1: the label is set by hand); with C = 1 the only weight is the zero one."""
    eps = {"plain": 0.0, "w": 0.0, "eps": 0.1, "w+eps": 0.1, "w0+eps": 0.3}[option]
    seed = B * 1000 + C
    while True:
        g = torch.Generator().manual_seed(seed)
        logits = 80.0 * (2.0 * torch.rand(B, C, generator=g) - 1.0)
        labels = torch.randint(0, C, (B,), generator=g)
        w = None
        if option in ("w", "w+eps", "w0+eps"):
            w = 0.25 + 2.0 * torch.rand(C, generator=g)
        if option != "w0+eps":
            return logits, labels, w, eps
        zero = (B + C) % C
        w[zero] = 0.0
        if B == 1 and C > 1:
            labels[0] = (zero + 1) % C
        if C == 1 or bool((w[labels] > 0).any()):
            return logits, labels, w, eps
        seed += 7919


def _run_ex(gpu, logits, labels, w, eps):
    B, C = logits.shape
    lg, lb = logits.to(gpu), labels.to(gpu)
    wd = None if w is None else w.to(gpu)
    wp = None if wd is None else wd.data_ptr()
    loss, dl = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
    dloss = torch.tensor([DLOSS], device=gpu)
    call("d2r_ce_fwd_ex", lg.data_ptr(), lb.data_ptr(), wp, eps, B, C, loss.ptr, _st())
    call("d2r_ce_bwd_ex", lg.data_ptr(), lb.data_ptr(), wp, eps, B, C, dloss.data_ptr(), dl.ptr, _st())
    torch.cuda.synchronize()
    return loss, dl


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("B,C", SHAPES, ids=[f"B{b}-C{c}" for b, c in SHAPES])
def test_cross_entropy_ex(gpu, B, C, option):
    logits, labels, w, eps = _case(B, C, option)
    tag = f"ce_ex[B={B} C={C} {option}]"
    loss, dl = _run_ex(gpu, logits, labels, w, eps)
    loss.intact(tag + ".loss")
    dl.intact(tag + ".dlogits")
    loss2, dl2 = _run_ex(gpu, logits, labels, w, eps)
    assert torch.equal(loss.buf.view(torch.int32), loss2.buf.view(torch.int32)), tag + ": the loss differs between two runs"
    assert torch.equal(dl.buf.view(torch.int32), dl2.buf.view(torch.int32)), tag + ": dlogits differ between two runs"
    lr = logits.double().requires_grad_(True)
    w64 = None if w is None else w.double()
    ref = torch.nn.functional.cross_entropy(lr, labels, weight=w64, label_smoothing=eps)
    wsum = float(B) if w is None else float(w64[labels].sum())
    if wsum == 0.0:  # C = 1 and its weight zero: every label carries weight 0 -> 0 / 0, NaN here as in torch
        assert C == 1 and bool(torch.isnan(ref)) and bool(torch.isnan(loss.t[0])), (tag, float(ref), float(loss.t[0]))
        return
    (DLOSS * ref).backward()
    print(f"{tag}: loss {float(loss.t[0]):.6f} ref {float(ref):.6f} err {abs(float(loss.t[0]) - float(ref)):.2e}; dlogits max err "
          f"{float((dl.t.double().cpu() - lr.grad).abs().max()):.2e}")
    wmax = 1.0 if w is None else float(w64.max())
    check(tag + ".loss", loss.t[0], ref.detach(), torch.float32, scale=max(float(ref.abs()), 1.0))
    check(tag + ".dlogits", dl.t, lr.grad, torch.float32, scale=1.7 * wmax / wsum)


@pytest.mark.parametrize("B,C", SHAPES, ids=[f"B{b}-C{c}" for b, c in SHAPES])
def test_cross_entropy_ex_plain_path_is_bit_identical(gpu, B, C):
    logits, labels, _, _ = _case(B, C, "plain")
    lg, lb = logits.to(gpu), labels.to(gpu)
    dloss = torch.tensor([DLOSS], device=gpu)
    loss0, dl0 = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
    call("d2r_ce_fwd", lg.data_ptr(), lb.data_ptr(), B, C, loss0.ptr, _st())
    call("d2r_ce_bwd", lg.data_ptr(), lb.data_ptr(), B, C, dloss.data_ptr(), dl0.ptr, _st())
    loss1, dl1 = _run_ex(gpu, logits, labels, None, 0.0)
    assert torch.equal(loss0.buf.view(torch.int32), loss1.buf.view(torch.int32)), (float(loss0.t[0]), float(loss1.t[0]))
    assert torch.equal(dl0.buf.view(torch.int32), dl1.buf.view(torch.int32))
    assert bool(torch.isfinite(loss1.t).all()) and bool(torch.isfinite(dl1.t).all())


def test_cross_entropy_ex_refuses_bad_smoothing(gpu):
    from d2r_amd import _lib
    lib = _lib.load()
    B, C = 5, 3
    logits, labels, w, _ = _case(B, C, "w")
    lg, lb, wd = logits.to(gpu), labels.to(gpu), w.to(gpu)
    dloss = torch.tensor([DLOSS], device=gpu)
    for eps in (-0.1, 1.0):
        for wp in (None, wd.data_ptr()):
            loss, dl = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
            assert lib.d2r_ce_fwd_ex(lg.data_ptr(), lb.data_ptr(), wp, eps, B, C, loss.ptr, _st()) != 0
            assert "label_smoothing" in lib.d2r_last_error().decode()
            assert lib.d2r_ce_bwd_ex(lg.data_ptr(), lb.data_ptr(), wp, eps, B, C, dloss.data_ptr(), dl.ptr, _st()) != 0
            torch.cuda.synchronize()
            for g in (loss, dl):  # nothing written: guards AND the poison fill of the output itself
                assert bool((g.buf.view(g.it) == g.sent).all()), f"eps {eps}: a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------
# the one-call head
# ------------------------------------------------------------------------------------------------------
def test_head_one_call_with_loss_options(gpu):
    """Both options on, B = 3, C = 3: the one-call head (d2r_head_desc.class_weight / label_smoothing) against the op-by-op path
    (F.cross_entropy with the options) - the same launches, so loss, logits and every parameter gradient are bit-identical, the
    bound of test_head_one_call_matches_op_by_op; the loss against fp64 torch on the returned logits plus js; and a second loss on
    the logits (d_logits) still adds, within the bound of test_head_one_call_backpropagates_a_second_loss_on_the_logits."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.params import ParamStore
    from oracle import d2r_oracle as O
    cfg = O.OracleConfig(text_layers=1, vision_layers=1, image_size=64, patch_size=32)
    sd = O.seeded_state_dict(cfg, seed=3, router_bias="normal")
    batch = tuple(t.to(gpu) for t in O.synthetic_batch(cfg, 3, 12, seed=4))
    labels = batch[3].cpu()
    weights, eps = [0.5, 2.0, 1.25], 0.1
    extra = torch.randn(3, 3, generator=torch.Generator().manual_seed(1)).to(gpu)
    res = {}
    for second in (False, True):
        for composite in (False, True):
            M.COMPOSITE_HEAD = composite
            try:
                model = M.UnimoModelF(default_args(label_smoothing=eps, class_weights=weights),
                                      VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                                      TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
                model.load_state_dict(sd, strict=True)
                model.to(gpu).set_compute_dtype(torch.float32).train()
                model.model.use_streams = False
                store = ParamStore(model, torch.float32)
                loss, logits = model(*batch)
                assert ("_HeadBackward" in repr(loss.grad_fn)) == composite, loss.grad_fn
                ((loss + 3.0 * (logits * extra).sum()) if second else loss * 64.0).backward()
                torch.cuda.synchronize()
                res[second, composite] = (loss.detach().clone(), logits.detach().clone(), store.flat_g.clone(),
                                          [(n, o, k) for n, _, o, k, _ in store.entries], model.last_aux["js_loss"].detach().clone())
            finally:
                M.COMPOSITE_HEAD = True
    (l0, g0, f0, ent, _), (l1, g1, f1, _, js) = res[False, False], res[False, True]
    assert torch.equal(l0, l1) and torch.equal(g0, g1), (float(l0), float(l1))
    bad = [n for n, o, k in ent if not torch.equal(f0[o:o + k], f1[o:o + k])]
    assert not bad, f"{len(bad)} parameter gradients differ, first {bad[:5]}"
    assert float(f1.abs().max()) > 0.0
    ref = torch.nn.functional.cross_entropy(g1.double().cpu(), labels, weight=torch.tensor(weights, dtype=torch.float64),
                                            label_smoothing=eps) + js.double().cpu()
    plain = torch.nn.functional.cross_entropy(g1.double().cpu(), labels) + js.double().cpu()
    print(f"head loss {float(l1):.7f} fp64 {float(ref):.7f} (without the options {float(plain):.7f})")
    check("head.loss", l1, ref, torch.float32, scale=max(float(ref.abs()), 1.0))
    assert abs(float(plain) - float(ref)) > 1e-3, "the options do not change this loss: vacuous"
    (_, _, s0, _, _), (_, _, s1, _, _) = res[True, False], res[True, True]
    for n, o, k in ent:
        a, b = s1[o:o + k], s0[o:o + k]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-9, n


# ------------------------------------------------------------------------------------------------------
# d2r_confusion_add
# ------------------------------------------------------------------------------------------------------
def _confusion_batch(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randint(-2, 3, (rows, C), generator=g).float()  # small integers: exact ties in most rows
    labels = torch.randint(-1, C + 1, (rows,), generator=g)        # -1 (unlabelled) and C (out of range) are skipped
    if rows >= 4:
        labels[0], labels[1], logits[2], logits[3] = -1, C, 1.0, float("-inf")  # both skips and two all-equal rows are present
    return logits, labels


def _confusion_ref(logits, labels, C):
    cm = np.zeros((C, C), dtype=np.int64)
    pred = np.argmax(logits.numpy(), axis=1)  # the first maximal index
    keep = (labels.numpy() >= 0) & (labels.numpy() < C)
    np.add.at(cm, (labels.numpy()[keep], pred[keep]), 1)
    return cm


CM_CASES = [(rows, C, pad) for rows in (1, 255, 256, 257, 5000) for C in (2, 3, 7) for pad in (0, 5)]


@pytest.mark.parametrize("rows,C,pad", CM_CASES, ids=[f"rows{r}-C{c}-ld{c + p}" for r, c, p in CM_CASES])
def test_confusion_add(gpu, rows, C, pad):
    ld = C + pad
    start = torch.randint(0, 5, (C, C), generator=torch.Generator().manual_seed(rows + C))
    counts = Guarded(gpu, torch.int64, C, C, fill=start.to(gpu))
    want = start.numpy().copy()
    for seed in (rows * 10 + C, rows * 10 + C + 1):  # two calls on the same counts: the sum
        logits, labels = _confusion_batch(rows, C, seed)
        buf = torch.full((rows, ld), float("inf"), device=gpu)  # a kernel that reads the ld gap predicts a class >= C
        buf[:, :C] = logits.to(gpu)
        call("d2r_confusion_add", buf.data_ptr(), ld, labels.to(gpu).data_ptr(), rows, C, counts.ptr, _st())
        want += _confusion_ref(logits, labels, C)
        torch.cuda.synchronize()
        counts.intact(f"confusion[rows={rows} C={C} ld={ld}]")
        assert np.array_equal(counts.t.cpu().numpy(), want), (counts.t.cpu().tolist(), want.tolist())
    assert int(want.sum() - start.sum()) < 2 * rows or rows == 1  # some rows were skipped (or none drawn at rows = 1)


def test_confusion_add_functional(gpu):
    from d2r_amd import _lib
    from d2r_amd import functional as F
    logits, labels = _confusion_batch(37, 3, 5)
    logits[4, 1] = float("nan")  # torch's rule: a NaN is the maximum
    counts = torch.zeros(3, 3, dtype=torch.int64, device=gpu)
    out = F.confusion_add(logits.to(gpu), labels.to(gpu), counts)
    assert out is counts
    cm = np.zeros((3, 3), dtype=np.int64)
    pred = torch.argmax(logits, dim=-1)
    for y, p in zip(labels.tolist(), pred.tolist()):
        if 0 <= y < 3:
            cm[y, p] += 1
    assert np.array_equal(counts.cpu().numpy(), cm)
    wide = torch.zeros(37, 8, device=gpu)
    wide[:, :3] = logits.to(gpu)
    F.confusion_add(wide[:, :3], labels.to(gpu), counts)  # a view with row stride 8
    assert np.array_equal(counts.cpu().numpy(), 2 * cm)
    for bad in (lambda: F.confusion_add(logits.to(gpu).t(), labels.to(gpu), counts),
                lambda: F.confusion_add(logits.to(gpu), labels.to(gpu)[:5], counts),
                lambda: F.confusion_add(logits.to(gpu), labels.to(gpu), counts.int()),
                lambda: F.confusion_add(logits.to(gpu), labels.to(gpu), torch.zeros(4, 4, dtype=torch.int64, device=gpu))):
        with pytest.raises(_lib.D2RError):
            bad()
    lib = _lib.load()
    x, y = logits.to(gpu), labels.to(gpu)
    for ld, rows, C in ((3, 0, 3), (3, 37, 0), (2, 37, 3)):
        assert lib.d2r_confusion_add(x.data_ptr(), ld, y.data_ptr(), rows, C, counts.data_ptr(), _st()) != 0
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), 2 * cm)


# ------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------
EPS, N_DEV = 0.1, 10


@pytest.fixture(scope="module")
def trained(gpu, tmp_path_factory):
    """One epoch of the tiny model of the trainer tests on synthetic data with --label_smoothing 0.1 --class_weights balanced."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.run import balanced_class_weights
    from d2r_amd.train import MSDTrainer
    torch.manual_seed(0)
    out = str(tmp_path_factory.mktemp("loss_metrics")) + "/"
    mk = lambda n, seed, sh: make_loader(SyntheticMSDDataset(n, 16, 64, 3, seed=seed, num_image_tokens=5), 4, sh, 0, drop_last=sh)
    train_dl, dev_dl = mk(32, 1, True), mk(N_DEV, 2, False)
    weights = balanced_class_weights(np.bincount(train_dl.dataset.labels, minlength=3).tolist())
    args = default_args(DR_step=3, compute_dtype=torch.bfloat16, device="cuda:0", num_epochs=1, batch_size=4, warmup_ratio=0.0,
                        save_path=out, lr=1e-4, label_smoothing=EPS, class_weights=weights)
    model = M.UnimoModelF(args, VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                          TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    lines = []
    logger = logging.getLogger("loss-metrics-test")

    class Catch(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())

    logger.addHandler(Catch())
    logger.setLevel(logging.INFO)
    tr = MSDTrainer(train_data=train_dl, dev_data=dev_dl, test_data=mk(8, 3, False), model=model, args=args, logger=logger, writer=None)
    tr.train(None, None)
    return tr, dev_dl, weights, lines, out


def test_trainer_dev_metrics_come_from_the_confusion_matrix(trained):
    from d2r_amd.train import get_four_metrics
    tr, dev_dl, weights, lines, _ = trained
    assert len(weights) == 3 and max(weights) > min(weights) > 0
    assert tr.last_dev_result is not None and tr.last_test_result is not None  # from the passes inside train()
    ret = tr.evaluate(1)
    res = tr.last_dev_result  # the result as logged: evaluate() itself returns the reference's scalar entries of it
    assert set(ret) == set(res) - {"confusion", "per_class"} and all(ret[k] == res[k] for k in ret)
    pred = tr.predict(dev_dl)
    acc, recall, precision, f1 = get_four_metrics(pred["labels"], pred["preds"].tolist(), type="weighted")
    assert (res["eval_accuracy"], res["recall"], res["precision"], res["f_score"]) == (acc, recall, precision, f1)
    assert sum(map(sum, res["confusion"])) == N_DEV and len(res["confusion"]) == 3
    assert [pc["support"] for pc in res["per_class"]] == np.bincount(pred["labels"], minlength=3).tolist()
    for k in ("eval_accuracy", "precision", "recall", "f_score", "confusion", "per_class"):
        assert pred["metrics"][k] == res[k], k
    # the log of the evaluate() inside train(): the aggregate lines, then one line per class
    at = lines.index("***** Dev Eval results *****")
    block = lines[at + 1:at + 11]
    assert [l.split(" = ")[0] for l in block[:6]] == ["  eval_accuracy", "  f_score", "  global_step", "  loss", "  precision", "  recall"]
    assert block[6].startswith("  confusion matrix (row: label, column: prediction): [[")
    assert [l.split(":")[0] for l in block[7:]] == ["  class 0", "  class 1", "  class 2"] and "support" in block[9]


def test_trainer_dev_loss_is_the_weighted_smoothed_loss(trained):
    """evaluate()'s loss (the sum over the dev batches of ce + js, with both options in eval mode too) against fp64 torch on
    predict()'s logits, batch by batch, plus each batch's js term."""
    tr, dev_dl, weights, _, _ = trained
    res = tr.evaluate(1)
    pred = tr.predict(dev_dl)
    tr.model.eval()
    js = []
    with torch.no_grad():
        for batch in dev_dl:
            tr._step(tr._to_device(batch), mode="dev")
            js.append(float(tr.model.last_aux["js_loss"]))
    tr.model.train()
    labels, w64 = torch.tensor(pred["labels"]), torch.tensor(weights, dtype=torch.float64)
    ref, plain = 0.0, 0.0
    for i, lo in enumerate(range(0, N_DEV, 4)):
        lg, y = pred["logits"][lo:lo + 4].double(), labels[lo:lo + 4]
        ref += float(torch.nn.functional.cross_entropy(lg, y, weight=w64, label_smoothing=EPS)) + js[i]
        plain += float(torch.nn.functional.cross_entropy(lg, y)) + js[i]
    print(f"dev loss {res['loss']:.7f} fp64 {ref:.7f} (without the options {plain:.7f})")
    check("dev loss", torch.tensor(res["loss"]), torch.tensor(ref, dtype=torch.float64), torch.float32, scale=max(abs(ref), 1.0))
    assert abs(plain - ref) > 1e-3, "the options do not change this loss: vacuous"


def test_trainer_checkpoint_keeps_the_reference_keys_and_loads_with_only_test(trained, tmp_path):
    import json
    from d2r_amd import run
    from oracle import d2r_oracle as O
    tr, _, _, _, out = trained
    ck = os.path.join(out, "best_model.pth")
    assert os.path.exists(ck)
    saved = torch.load(ck, map_location="cpu")
    cfg = O.OracleConfig(text_layers=1, vision_layers=1, image_size=64, patch_size=32)
    assert set(saved) == set(O.param_spec(cfg)), "checkpoint keys differ from the reference's state-dict names"
    path = str(tmp_path / "pred.jsonl")
    run.main(["--only_test", "--load_path", ck, "--write_path", path, "--label_smoothing", "0.1", "--class_weights", "balanced",
              "--train_samples", "32", "--eval_samples", "8", "--batch_size", "4", "--encoder_layers", "1", "--image_size", "64",
              "--max_seq", "16", "--num_workers", "0", "--save_path", str(tmp_path) + "/", "--dtype", "bf16"])
    with open(path) as f:
        recs = [json.loads(line) for line in f]
    assert len(recs) == 8 and all(r["label"] is not None and 0 <= r["pred"] < 3 for r in recs)
