"""GPU: focal loss.  d2r_ce_focal_fwd / d2r_ce_focal_bwd through the C ABI against the fp64 model of test_focal_host.py and, at
gamma == 0, against d2r_ce_mix_* / d2r_ce_*_ex / d2r_ce_* bit for bit; the autograd function; the focal loss inside the one-call head;
the trainer and the command line with --focal_gamma.

Branch                                                          Test
--------------------------------------------------------------  ------------------------------------------------------------
thread loop (B > 256), multi-block bwd, C == 1, the four        test_cross_entropy_focal[*]
  options x gamma 0.5 / 2 / 5 x logit amplitude 80 / 4 x pair
  NULL / lam all 1 / random / y2 == y
u underflows (target ahead by > 104), su denormal, C == 1       test_focal_is_finite_where_nothing_is_left_off_the_target
gamma == 0: the launches of mix / _ex / plain                   test_gamma_zero_has_the_bits_of_the_kernels_it_forwards_to[*]
not vacuous; every refusal writes nothing; F.cross_entropy      test_focal_is_not_vacuous_refusals_and_autograd
head: d2r_head_focal_desc, one call = op by op                  test_head_one_call_with_focal[*]
trainer: off = no focal call and the old steps, on = the        test_trainer_*, test_cli_trains_with_the_flag_and_logs_it
  focal loss in the training and the dev pass"""
import logging

import pytest
import torch

from test_focal_host import focal_ce_model
from test_gpu_kernel_edges import Guarded, _st, call, check
from test_mix_host import mixed_ce_model

pytestmark = pytest.mark.gpu

BS, CS = (1, 2, 255, 256, 257, 600), (1, 2, 3, 7)
CE_SHAPES = [(B, C) for B in BS for C in CS]
CE_OPTIONS = ["plain", "w", "eps", "w+eps"]
GAMMAS = (0.5, 2.0, 5.0)
PAIRS = ["null", "ones", "random", "same"]
DLOSS = -1.7


def _ce_case(B, C, option, amp=80.0):
    """The generator of test_gpu_mix.py, with the logits' amplitude as a parameter."""
    eps = {"plain": 0.0, "w": 0.0, "eps": 0.1, "w+eps": 0.1}[option]
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = amp * (2.0 * torch.rand(B, C, generator=g) - 1.0)
    y, y2 = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    w = 0.25 + 2.0 * torch.rand(C, generator=g) if option in ("w", "w+eps") else None  # every weight positive: every W is
    return logits, y, y2, torch.rand(B, generator=g), w, eps


def _pair(pattern, y, y2, lam_r):
    B = y.shape[0]
    return {"null": (None, None), "ones": (y2, torch.ones(B)), "random": (y2, lam_r), "same": (y, lam_r)}[pattern]


def _run_ce(gpu, name, logits, y, y2, lam, w, eps, gamma=0.0):
    """name: "focal", "mix" (y2 / lam may be None: NULL), "ex" or "plain"; -> (loss, dlogits) in guarded buffers."""
    B, C = logits.shape
    lg, yd = logits.to(gpu), y.to(gpu)
    y2d, lamd, wd = (None if t is None else t.to(gpu) for t in (y2, lam, w))
    p = lambda t: None if t is None else t.data_ptr()
    loss, dl = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
    dloss = torch.tensor([DLOSS], device=gpu)
    if name == "focal":
        call("d2r_ce_focal_fwd", lg.data_ptr(), yd.data_ptr(), p(y2d), p(lamd), p(wd), eps, gamma, B, C, loss.ptr, _st())
        call("d2r_ce_focal_bwd", lg.data_ptr(), yd.data_ptr(), p(y2d), p(lamd), p(wd), eps, gamma, B, C, dloss.data_ptr(), dl.ptr, _st())
    elif name == "mix":
        call("d2r_ce_mix_fwd", lg.data_ptr(), yd.data_ptr(), p(y2d), p(lamd), p(wd), eps, B, C, loss.ptr, _st())
        call("d2r_ce_mix_bwd", lg.data_ptr(), yd.data_ptr(), p(y2d), p(lamd), p(wd), eps, B, C, dloss.data_ptr(), dl.ptr, _st())
    elif name == "ex":
        call("d2r_ce_fwd_ex", lg.data_ptr(), yd.data_ptr(), p(wd), eps, B, C, loss.ptr, _st())
        call("d2r_ce_bwd_ex", lg.data_ptr(), yd.data_ptr(), p(wd), eps, B, C, dloss.data_ptr(), dl.ptr, _st())
    else:
        call("d2r_ce_fwd", lg.data_ptr(), yd.data_ptr(), B, C, loss.ptr, _st())
        call("d2r_ce_bwd", lg.data_ptr(), yd.data_ptr(), B, C, dloss.data_ptr(), dl.ptr, _st())
    torch.cuda.synchronize()
    return loss, dl


def _same_bits(a, b):
    return torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))


def _untouched(g):
    return bool((g.buf.view(g.it) == g.sent).all())


# ------------------------------------------------------------------------------------------------------
# d2r_ce_focal_fwd / d2r_ce_focal_bwd
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [80.0, 4.0], ids=["amp80", "amp4"])
@pytest.mark.parametrize("option", CE_OPTIONS)
@pytest.mark.parametrize("B,C", CE_SHAPES, ids=[f"B{b}-C{c}" for b, c in CE_SHAPES])
def test_cross_entropy_focal(gpu, B, C, option, amp):
    logits, y, y2, lam_r, w, eps = _ce_case(B, C, option, amp)
    w64 = None if w is None else w.double()
    wmax = 1.0 if w is None else float(w64.max())
    for gamma in GAMMAS:
        for pattern in PAIRS:
            yb, lam = _pair(pattern, y, y2, lam_r)
            tag = f"ce_focal[B={B} C={C} {option} amp {amp:g} gamma {gamma:g} pair {pattern}]"
            loss, dl = _run_ce(gpu, "focal", logits, y, yb, lam, w, eps, gamma)
            loss.intact(tag + ".loss")
            dl.intact(tag + ".dlogits")
            loss2, dl2 = _run_ce(gpu, "focal", logits, y, yb, lam, w, eps, gamma)
            assert _same_bits(loss, loss2) and _same_bits(dl, dl2), tag + ": two runs differ"
            ref, dref, W = focal_ce_model(logits, y, yb, lam, w64, eps, gamma, dloss=DLOSS)
            scale = max(float(dref.abs().max()), 1.7 * wmax / W)
            print(f"{tag}: loss {float(loss.t[0]):.6f} ref {float(ref):.6f} err {abs(float(loss.t[0]) - float(ref)):.2e}; dlogits max err "
                  f"{float((dl.t.double().cpu() - dref).abs().max()):.2e} of scale {scale:.2e}")
            assert bool(torch.isfinite(loss.t).all()) and bool(torch.isfinite(dl.t).all()), tag + ": an output is not finite"
            check(tag + ".loss", loss.t[0], ref, torch.float32, scale=max(float(ref.abs()), 1.0))
            check(tag + ".dlogits", dl.t, dref, torch.float32, scale=scale)
            if C == 1:  # nothing off the target: loss 0, gradient 0
                assert float(loss.t[0]) == 0.0 and float(dl.t.abs().max()) == 0.0, tag


def test_focal_is_finite_where_nothing_is_left_off_the_target(gpu):
    """Rows whose target leads by more than fp32's exponent range (u underflows: u^g = 0, r = 0), by a little less (su is a denormal or
    close: 1 / su overflows, the quotient does not), the same with a pair on one class, and ordinary rows next to them."""
    leads = [200.0, 120.0, 104.5, 103.0, 100.0, 95.0, 88.0, 87.0, 80.0, 40.0, 0.0, -50.0]
    logits = torch.tensor([[lead, 0.0, -1.0] for lead in leads])
    B = len(leads)
    y = torch.zeros(B, dtype=torch.int64)
    w = torch.tensor([0.5, 2.0, 1.25])
    for yb, lam in ((None, None), (y, torch.full((B,), 0.3)), (torch.ones(B, dtype=torch.int64), torch.full((B,), 0.999))):
        for gamma in GAMMAS:
            tag = f"focal underflow[gamma {gamma:g} pair {None if yb is None else int(yb[0])}]"
            loss, dl = _run_ce(gpu, "focal", logits, y, yb, lam, w, 0.1, gamma)
            assert bool(torch.isfinite(loss.t).all()) and bool(torch.isfinite(dl.t).all()), tag
            ref, dref, W = focal_ce_model(logits, y, yb, lam, w.double(), 0.1, gamma, dloss=DLOSS)
            check(tag + ".loss", loss.t[0], ref, torch.float32, scale=max(float(ref.abs()), 1.0))
            check(tag + ".dlogits", dl.t, dref, torch.float32, scale=max(float(dref.abs().max()), 1.7 * 2.0 / W))
            if yb is None or int(yb[0]) == 0:
                assert float(dl.t[:2].abs().max()) == 0.0, tag + ": a row with u == 0 has a gradient"


@pytest.mark.parametrize("option", CE_OPTIONS)
def test_gamma_zero_has_the_bits_of_the_kernels_it_forwards_to(gpu, option):
    for B, C in CE_SHAPES:
        logits, y, y2, lam_r, w, eps = _ce_case(B, C, option)
        tag = f"focal gamma 0[B={B} C={C} {option}]"
        for pattern in ("random", "same", "ones"):
            yb, lam = _pair(pattern, y, y2, lam_r)
            got, want = _run_ce(gpu, "focal", logits, y, yb, lam, w, eps, 0.0), _run_ce(gpu, "mix", logits, y, yb, lam, w, eps)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), f"{tag} pair {pattern}: not the bits of d2r_ce_mix_*"
        got = _run_ce(gpu, "focal", logits, y, None, None, w, eps, 0.0)
        for name in ("mix", "ex") + (("plain",) if option == "plain" else ()):
            want = _run_ce(gpu, name, logits, y, None, None, w, eps)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), f"{tag} NULL pair: not the bits of {name}"


def test_focal_is_not_vacuous_refusals_and_autograd(gpu):
    from d2r_amd import _lib
    from d2r_amd import functional as F
    lib = _lib.load()
    B, C = 257, 7
    logits, y, y2, lam, w, eps = _ce_case(B, C, "w+eps", 4.0)
    focal, dfocal = _run_ce(gpu, "focal", logits, y, y2, lam, w, eps, 2.0)
    plain, _ = _run_ce(gpu, "mix", logits, y, y2, lam, w, eps)
    print(f"B = 257, C = 7: loss {float(plain.t[0]):.6f}, with gamma = 2 {float(focal.t[0]):.6f}")
    assert abs(float(focal.t[0]) - float(plain.t[0])) > 1e-3, "gamma = 2 does not change this loss: vacuous"
    lg, yd, y2d, lamd, wd = (t.to(gpu) for t in (logits, y, y2, lam, w))
    dloss = torch.tensor([DLOSS], device=gpu)

    def refused(what, pb, pl, e, gamma):
        loss, dl = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
        assert lib.d2r_ce_focal_fwd(lg.data_ptr(), yd.data_ptr(), pb, pl, wd.data_ptr(), e, gamma, B, C, loss.ptr, _st()) != 0
        msg = lib.d2r_last_error().decode()
        assert "d2r_ce_focal_fwd" in msg and what in msg, (what, msg)
        assert lib.d2r_ce_focal_bwd(lg.data_ptr(), yd.data_ptr(), pb, pl, wd.data_ptr(), e, gamma, B, C, dloss.data_ptr(), dl.ptr, _st()) != 0
        msg = lib.d2r_last_error().decode()
        assert "d2r_ce_focal_bwd" in msg and what in msg, (what, msg)
        torch.cuda.synchronize()
        assert _untouched(loss) and _untouched(dl), f"{what}: a refused call wrote to its output"

    for bad in (-0.5, float("nan"), float("inf")):
        refused("focal_gamma", y2d.data_ptr(), lamd.data_ptr(), eps, bad)
        refused("focal_gamma", None, None, 0.0, bad)
    for gamma in (0.0, 2.0):
        refused("labels_b and lam", y2d.data_ptr(), None, eps, gamma)
        refused("labels_b and lam", None, lamd.data_ptr(), eps, gamma)
        for bad in (-0.1, 1.0, float("nan")):
            refused("label_smoothing", y2d.data_ptr(), lamd.data_ptr(), bad, gamma)
    # the autograd function: the same numbers as the C calls, the gradient scaled by what arrives
    x = lg.clone().requires_grad_(True)
    out = F.cross_entropy(x, yd, wd, eps, labels_b=y2d, lam=lamd, focal_gamma=2.0)
    assert "_CrossEntropyFocal" in repr(out.grad_fn)
    (DLOSS * out).backward()
    assert float(out.detach()) == float(focal.t[0]) and torch.equal(x.grad, dfocal.t)
    x = lg.clone().requires_grad_(True)  # ... and without a pair
    out = F.cross_entropy(x, yd, focal_gamma=0.5)
    (DLOSS * out).backward()
    want = _run_ce(gpu, "focal", logits, y, None, None, None, 0.0, 0.5)
    assert float(out.detach()) == float(want[0].t[0]) and torch.equal(x.grad, want[1].t)
    x = lg.clone().requires_grad_(True)  # focal_gamma = 0: the function, and so the calls, of a call without the option
    out = F.cross_entropy(x, yd, wd, eps, labels_b=y2d, lam=lamd, focal_gamma=0.0)
    assert "_CrossEntropyMix" in repr(out.grad_fn) and float(out.detach()) == float(plain.t[0])


# ------------------------------------------------------------------------------------------------------
# the one-call head
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_labels", [False, True], ids=["one-label", "two-labels"])
def test_head_one_call_with_focal(gpu, two_labels):
    """The model of test_head_one_call_with_two_labels (1 + 1 layers, B = 3, C = 3, fp32, both loss options on) with focal_gamma = 2:
    the one-call head (d2r_head_focal_fwd / d2r_head_focal_bwd) and the op-by-op path make the same launches, so loss, logits and every
    parameter gradient are bit-identical; the loss against the fp64 model on the returned logits plus js."""
    from d2r_amd import _lib
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.params import ParamStore
    from oracle import d2r_oracle as O
    cfg = O.OracleConfig(text_layers=1, vision_layers=1, image_size=64, patch_size=32)
    sd = O.seeded_state_dict(cfg, seed=3, router_bias="normal")
    batch = tuple(t.to(gpu) for t in O.synthetic_batch(cfg, 3, 12, seed=4))
    labels = batch[3].cpu()
    labels_b, lam = ((labels + 1) % 3, torch.tensor([0.3, 1.0, 0.0])) if two_labels else (None, None)
    more = dict(labels_b=labels_b.to(gpu), mix_lam=lam.to(gpu)) if two_labels else {}
    weights, eps, gamma = [0.5, 2.0, 1.25], 0.1, 2.0
    res, names = {}, []
    real_call = _lib.call

    def recording_call(name, *a, **k):
        names.append(name)
        return real_call(name, *a, **k)

    for composite in (False, True):
        M.COMPOSITE_HEAD = composite
        _lib.call = recording_call
        del names[:]
        try:
            model = M.UnimoModelF(default_args(label_smoothing=eps, class_weights=weights, focal_gamma=gamma),
                                  VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                                  TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
            model.load_state_dict(sd, strict=True)
            model.to(gpu).set_compute_dtype(torch.float32).train()
            model.model.use_streams = False
            store = ParamStore(model, torch.float32)
            loss, logits = model(*batch, **more)
            assert ("_HeadBackward" in repr(loss.grad_fn)) == composite, loss.grad_fn
            (loss * 64.0).backward()
            torch.cuda.synchronize()
            res[composite] = (loss.detach().clone(), logits.detach().clone(), store.flat_g.clone(),
                              [(n, o, k) for n, _, o, k, _ in store.entries], model.last_aux["js_loss"].detach().clone())
            focal_calls = [n for n in names if "focal" in n]
            assert focal_calls == (["d2r_head_focal_fwd", "d2r_head_focal_bwd"] if composite else ["d2r_ce_focal_fwd", "d2r_ce_focal_bwd"])
            assert not [n for n in names if n.startswith("d2r_ce_") or n.startswith("d2r_head_")
                        if "focal" not in n], "a loss call without the focal term was made next to the focal one"
        finally:
            M.COMPOSITE_HEAD = True
            _lib.call = real_call
    (l0, g0, f0, ent, _), (l1, g1, f1, _, js) = res[False], res[True]
    assert torch.equal(l0, l1) and torch.equal(g0, g1), (float(l0), float(l1))
    bad = [n for n, o, k in ent if not torch.equal(f0[o:o + k], f1[o:o + k])]
    assert not bad, f"{len(bad)} parameter gradients differ, first {bad[:5]}"
    assert float(f1.abs().max()) > 0.0
    w64 = torch.tensor(weights, dtype=torch.float64)
    ref = focal_ce_model(g1, labels, labels_b, lam, w64, eps, gamma)[0] + js.double().cpu()
    plain = focal_ce_model(g1, labels, labels_b, lam, w64, eps, 0.0)[0] + js.double().cpu()
    print(f"head loss {float(l1):.7f} fp64 {float(ref):.7f} (with gamma = 0 {float(plain):.7f})")
    check("head.loss", l1, ref, torch.float32, scale=max(float(ref.abs()), 1.0))
    assert abs(float(plain) - float(ref)) > 1e-3, "gamma = 2 does not change this loss: vacuous"


# ------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------
W3 = [0.5, 2.0, 1.25]


def _train(dev=False, **args_kw):
    """A few fp32 steps of the tiny model of the trainer tests on synthetic data, as test_gpu_mix.py's; -> (trainer, records of every
    training and dev step, names of every library call made)."""
    from d2r_amd import _lib
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.train import MSDTrainer
    torch.manual_seed(0)
    mk = lambda n, s, sh: make_loader(SyntheticMSDDataset(n, 16, 64, 3, seed=s, num_image_tokens=5), 4, sh, 0, drop_last=sh)
    args = default_args(DR_step=3, compute_dtype=torch.float32, device="cuda:0", num_epochs=1, batch_size=4, warmup_ratio=0.0,
                        save_path=None, lr=1e-4, label_smoothing=0.1, class_weights=W3, eval_begin_epoch=99, **args_kw)
    model = M.UnimoModelF(args, VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                          TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
    logger = logging.getLogger("focal-test")
    logger.handlers[:] = []
    logger.setLevel(logging.INFO)
    tr = MSDTrainer(train_data=mk(16, 1, True), dev_data=mk(10, 2, False) if dev else None, test_data=None, model=model,
                    args=args, logger=logger, writer=None)
    records, names = [], []
    step, real_call = tr._step, _lib.call

    def recording_step(batch, mode="train"):
        (loss, logits), labels = step(batch, mode)
        records.append(dict(mode=mode, labels=labels.detach().clone(), loss=loss.detach().clone(), logits=logits.detach().clone(),
                            js=tr.model.last_aux["js_loss"].detach().clone()))
        return (loss, logits), labels

    def recording_call(name, *a, **k):
        names.append(name)
        return real_call(name, *a, **k)

    tr._step = recording_step
    _lib.call = recording_call
    try:
        tr.train(None, None)
        if dev:
            tr.evaluate(1)
        torch.cuda.synchronize()
    finally:
        _lib.call = real_call
    return tr, records, names


def _fp64_loss(rec, gamma):
    return focal_ce_model(rec["logits"], rec["labels"], None, None, torch.tensor(W3, dtype=torch.float64), 0.1, gamma)[0] + rec["js"].double().cpu()


@pytest.fixture(scope="module")
def runs(gpu):
    return dict(absent=_train(), zero=_train(focal_gamma=0.0), on=_train(dev=True, focal_gamma=2.0))


def test_trainer_without_the_flag_is_what_it_was(runs):
    """args without focal_gamma (every caller from before the option) and focal_gamma = 0: no call with `focal` in its name, the same
    weights bit for bit, and every step's loss is the smoothed, weighted cross entropy of its logits plus js."""
    (a, rec_a, names_a), (z, rec_z, names_z) = runs["absent"], runs["zero"]
    assert a.model.focal_gamma == 0.0 and z.model.focal_gamma == 0.0
    assert len(rec_a) == len(rec_z) == 4 and names_a == names_z
    assert not [n for n in names_a if "focal" in n], "a focal call without the flag"
    assert "d2r_head_fwd" in names_a and "d2r_head_bwd" in names_a
    assert torch.equal(a.store.flat_w, z.store.flat_w)
    assert [float(r["loss"]) for r in rec_a] == [float(r["loss"]) for r in rec_z]
    for r in rec_a:
        ref = mixed_ce_model(r["logits"], r["labels"], r["labels"], torch.ones(4), torch.tensor(W3, dtype=torch.float64), 0.1)[0] \
            + r["js"].double().cpu()
        check("step loss", r["loss"], ref, torch.float32, scale=max(float(ref.abs()), 1.0))


def test_trainer_with_the_flag_trains_and_evaluates_on_the_focal_loss(runs):
    (a, rec_a, _), (on, rec, names) = runs["absent"], runs["on"]
    assert on.model.focal_gamma == 2.0
    train, dev = [r for r in rec if r["mode"] == "train"], [r for r in rec if r["mode"] == "dev"]
    assert len(train) == 4 and len(dev) == 3
    assert names.count("d2r_head_focal_fwd") == 7 and names.count("d2r_head_focal_bwd") == 4
    assert not [n for n in names if n in ("d2r_head_fwd", "d2r_head_bwd", "d2r_head_mix_fwd", "d2r_head_mix_bwd")]
    assert torch.equal(train[0]["logits"], rec_a[0]["logits"])  # the first forward is the same; the loss is not
    assert not torch.equal(a.store.flat_w, on.store.flat_w)
    for r in train + dev:
        ref, plain = _fp64_loss(r, 2.0), _fp64_loss(r, 0.0)
        print(f"{r['mode']} loss {float(r['loss']):.7f} fp64 {float(ref):.7f} (with gamma = 0 {float(plain):.7f})")
        check(r["mode"] + " step loss", r["loss"], ref, torch.float32, scale=max(float(ref.abs()), 1.0))
        assert abs(float(plain) - float(ref)) > 1e-3, "gamma = 2 does not change this loss: vacuous"
    # the dev result's loss is the sum of the dev batches' focal losses
    want = sum(_fp64_loss(r, 2.0) for r in dev)
    check("dev loss", torch.tensor(on.last_dev_result["loss"]), want, torch.float32, scale=max(float(want.abs()), 1.0))
    assert sum(map(sum, on.last_dev_result["confusion"])) == 10


def test_cli_trains_with_the_flag_and_logs_it(gpu, caplog, tmp_path):
    from d2r_amd import run
    argv = ["--num_epochs", "1", "--train_samples", "8", "--eval_samples", "4", "--batch_size", "4", "--encoder_layers", "1",
            "--image_size", "64", "--max_seq", "16", "--num_workers", "0", "--focal_gamma", "2", "--label_smoothing", "0.1",
            "--aug_mixup", "0.8", "--save_path", str(tmp_path) + "/"]
    with caplog.at_level(logging.INFO):
        run.main(argv)
    text = "\n".join(r.getMessage() for r in caplog.records)
    assert "cross entropy: class weights None, label smoothing 0.1, focal gamma 2" in text
    assert "MixUp / CutMix of the training batches" in text and "Dev Eval results" in text
