"""GPU: MixUp / CutMix.  d2r_image_mix against the selected inputs bit for bit and the blend against fp64, on the vector and the scalar
path; d2r_ce_mix_fwd / d2r_ce_mix_bwd against the fp64 model of test_mix_host.py and, where lam == 1 or the pair is NULL, against
d2r_ce_*_ex bit for bit; the two labels inside the one-call head; the trainer with a Mixer.

Branch                                                          Test
--------------------------------------------------------------  ------------------------------------------------------------
float4 path / scalar path (odd S, out or in off 16 bytes),      test_image_mix[*]
  identity, blend, full / empty / corner / unaligned box,
  shared partner, partner == self, several workgroups (S = 224)
every refusal: nothing launched, nothing written                test_image_mix_refusals
ce_mix thread loop (B > 256), multi-block bwd, the four         test_cross_entropy_mix[*]
  options x lam all 1 / all 0 / random / y2 == y; lam == 1 and
  NULL pair = the _ex kernels' bits; half a pair refused
head: d2r_head_mix_desc, one call = op by op                    test_head_one_call_with_two_labels
trainer: off = as before, on = other weights and the mixed      test_trainer_*
  loss, same default-generator draws, dev pass untouched"""
import logging

import pytest
import torch

from test_gpu_kernel_edges import Guarded, _st, call, check
from test_mix_host import mixed_ce_model

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------
# d2r_image_mix
# ------------------------------------------------------------------------------------------------------
KINDS = ("identity", "mixup", "full", "empty", "corner", "unaligned", "shared", "self")


def _f32_bits(v):
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32)[0])


def _desc_row(kind, b, B, S):
    """{partner, bits of a, x0, y0, w, h, 0, 0} of sample b of a batch of B.  `other` is sample 0 (B - 1 for sample 0 itself), so
    two samples of a batch of three or more share a partner; "shared" always names sample 0."""
    other = (B - 1) if b == 0 else 0
    half = max(1, S // 2)
    ux, uy = min(3, S - 1), min(2, S - 1)
    uw, uh = max(1, min(S - ux - 1, 22)), max(1, min(S - uy - 1, 9))  # S = 8: columns 3..6, rows 2..6; S = 224: columns 3..24
    partner, a, box = {
        "identity": (b, 1.0, (0, 0, 0, 0)),
        "mixup": (other, 0.3, (0, 0, 0, 0)),
        "full": (other, 1.0, (0, 0, S, S)),
        "empty": (other, 1.0, (min(1, S), 0, 0, S)),       # w == 0 with a full height: still empty -> a copy of the sample's own
        "corner": (other, 1.0, (S - half, S - half, half, half)),
        "unaligned": (other, 0.3, (ux, uy, uw, uh)),       # a blend outside the box, the partner inside
        "shared": (0, 0.5, (0, 0, 0, 0)),
        "self": (b, 0.3, (0, 0, half, 1)),
    }[kind]
    return [partner, _f32_bits(a), *box, 0, 0]


def _mix_reference(x, desc):
    """(fp64 expected values, mask of the elements that must carry the selected input's bits) for fp32 x [B, 3, S, S] on the host."""
    B, _, S, _ = x.shape
    want = torch.empty(B, 3, S, S, dtype=torch.float64)
    exact = torch.zeros(B, 3, S, S, dtype=torch.bool)
    a32 = desc[:, 1].contiguous().view(torch.float32)
    for b in range(B):
        partner, _, x0, y0, w, h = desc[b, :6].tolist()
        a = float(a32[b])  # the fp32 value
        own, other = x[b].double(), x[partner].double()
        want[b] = own if a == 1.0 else a * own + (1.0 - a) * other
        exact[b] = a == 1.0
        want[b, :, y0:y0 + h, x0:x0 + w] = other[:, y0:y0 + h, x0:x0 + w]
        exact[b, :, y0:y0 + h, x0:x0 + w] = True
    return want, exact


def _run_mix(gpu, xin, desc, out_shift):
    B, _, S, _ = xin.shape
    out = Guarded(gpu, torch.float32, B * 3 * S * S, shift=out_shift)
    call("d2r_image_mix", xin.data_ptr(), out.ptr, B, S, desc.data_ptr(), desc.to(gpu).data_ptr(), _st())
    torch.cuda.synchronize()
    return out


MIX_SHAPES = [(S, B) for S in (1, 3, 4, 7, 8, 32) for B in (1, 2, 5)] + [(224, 2)]


@pytest.mark.parametrize("shift", [(0, 0), (0, 1), (1, 0)], ids=["aligned", "out+1", "in+1"])
@pytest.mark.parametrize("S,B", MIX_SHAPES, ids=[f"S{s}-B{b}" for s, b in MIX_SHAPES])
def test_image_mix(gpu, S, B, shift):
    in_shift, out_shift = shift
    g = torch.Generator().manual_seed(S * 10 + B)
    n = B * 3 * S * S
    calls = -(-len(KINDS) // B)
    kinds = [KINDS[i % len(KINDS)] for i in range(calls * B)]
    seen_shared = False
    for c in range(calls):
        x = 3.0 * torch.randn(B, 3, S, S, generator=g)
        store = torch.empty(n + 4, device=gpu)
        xin = store[in_shift:in_shift + n].view(B, 3, S, S)  # in_shift = 1: four bytes past a 16-byte boundary
        xin.copy_(x)
        assert xin.data_ptr() % 16 == 4 * in_shift
        desc = torch.tensor([_desc_row(kinds[c * B + b], b, B, S) for b in range(B)], dtype=torch.int32)
        partners = desc[:, 0].tolist()
        seen_shared = seen_shared or len(set(partners)) < B
        tag = f"image_mix[S={S} B={B} {shift} call {c}: {kinds[c * B:(c + 1) * B]}]"
        out = _run_mix(gpu, xin, desc, out_shift)
        out.intact(tag)
        again = _run_mix(gpu, xin, desc, out_shift)
        assert torch.equal(out.buf.view(torch.int32), again.buf.view(torch.int32)), tag + ": two runs differ"
        assert torch.equal(xin.cpu(), x), tag + ": the input was written"
        got = out.t.view(B, 3, S, S).cpu()
        want, exact = _mix_reference(x, desc)
        assert torch.equal(got[exact].view(torch.int32), want[exact].float().view(torch.int32)), tag + ": a copied element is not bit-equal"
        if bool((~exact).any()):
            check(tag + ".blend", got[~exact], want[~exact], torch.float32, scale=float(x.abs().max()))
    assert seen_shared or B == 1, "no batch of this shape had two samples with one partner"


def test_image_mix_functional_and_mixer_apply(gpu):
    """F.image_mix returns a new tensor and leaves its input alone; Mixer.apply mixes with its own draw and picks the partners' labels."""
    from d2r_amd import _lib
    from d2r_amd import functional as F
    from d2r_amd.mix import Mixer
    B, S = 6, 8
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(1))
    xg, labels = x.to(gpu), torch.arange(B, device=gpu) % 3
    desc, lam = Mixer(S, 0.8, 1.0, 1.0, seed=3).draw(B)
    mixed, y, y2, lam_d = Mixer(S, 0.8, 1.0, 1.0, seed=3).apply(xg, labels)
    torch.cuda.synchronize()
    assert mixed.data_ptr() != xg.data_ptr() and torch.equal(xg.cpu(), x) and y is labels
    assert torch.equal(y2.cpu(), labels.cpu()[desc[:, 0].long()]) and torch.equal(lam_d.cpu(), lam) and lam_d.dtype == torch.float32
    want, exact = _mix_reference(x, desc)
    assert torch.equal(mixed.cpu()[exact], want[exact].float())
    check("mixer.apply", mixed.cpu()[~exact], want[~exact], torch.float32, scale=float(x.abs().max()))
    assert torch.equal(F.image_mix(xg, desc, desc.to(gpu)), mixed)
    with pytest.raises(_lib.D2RError):
        F.image_mix(xg.double(), desc, desc.to(gpu))
    with pytest.raises(_lib.D2RError):
        F.image_mix(xg, desc[:3], desc.to(gpu))
    with pytest.raises(ValueError):
        Mixer(16, 0.8, 0.0).apply(xg, labels)


def test_image_mix_refusals(gpu):
    from d2r_amd import _lib
    lib = _lib.load()
    B, S = 2, 4
    n = B * 3 * S * S
    store = torch.randn(2 * n + 8, device=gpu)
    xin = store[:n]
    good = [[1, _f32_bits(0.5), 1, 1, 2, 2, 0, 0], [0, _f32_bits(1.0), 0, 0, 0, 0, 0, 0]]

    def refused(what, *, B=B, S=S, row=None, in_ptr=None, out_ptr=None, desc_off=0):
        rows = [list(r) for r in good]
        if row is not None:
            rows[1] = row
        h = torch.tensor(rows, dtype=torch.int32)
        dbuf = torch.zeros(h.numel() + 4, dtype=torch.int32, device=gpu)
        dbuf[:h.numel()] = h.view(-1)
        out = Guarded(gpu, torch.float32, n)
        rc = lib.d2r_image_mix(xin.data_ptr() if in_ptr is None else in_ptr, out.ptr if out_ptr is None else out_ptr, B, S,
                               h.data_ptr(), dbuf.data_ptr() + desc_off, _st())
        msg = lib.d2r_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        assert what in msg, (what, msg)
        assert bool((out.buf.view(out.it) == out.sent).all()), f"{what}: a refused call wrote to its output"
        return msg

    half = _f32_bits(0.5)
    assert "sample 1" in refused("partner", row=[-1, half, 0, 0, 0, 0, 0, 0])
    assert "sample 1" in refused("partner", row=[B, half, 0, 0, 0, 0, 0, 0])
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        assert "sample 1" in refused("a is", row=[0, _f32_bits(bad), 0, 0, 0, 0, 0, 0])
    assert "sample 1" in refused("w is", row=[0, half, 0, 0, -1, 2, 0, 0])
    assert "sample 1" in refused("h is", row=[0, half, 0, 0, 2, -1, 0, 0])
    for box in ((3, 0, 2, 1), (0, 3, 1, 2), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, S + 1, 1), (S + 1, 0, 0, 0), (0, S + 1, 0, 0)):
        assert "sample 1" in refused("box", row=[0, half, *box, 0, 0])
    refused("overlaps", out_ptr=xin.data_ptr())                 # in place
    refused("overlaps", out_ptr=xin.data_ptr() + 4 * (n - 1))   # the last element of in is the first of out
    refused("overlaps", in_ptr=xin.data_ptr() + 4 * (n - 1), out_ptr=xin.data_ptr())
    refused("aligned", in_ptr=xin.data_ptr() + 2)
    refused("aligned", out_ptr=store.data_ptr() + 4 * n + 2)
    refused("aligned", desc_off=2)
    refused("batch", B=0)
    refused("batch", B=65536)
    refused("crop size", S=0)
    refused("crop size", S=4097)
    refused("null", in_ptr=0)
    out = Guarded(gpu, torch.float32, n)  # and the same descriptors are accepted when nothing is wrong; out may follow in directly
    h = torch.tensor(good, dtype=torch.int32)
    assert lib.d2r_image_mix(xin.data_ptr(), out.ptr, B, S, h.data_ptr(), h.to(gpu).data_ptr(), _st()) == 0
    assert lib.d2r_image_mix(xin.data_ptr(), xin.data_ptr() + 4 * n, B, S, h.data_ptr(), h.to(gpu).data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    out.intact("accepted")


# ------------------------------------------------------------------------------------------------------
# d2r_ce_mix_fwd / d2r_ce_mix_bwd
# ------------------------------------------------------------------------------------------------------
BS, CS = (1, 2, 255, 256, 257, 600), (1, 2, 3, 7)  # the grid of test_gpu_loss_metrics.py
CE_SHAPES = [(B, C) for B in BS for C in CS]
CE_OPTIONS = ["plain", "w", "eps", "w+eps"]
LAMS = ["ones", "zeros", "random", "same"]
DLOSS = -1.7


def _ce_case(B, C, option):
    eps = {"plain": 0.0, "w": 0.0, "eps": 0.1, "w+eps": 0.1}[option]
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = 80.0 * (2.0 * torch.rand(B, C, generator=g) - 1.0)
    y, y2 = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    w = 0.25 + 2.0 * torch.rand(C, generator=g) if option in ("w", "w+eps") else None  # every weight positive: every W is
    return logits, y, y2, torch.rand(B, generator=g), w, eps


def _run_ce(gpu, name, logits, y, y2, lam, w, eps):
    """name: "mix" (y2 / lam may be None: NULL) or "ex"."""
    B, C = logits.shape
    lg, yd = logits.to(gpu), y.to(gpu)
    y2d, lamd, wd = (None if t is None else t.to(gpu) for t in (y2, lam, w))
    p = lambda t: None if t is None else t.data_ptr()
    loss, dl = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
    dloss = torch.tensor([DLOSS], device=gpu)
    if name == "mix":
        call("d2r_ce_mix_fwd", lg.data_ptr(), yd.data_ptr(), p(y2d), p(lamd), p(wd), eps, B, C, loss.ptr, _st())
        call("d2r_ce_mix_bwd", lg.data_ptr(), yd.data_ptr(), p(y2d), p(lamd), p(wd), eps, B, C, dloss.data_ptr(), dl.ptr, _st())
    else:
        call("d2r_ce_fwd_ex", lg.data_ptr(), yd.data_ptr(), p(wd), eps, B, C, loss.ptr, _st())
        call("d2r_ce_bwd_ex", lg.data_ptr(), yd.data_ptr(), p(wd), eps, B, C, dloss.data_ptr(), dl.ptr, _st())
    torch.cuda.synchronize()
    return loss, dl


def _same_bits(a, b):
    return torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))


@pytest.mark.parametrize("option", CE_OPTIONS)
@pytest.mark.parametrize("B,C", CE_SHAPES, ids=[f"B{b}-C{c}" for b, c in CE_SHAPES])
def test_cross_entropy_mix(gpu, B, C, option):
    logits, y, y2, lam_r, w, eps = _ce_case(B, C, option)
    w64 = None if w is None else w.double()
    wmax = 1.0 if w is None else float(w64.max())
    for pattern in LAMS:
        lam = {"ones": torch.ones(B), "zeros": torch.zeros(B), "random": lam_r, "same": lam_r}[pattern]
        yb = y if pattern == "same" else y2
        tag = f"ce_mix[B={B} C={C} {option} lam {pattern}]"
        loss, dl = _run_ce(gpu, "mix", logits, y, yb, lam, w, eps)
        loss.intact(tag + ".loss")
        dl.intact(tag + ".dlogits")
        loss2, dl2 = _run_ce(gpu, "mix", logits, y, yb, lam, w, eps)
        assert _same_bits(loss, loss2) and _same_bits(dl, dl2), tag + ": two runs differ"
        ref, dref, W = mixed_ce_model(logits, y, yb, lam, w64, eps, dloss=DLOSS)
        print(f"{tag}: loss {float(loss.t[0]):.6f} ref {float(ref):.6f} err {abs(float(loss.t[0]) - float(ref)):.2e}; dlogits max err "
              f"{float((dl.t.double().cpu() - dref).abs().max()):.2e}")
        check(tag + ".loss", loss.t[0], ref, torch.float32, scale=max(float(ref.abs()), 1.0))
        check(tag + ".dlogits", dl.t, dref, torch.float32, scale=1.7 * wmax / W)
        if pattern == "ones":  # the formula of the _ex kernels exactly: their bits, and with a NULL pair their launches
            loss_ex, dl_ex = _run_ce(gpu, "ex", logits, y, None, None, w, eps)
            assert _same_bits(loss, loss_ex), (tag, float(loss.t[0]), float(loss_ex.t[0]))
            assert _same_bits(dl, dl_ex), (tag, float((dl.t - dl_ex.t).abs().max()))
            loss_n, dl_n = _run_ce(gpu, "mix", logits, y, None, None, w, eps)
            assert _same_bits(loss_n, loss_ex) and _same_bits(dl_n, dl_ex), tag + ": NULL labels_b / lam differ from d2r_ce_*_ex"


def test_cross_entropy_mix_is_not_vacuous_and_refuses_half_a_pair(gpu):
    from d2r_amd import _lib
    from d2r_amd import functional as F
    lib = _lib.load()
    B, C = 257, 7
    logits, y, y2, lam, w, eps = _ce_case(B, C, "w+eps")
    mixed, _ = _run_ce(gpu, "mix", logits, y, y2, lam, w, eps)
    unmixed, _ = _run_ce(gpu, "ex", logits, y, None, None, w, eps)
    assert abs(float(mixed.t[0]) - float(unmixed.t[0])) > 1e-3, "the second labels do not change this loss: vacuous"
    lg, yd, y2d, lamd = logits.to(gpu), y.to(gpu), y2.to(gpu), lam.to(gpu)
    dloss = torch.tensor([DLOSS], device=gpu)
    for pb, pl in ((y2d.data_ptr(), None), (None, lamd.data_ptr())):
        loss, dl = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, C)
        assert lib.d2r_ce_mix_fwd(lg.data_ptr(), yd.data_ptr(), pb, pl, None, 0.0, B, C, loss.ptr, _st()) != 0
        assert "labels_b and lam" in lib.d2r_last_error().decode()
        assert lib.d2r_ce_mix_bwd(lg.data_ptr(), yd.data_ptr(), pb, pl, None, 0.0, B, C, dloss.data_ptr(), dl.ptr, _st()) != 0
        torch.cuda.synchronize()
        for g in (loss, dl):
            assert bool((g.buf.view(g.it) == g.sent).all()), "a refused call wrote to its output"
    for bad in (-0.1, 1.0):
        loss = Guarded(gpu, torch.float32, 1)
        assert lib.d2r_ce_mix_fwd(lg.data_ptr(), yd.data_ptr(), y2d.data_ptr(), lamd.data_ptr(), None, bad, B, C, loss.ptr, _st()) != 0
        assert "label_smoothing" in lib.d2r_last_error().decode()
    # the autograd function: the same numbers as the C calls, the gradient scaled by what arrives
    x = lg.clone().requires_grad_(True)
    out = F.cross_entropy(x, yd, w.to(gpu), eps, labels_b=y2d, lam=lamd)
    (DLOSS * out).backward()
    _, dl = _run_ce(gpu, "mix", logits, y, y2, lam, w, eps)
    assert float(out.detach()) == float(mixed.t[0]) and torch.equal(x.grad, dl.t)


# ------------------------------------------------------------------------------------------------------
# the one-call head
# ------------------------------------------------------------------------------------------------------
def test_head_one_call_with_two_labels(gpu):
    """The model of test_head_one_call_with_loss_options (1 + 1 layers, B = 3, C = 3, fp32, both loss options on) with labels_b /
    mix_lam: the one-call head (d2r_head_mix_fwd / d2r_head_mix_bwd) and the op-by-op path make the same launches, so loss, logits
    and every parameter gradient are bit-identical; the loss against the fp64 model on the returned logits plus js."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.params import ParamStore
    from oracle import d2r_oracle as O
    cfg = O.OracleConfig(text_layers=1, vision_layers=1, image_size=64, patch_size=32)
    sd = O.seeded_state_dict(cfg, seed=3, router_bias="normal")
    batch = tuple(t.to(gpu) for t in O.synthetic_batch(cfg, 3, 12, seed=4))
    labels = batch[3].cpu()
    labels_b = ((labels + 1) % 3)
    lam = torch.tensor([0.3, 1.0, 0.0])
    weights, eps = [0.5, 2.0, 1.25], 0.1
    res = {}
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
            loss, logits = model(*batch, labels_b=labels_b.to(gpu), mix_lam=lam.to(gpu))
            assert ("_HeadBackward" in repr(loss.grad_fn)) == composite, loss.grad_fn
            (loss * 64.0).backward()
            torch.cuda.synchronize()
            res[composite] = (loss.detach().clone(), logits.detach().clone(), store.flat_g.clone(),
                              [(n, o, k) for n, _, o, k, _ in store.entries], model.last_aux["js_loss"].detach().clone())
            if composite:
                with pytest.raises(ValueError):
                    model(*batch, labels_b=labels_b.to(gpu))
                with torch.no_grad(), pytest.raises(ValueError):
                    model(batch[0], batch[1], batch[2], None, batch[4], labels_b=labels_b.to(gpu), mix_lam=lam.to(gpu))
        finally:
            M.COMPOSITE_HEAD = True
    (l0, g0, f0, ent, _), (l1, g1, f1, _, js) = res[False], res[True]
    assert torch.equal(l0, l1) and torch.equal(g0, g1), (float(l0), float(l1))
    bad = [n for n, o, k in ent if not torch.equal(f0[o:o + k], f1[o:o + k])]
    assert not bad, f"{len(bad)} parameter gradients differ, first {bad[:5]}"
    assert float(f1.abs().max()) > 0.0
    w64 = torch.tensor(weights, dtype=torch.float64)
    ref = mixed_ce_model(g1, labels, labels_b, lam, w64, eps)[0] + js.double().cpu()
    unmixed = torch.nn.functional.cross_entropy(g1.double().cpu(), labels, weight=w64, label_smoothing=eps) + js.double().cpu()
    print(f"head loss {float(l1):.7f} fp64 {float(ref):.7f} (with one label per row {float(unmixed):.7f})")
    check("head.loss", l1, ref, torch.float32, scale=max(float(ref.abs()), 1.0))
    assert abs(float(unmixed) - float(ref)) > 1e-3, "the second labels do not change this loss: vacuous"


# ------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------
def _train(mixer, seed=0, steps_data=16, dev=False, train=True, **trainer_kw):
    """A few steps of the tiny model of the trainer tests on synthetic data (fp32); -> (trainer, records of every training step)."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.train import MSDTrainer
    torch.manual_seed(seed)
    mk = lambda n, s, sh: make_loader(SyntheticMSDDataset(n, 16, 64, 3, seed=s, num_image_tokens=5), 4, sh, 0, drop_last=sh)
    args = default_args(DR_step=3, compute_dtype=torch.float32, device="cuda:0", num_epochs=1, batch_size=4, warmup_ratio=0.0,
                        save_path=None, lr=1e-4, label_smoothing=0.1, class_weights=[0.5, 2.0, 1.25], eval_begin_epoch=99)
    model = M.UnimoModelF(args, VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                          TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
    logger = logging.getLogger("mix-test")
    lines = []

    class Catch(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())

    logger.handlers[:] = [Catch()]
    logger.setLevel(logging.INFO)
    if mixer != "absent":
        trainer_kw["mixer"] = mixer
    tr = MSDTrainer(train_data=mk(steps_data, 1, True), dev_data=mk(10, 2, False) if dev else None, test_data=None, model=model,
                    args=args, logger=logger, writer=None, **trainer_kw)
    records = []
    step = tr._step

    def recording_step(batch, mode="train"):
        (loss, logits), labels = step(batch, mode)
        if mode == "train":
            records.append(dict(batch=[t.detach().clone() for t in batch], loss=loss.detach().clone(), logits=logits.detach().clone(),
                                js=tr.model.last_aux["js_loss"].detach().clone()))
        return (loss, logits), labels

    tr._step = recording_step
    if train:
        tr.train(None, None)
        torch.cuda.synchronize()
    tr.lines = lines
    return tr, records


def _mixer(**kw):
    from d2r_amd.mix import Mixer
    return Mixer(64, kw.pop("mixup", 0.8), kw.pop("cutmix", 1.0), kw.pop("prob", 1.0), seed=0, rank=0)


@pytest.fixture(scope="module")
def runs(gpu):
    absent, rec_absent = _train("absent")
    rng_absent = torch.get_rng_state().clone()
    none, _ = _train(None)
    on, rec_on = _train(_mixer())
    rng_on = torch.get_rng_state().clone()
    return dict(absent=absent, rec_absent=rec_absent, rng_absent=rng_absent, none=none, on=on, rec_on=rec_on, rng_on=rng_on)


def test_trainer_without_a_mixer_is_what_it_was(runs, monkeypatch):
    """mixer=None and a trainer built without the keyword (the call run.main makes with the flags off) end on the same bits; so
    does a Mixer that mixes no sample (prob = 0): identity copies and lam == 1 rows have the unmixed kernels' bits."""
    a, b = runs["absent"], runs["none"]
    assert a.mixer is None and b.mixer is None and all(len(r["batch"]) == 6 for r in runs["rec_absent"])
    assert torch.equal(a.store.flat_w, b.store.flat_w) and len(runs["rec_absent"]) == 4
    assert not any("MixUp" in line for line in a.lines)
    idle, rec = _train(_mixer(prob=0.0))
    assert all(len(r["batch"]) == 8 and bool((r["batch"][7] == 1).all()) for r in rec)
    assert torch.equal(a.store.flat_w, idle.store.flat_w)
    assert [float(r["loss"]) for r in rec] == [float(r["loss"]) for r in runs["rec_absent"]]


def test_trainer_with_a_mixer_trains_on_the_mixed_loss(runs):
    a, on, rec_a, rec = runs["absent"], runs["on"], runs["rec_absent"], runs["rec_on"]
    # the default generator (sampler order, dropout seeds) is drawn from exactly as without the flags
    assert torch.equal(runs["rng_absent"], runs["rng_on"])
    assert len(rec) == len(rec_a) == 4 and all(torch.equal(r["batch"][0], s["batch"][0]) and torch.equal(r["batch"][4], s["batch"][4])
                                               for r, s in zip(rec, rec_a))
    assert not torch.equal(a.store.flat_w, on.store.flat_w)
    assert sum("MixUp / CutMix of the training batches" in line for line in on.lines) == 1
    # step 1: the images are the mixer's own first draw applied to the unmixed images; the loss is the fp64 model's on the logits
    first, plain = rec[0], rec_a[0]
    desc, lam = _mixer().draw(4)
    labels, labels_b, lam_d = first["batch"][4].cpu(), first["batch"][6].cpu(), first["batch"][7].cpu()
    assert torch.equal(lam_d, lam) and torch.equal(labels_b.view(-1), labels.view(-1)[desc[:, 0].long()])
    want, exact = _mix_reference(plain["batch"][5].cpu(), desc)
    got = first["batch"][5].cpu()
    assert torch.equal(got[exact], want[exact].float()) and not torch.equal(got, plain["batch"][5].cpu())
    w64 = torch.tensor([0.5, 2.0, 1.25], dtype=torch.float64)
    ref = mixed_ce_model(first["logits"], labels, labels_b, lam_d, w64, 0.1)[0] + first["js"].double().cpu()
    unmixed = mixed_ce_model(first["logits"], labels, labels, torch.ones(4), w64, 0.1)[0] + first["js"].double().cpu()
    print(f"step 1 loss {float(first['loss']):.7f} fp64 {float(ref):.7f} (with one label per row {float(unmixed):.7f})")
    check("step 1 loss", first["loss"], ref, torch.float32, scale=max(float(ref.abs()), 1.0))
    assert abs(float(unmixed) - float(ref)) > 1e-3, "the second labels do not change this loss: vacuous"


def test_trainer_dev_pass_never_sees_the_mixer(gpu):
    res = []
    for mixer in ("absent", _mixer()):
        tr, records = _train(mixer, dev=True, train=False)
        tr.evaluate(1)
        assert records == [] and tr.last_dev_result is not None
        res.append(tr.last_dev_result)
        if tr.mixer is not None:
            assert tr.mixer.batches == 0  # nothing was drawn
    assert res[0]["loss"] == res[1]["loss"] and res[0]["confusion"] == res[1]["confusion"]
    assert sum(map(sum, res[0]["confusion"])) == 10


def test_cli_trains_with_the_flags_and_logs_the_mixer(gpu, caplog, tmp_path):
    from d2r_amd import run
    argv = ["--num_epochs", "1", "--train_samples", "8", "--eval_samples", "4", "--batch_size", "4", "--encoder_layers", "1",
            "--image_size", "64", "--max_seq", "16", "--num_workers", "0", "--aug_mixup", "0.8", "--aug_cutmix", "1.0",
            "--save_path", str(tmp_path) + "/"]
    with caplog.at_level(logging.INFO):
        run.main(argv)
    text = "\n".join(r.getMessage() for r in caplog.records)
    assert "MixUp / CutMix of the training batches: MixUp with lam ~ Beta(0.8, 0.8); CutMix with lam ~ Beta(1, 1)" in text
