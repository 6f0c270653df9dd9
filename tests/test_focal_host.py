"""Focal loss on the host (no GPU): the fp64 model of d2r_ce_focal_fwd / d2r_ce_focal_bwd that the GPU tests (test_gpu_focal.py) compare
the kernels with - against fp64 autograd of the definition, the usual one-line focal loss and, at gamma == 0, the mixed-label model -
the C ABI of the four new entry points, the refusals that need no launch, the command-line flag and run.main's wiring."""
import ctypes
import logging
import os
import re

import pytest
import torch

from test_mix_host import _StubTrainer, mixed_ce_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d2r_ce_focal_fwd", "d2r_ce_focal_bwd", "d2r_head_focal_fwd", "d2r_head_focal_bwd")


# ------------------------------------------------------------------------------------------------------
# the fp64 model (imported by test_gpu_focal.py)
# ------------------------------------------------------------------------------------------------------
def _targets(B, C, labels, labels_b, lam):
    """(t, 1 - t) as fp64 [B, C], each written from its own terms: t_b = lam_b onehot(y_b) + (1 - lam_b) onehot(y2_b), the one-hot of
    y_b without a pair or where the two labels are one class; 1 - t_b is then exactly 0 at the target, never a rounded difference."""
    y = labels.cpu().view(-1).long()
    rows = torch.arange(B)
    t, nt = torch.zeros(B, C, dtype=torch.float64), torch.ones(B, C, dtype=torch.float64)
    if labels_b is None:
        assert lam is None
        t[rows, y], nt[rows, y] = 1.0, 0.0
        return t, nt
    y2, lam = labels_b.cpu().view(-1).long(), lam.detach().cpu().view(-1).double()
    same = y2 == y
    t[rows, y], nt[rows, y] = torch.where(same, torch.ones_like(lam), lam), torch.where(same, torch.zeros_like(lam), 1.0 - lam)
    two = ~same
    t[rows[two], y2[two]], nt[rows[two], y2[two]] = (1.0 - lam)[two], lam[two]
    return t, nt


def focal_ce_model(logits, labels, labels_b=None, lam=None, weight=None, eps=0.0, gamma=0.0, dloss=1.0):
    """(loss, dlogits, W) in fp64 from the formulas of include/d2r_hip.h, written out term by term (no autograd):
        a_b(c) = (1-e) w[c] t_b(c) + (e/C) w[c],  row_b = sum_c a_b(c) (-lp[b,c]),  q_b = sum_c t_b(c) p[b,c],
        u_b = sum_c (1 - t_b(c)) p[b,c],  W = sum_b sum_c t_b(c) w[c],  loss = sum_b u_b^g row_b / W,
        dlogits[b,c] = dloss / W (u_b^g (p[b,c] sum_k a_b(k) - a_b(c)) - g u_b^g row_b (p[b,c] t_b(c) - r_b(c) q_b)),
        r_b(c) = p[b,c] (1 - t_b(c)) / u_b;  u_b == 0: u_b^g = 0 and r_b = 0 for g > 0 (u_b^0 = 1)."""
    x = logits.detach().double().cpu()
    B, C = x.shape
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().double().cpu()
    t, nt = _targets(B, C, labels, labels_b, lam)
    lp = x - torch.logsumexp(x, dim=1, keepdim=True)
    p = lp.exp()
    a = (1.0 - eps) * w * t + (eps / C) * w.expand(B, C)
    row = (a * -lp).sum(1)
    q = (t * p).sum(1)
    u = (nt * p).sum(1)
    live = u > 0
    safe_u = torch.where(live, u, torch.ones_like(u))
    ug = torch.where(live, safe_u ** gamma, torch.full_like(u, 1.0 if gamma == 0 else 0.0))
    r = torch.where(live[:, None], p * nt / safe_u[:, None], torch.zeros_like(p))
    W = float((t * w).sum())
    loss = float((ug * row).sum()) / W
    dlogits = dloss / W * (ug[:, None] * (p * a.sum(1, keepdim=True) - a) - (gamma * ug * row)[:, None] * (p * t - r * q[:, None]))
    return torch.tensor(loss, dtype=torch.float64), dlogits, W


def _ce_case(B, C, seed, amp=8.0):
    g = torch.Generator().manual_seed(seed)
    logits = amp * (2.0 * torch.rand(B, C, generator=g, dtype=torch.float64) - 1.0)
    return (logits, torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g),
            torch.rand(B, generator=g, dtype=torch.float64), 0.25 + 2.0 * torch.rand(C, generator=g, dtype=torch.float64))


SHAPES = [(1, 1), (1, 3), (5, 2), (33, 7)]


@pytest.mark.parametrize("gamma", [0.5, 2.0, 5.0])
@pytest.mark.parametrize("pair", ["null", "random", "same"])
@pytest.mark.parametrize("option", ["plain", "w+eps"])
@pytest.mark.parametrize("B,C", SHAPES)
def test_model_is_autograd_of_the_definition(B, C, option, pair, gamma):
    """fp64 autograd of loss = sum_b u_b^g row_b / W with u_b summed from its non-negative terms; compared to 1e-9 relative on every
    row where autograd is finite (it gives NaN where u_b == 0 and g < 1: C == 1)."""
    logits, y, y2, lam, w = _ce_case(B, C, 100 * B + C)
    w, eps = (w, 0.1) if option == "w+eps" else (None, 0.0)
    yb, lm = {"null": (None, None), "random": (y2, lam), "same": (y, lam)}[pair]
    loss, dl, W = focal_ce_model(logits, y, yb, lm, w, eps, gamma, dloss=-1.7)
    t, nt = _targets(B, C, y, yb, lm)
    wv = torch.ones(C, dtype=torch.float64) if w is None else w
    lr = logits.clone().requires_grad_(True)
    lp = torch.log_softmax(lr, dim=1)
    a = (1.0 - eps) * wv * t + (eps / C) * wv.expand(B, C)
    ref = (((nt * lp.exp()).sum(1) ** gamma) * (a * -lp).sum(1)).sum() / (t * wv).sum()
    (-1.7 * ref).backward()
    ref = ref.detach()
    assert abs(W - float((t * wv).sum())) <= 1e-12 * W
    assert abs(float(loss) - float(ref)) <= 1e-9 * max(abs(float(ref)), 1.0)
    finite = torch.isfinite(lr.grad).all(1)
    assert bool(finite.all()) or C == 1
    scale = max(float(dl.abs().max()), 1e-300)
    assert float((dl[finite] - lr.grad[finite]).abs().max() if bool(finite.any()) else 0.0) <= 1e-9 * scale
    if C == 1:  # nothing off the target: loss 0 and gradient 0, where autograd has 0 * inf
        assert float(loss) == 0.0 and float(dl.abs().max()) == 0.0


@pytest.mark.parametrize("gamma", [0.5, 2.0, 5.0])
@pytest.mark.parametrize("B,C", SHAPES[1:])
def test_model_is_the_usual_focal_loss_without_options(B, C, gamma):
    logits, y, _, _, _ = _ce_case(B, C, 7 * B + C)
    lr = logits.clone().requires_grad_(True)
    pt = torch.softmax(lr, dim=1)[torch.arange(B), y]
    ref = ((1.0 - pt) ** gamma * torch.nn.functional.cross_entropy(lr, y, reduction="none")).mean()
    ref.backward()
    ref = ref.detach()
    loss, dl, W = focal_ce_model(logits, y, gamma=gamma)
    assert W == B
    assert abs(float(loss) - float(ref)) <= 1e-9 * max(abs(float(ref)), 1.0)
    assert float((dl - lr.grad).abs().max()) <= 1e-9 * max(float(lr.grad.abs().max()), 1.0 / B)


@pytest.mark.parametrize("option", ["plain", "w+eps"])
@pytest.mark.parametrize("B,C", SHAPES)
def test_model_at_gamma_zero_is_the_mixed_label_model(B, C, option):
    logits, y, y2, lam, w = _ce_case(B, C, 3 * B + C)
    w, eps = (w, 0.1) if option == "w+eps" else (None, 0.0)
    for yb, lm in ((y2, lam), (y, lam), (y2, torch.ones(B, dtype=torch.float64))):
        loss, dl, W = focal_ce_model(logits, y, yb, lm, w, eps, 0.0, dloss=-1.7)
        ref, dref, Wr = mixed_ce_model(logits, y, yb, lm, w, eps, dloss=-1.7)
        assert abs(W - Wr) <= 1e-13 * Wr and abs(float(loss) - float(ref)) <= 1e-13 * max(abs(float(ref)), 1.0)
        assert float((dl - dref).abs().max()) <= 1e-13 * max(float(dref.abs().max()), 1.0 / B)
    loss, dl, _ = focal_ce_model(logits, y, None, None, w, eps, 0.0, dloss=-1.7)  # no pair: lam == 1
    ref, dref, _ = mixed_ce_model(logits, y, y, torch.ones(B, dtype=torch.float64), w, eps, dloss=-1.7)
    assert abs(float(loss) - float(ref)) <= 1e-13 * max(abs(float(ref)), 1.0)
    assert float((dl - dref).abs().max()) <= 1e-13 * max(float(dref.abs().max()), 1.0 / B)


def test_model_is_finite_where_the_target_leads_by_far():
    """A target 800 ahead: p underflows in fp64 too, u == 0, and the row gives loss 0 and gradient 0 instead of 0 * inf."""
    logits = torch.tensor([[800.0, 0.0, -3.0], [0.0, 1.0, 2.0]], dtype=torch.float64)
    y = torch.tensor([0, 2])
    for gamma in (0.5, 2.0):
        loss, dl, _ = focal_ce_model(logits, y, None, None, None, 0.1, gamma)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dl).all()) and float(dl[0].abs().max()) == 0.0
        assert float(dl[1].abs().max()) > 0.0


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
    kinds = {_lib.i32: "int", _lib.i64: "int64_t", _lib.f32: "float", _lib.vp: "pointer",
             ctypes.POINTER(_lib.HeadFocalDesc): "pointer"}
    for name in NEW:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/d2r_hip.h"
        assert name in comments, f"{name} has no comment in the header"
        assert hasattr(lib, name), f"{name} declared but not exported"
        res, argtypes = _lib.SIGNATURES[name]
        want = ["pointer" if "*" in a else a.split()[-2] for a in (x.strip() for x in m.group(2).split(","))]
        assert kinds[res] == m.group(1) and [kinds[t] for t in argtypes] == want, (name, want)
    # the arguments of d2r_ce_mix_*, with focal_gamma after label_smoothing
    for way in ("fwd", "bwd"):
        mix, focal = (re.search(r"d2r_ce_" + k + "_" + way + r"\s*\(([^)]*)\)", hdr).group(1) for k in ("mix", "focal"))
        names = lambda s: [re.sub(r"\s+", " ", a).strip().split()[-1].lstrip("*") for a in s.split(",")]
        got, want = names(focal), names(mix)
        i = want.index("label_smoothing")
        assert got == want[:i + 1] + ["focal_gamma"] + want[i + 1:], (got, want)
        mix_t, focal_t = _lib.SIGNATURES["d2r_ce_mix_" + way][1], _lib.SIGNATURES["d2r_ce_focal_" + way][1]
        assert focal_t == mix_t[:i + 1] + [_lib.f32] + mix_t[i + 1:]
    # the formulas are in the header's comment
    for piece in ("u_b^g", "r_b(c)", "focal_gamma == 0 forwards"):
        assert piece in comments, piece
    # the descriptor: the mixed head's, then focal_gamma; the two older descriptors keep their layouts
    body = re.search(r"typedef struct \{([^}]*)\} d2r_head_focal_desc;", hdr).group(1)
    assert re.fullmatch(r"\s*d2r_head_mix_desc mix;\s*float focal_gamma;\s*", body), body
    assert [(n, t) for n, t in _lib.HeadFocalDesc._fields_] == [("mix", _lib.HeadMixDesc), ("focal_gamma", _lib.f32)]
    assert _lib.HeadFocalDesc.mix.offset == 0 and _lib.HeadFocalDesc.focal_gamma.offset == ctypes.sizeof(_lib.HeadMixDesc)
    assert [f[0] for f in _lib.HeadMixDesc._fields_] == ["head", "labels_b", "mix_lam"]
    assert [f[0] for f in _lib.HeadDesc._fields_][-3:] == ["d_pooled", "class_weight", "label_smoothing"]


def test_refusals_need_no_gpu():
    """Bad focal_gamma, bad smoothing and half a pair are refused before any launch: the pointers here are never dereferenced."""
    from d2r_amd import _lib
    from d2r_amd import functional as F
    lib = _lib.load()
    for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert lib.d2r_ce_focal_fwd(1, 1, None, None, None, 0.0, bad, 2, 3, 1, None) != 0
        assert b"d2r_ce_focal_fwd: focal_gamma" in lib.d2r_last_error()
        assert lib.d2r_ce_focal_bwd(1, 1, None, None, None, 0.0, bad, 2, 3, 1, 1, None) != 0
        assert b"d2r_ce_focal_bwd: focal_gamma" in lib.d2r_last_error()
        with pytest.raises(_lib.D2RError, match="focal_gamma"):
            F.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), focal_gamma=bad)
        d = _lib.HeadFocalDesc()
        d.focal_gamma = bad
        assert lib.d2r_head_focal_fwd(ctypes.byref(d), None) != 0 and b"d2r_head_focal_fwd: focal_gamma" in lib.d2r_last_error()
        assert lib.d2r_head_focal_bwd(ctypes.byref(d), None) != 0 and b"d2r_head_focal_bwd: focal_gamma" in lib.d2r_last_error()
    assert lib.d2r_head_focal_fwd(None, None) != 0 and b"null descriptor" in lib.d2r_last_error()
    assert lib.d2r_head_focal_bwd(None, None) != 0 and b"null descriptor" in lib.d2r_last_error()
    for gamma in (0.0, 2.0):  # also when gamma == 0 forwards to d2r_ce_mix_*
        assert lib.d2r_ce_focal_fwd(1, 1, 1, None, None, 0.0, gamma, 2, 3, 1, None) != 0 and b"labels_b and lam" in lib.d2r_last_error()
        assert lib.d2r_ce_focal_bwd(1, 1, None, 1, None, 0.0, gamma, 2, 3, 1, 1, None) != 0 and b"labels_b and lam" in lib.d2r_last_error()
        for eps in (-0.1, 1.0, float("nan")):
            assert lib.d2r_ce_focal_fwd(1, 1, 1, 1, None, eps, gamma, 2, 3, 1, None) != 0 and b"label_smoothing" in lib.d2r_last_error()
            assert lib.d2r_ce_focal_bwd(1, 1, 1, 1, None, eps, gamma, 2, 3, 1, 1, None) != 0 and b"label_smoothing" in lib.d2r_last_error()
    assert lib.d2r_ce_focal_fwd(None, None, None, None, None, 0.0, 2.0, 2, 3, None, None) != 0 and b"bad arguments" in lib.d2r_last_error()
    assert lib.d2r_ce_focal_fwd(1, 1, None, None, None, 0.0, 2.0, 0, 3, 1, None) != 0 and b"bad arguments" in lib.d2r_last_error()


# ------------------------------------------------------------------------------------------------------
# model and command line
# ------------------------------------------------------------------------------------------------------
def _model(**kw):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    return M.UnimoModelF(default_args(**kw), VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32),
                         TextConfig(num_hidden_layers=1))


def test_model_reads_the_option_and_refuses_bad_values():
    plain, focal = _model(), _model(focal_gamma=2.0, label_smoothing=0.1)
    assert plain.focal_gamma == 0.0 and focal.focal_gamma == 2.0 and focal.label_smoothing == 0.1
    assert list(plain.state_dict()) == list(focal.state_dict())
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="focal_gamma"):
            _model(focal_gamma=bad)


def test_cli_flag_parses_and_refuses_bad_values():
    from d2r_amd.run import build_parser
    p = build_parser()
    assert p.parse_args([]).focal_gamma == 0.0
    assert p.parse_args(["--focal_gamma", "2"]).focal_gamma == 2.0 and p.parse_args(["--focal_gamma", "0.5"]).focal_gamma == 0.5
    for bad in ("-0.1", "-1", "nan", "inf", "-inf", "x", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["--focal_gamma", bad])
    a = p.parse_args(["--focal_gamma", "2", "--only_test", "--load_path", "x"])
    assert a.focal_gamma == 2.0 and a.only_test
    a = p.parse_args(["--focal_gamma", "2", "--dp_exact", "--label_smoothing", "0.1", "--class_weights", "balanced", "--aug_mixup", "0.8",
                      "--aug_cutmix", "1.0"])
    assert a.focal_gamma == 2.0 and a.dp_exact and a.aug_mixup == 0.8


def test_run_hands_the_flag_to_the_model_and_logs_it(monkeypatch, tmp_path, caplog):
    """run.main's wiring on synthetic data with the model and the trainer stubbed: the model's args carry focal_gamma, the value is in
    the "cross entropy:" line (which is absent with every loss option off), --dp_exact is allowed and --only_test accepts the flag."""
    from d2r_amd import modules as M, run, train as T
    seen = []
    monkeypatch.setattr(M, "UnimoModelF", lambda **kwargs: seen.append(kwargs["args"]) or object())
    monkeypatch.setattr(T, "MSDTrainer", _StubTrainer)
    monkeypatch.setattr(run, "set_seed", lambda seed: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--device", "cpu", "--seed", "5", "--num_workers", "0", "--train_samples", "8", "--eval_samples", "8", "--batch_size", "4",
            "--image_size", "64", "--patch_size", "32"]

    def main(extra):
        del seen[:], _StubTrainer.made[:], caplog.records[:]
        with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
            run.main(base + extra)
        assert len(seen) == 1 and len(_StubTrainer.made) == 1
        return seen[0], [r.getMessage() for r in caplog.records if r.getMessage().startswith("cross entropy:")]

    args, lines = main([])
    assert args.focal_gamma == 0.0 and lines == []
    args, lines = main(["--focal_gamma", "2"])
    assert args.focal_gamma == 2.0 and lines == ["cross entropy: class weights None, label smoothing 0, focal gamma 2"]
    args, lines = main(["--label_smoothing", "0.1"])
    assert args.focal_gamma == 0.0 and lines == ["cross entropy: class weights None, label smoothing 0.1, focal gamma 0"]
    args, lines = main(["--focal_gamma", "0.5", "--label_smoothing", "0.1", "--class_weights", "1,2,3", "--aug_mixup", "0.8"])
    assert args.focal_gamma == 0.5 and args.class_weights == [1.0, 2.0, 3.0] and "mixer" in _StubTrainer.made[0].kwargs
    assert lines == ["cross entropy: class weights [1.0, 2.0, 3.0], label smoothing 0.1, focal gamma 0.5"]
    args, lines = main(["--focal_gamma", "2", "--dp_exact"])  # W is unchanged, so the global-batch loss still is what --dp_exact promises
    assert args.focal_gamma == 2.0 and args.dp_exact and len(lines) == 1
    args, lines = main(["--focal_gamma", "2", "--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert args.focal_gamma == 2.0 and len(lines) == 1 and lines[0].endswith("(no loss is computed with --only_test: no effect)")
