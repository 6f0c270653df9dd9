"""MixUp / CutMix on the host (no GPU): the draws of d2r_amd.mix.Mixer, the command-line flags and run.main's wiring, and the fp64
model of the mixed-label cross entropy that the GPU tests (test_gpu_mix.py) compare the kernels with."""
import logging

import pytest
import torch


# ------------------------------------------------------------------------------------------------------
# the fp64 model of d2r_ce_mix_fwd / d2r_ce_mix_bwd (imported by test_gpu_mix.py)
# ------------------------------------------------------------------------------------------------------
def mixed_ce_model(logits, labels, labels_b, lam, weight=None, eps=0.0, dloss=1.0):
    """(loss, dlogits, W) in fp64 from the formulas of include/d2r_hip.h, written out term by term (no autograd):
        hard_b(c) = (1-e) (lam w[y] [c == y] + (1-lam) w[y2] [c == y2]),  W = sum_b (lam w[y] + (1-lam) w[y2]),
        loss = sum_b [sum_c hard_b(c) (-lp[b,c]) + (e/C) sum_c w[c] (-lp[b,c])] / W,
        dlogits[b,c] = dloss / W (p[b,c] (sum_k hard_b(k) + (e/C) sum_k w[k]) - hard_b(c) - (e/C) w[c])."""
    x = logits.detach().double().cpu()
    B, C = x.shape
    y, y2, lam = labels.cpu().view(-1).long(), labels_b.cpu().view(-1).long(), lam.detach().cpu().view(-1).double()
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().double().cpu()
    lp = x - torch.logsumexp(x, dim=1, keepdim=True)
    p = lp.exp()
    rows = torch.arange(B)
    hard = torch.zeros(B, C, dtype=torch.float64)
    hard[rows, y] += (1.0 - eps) * lam * w[y]
    hard[rows, y2] += (1.0 - eps) * (1.0 - lam) * w[y2]  # (+=: y2 == y puts both shares on one class)
    soft = (eps / C) * w.expand(B, C)
    W = float((lam * w[y] + (1.0 - lam) * w[y2]).sum())
    loss = float(((hard + soft) * -lp).sum()) / W
    dlogits = dloss / W * (p * (hard + soft).sum(1, keepdim=True) - hard - soft)
    return torch.tensor(loss, dtype=torch.float64), dlogits, W


def _ce_case(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    logits = 8.0 * (2.0 * torch.rand(B, C, generator=g, dtype=torch.float64) - 1.0)
    return (logits, torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g),
            torch.rand(B, generator=g, dtype=torch.float64), 0.25 + 2.0 * torch.rand(C, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", [(1, 1), (1, 3), (5, 2), (33, 7)])
def test_model_is_torchs_cross_entropy_on_probability_targets(B, C, eps):
    logits, y, y2, lam, _ = _ce_case(B, C, 10 * B + C)
    target = lam[:, None] * torch.nn.functional.one_hot(y, C).double() + (1 - lam)[:, None] * torch.nn.functional.one_hot(y2, C).double()
    lr = logits.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, target, label_smoothing=eps)
    (-1.7 * ref).backward()
    ref = ref.detach()
    loss, dl, W = mixed_ce_model(logits, y, y2, lam, None, eps, dloss=-1.7)
    assert abs(W - B) < 1e-12 * B
    assert abs(float(loss) - float(ref)) <= 1e-13 * max(abs(float(ref)), 1.0)
    assert float((dl - lr.grad).abs().max()) <= 1e-14


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", [(1, 1), (1, 3), (5, 2), (33, 7)])
def test_model_is_torchs_cross_entropy_on_index_targets_at_lam_one(B, C, eps, weighted):
    logits, y, y2, _, w = _ce_case(B, C, 10 * B + C + 1)
    w = w if weighted else None
    lr = logits.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, y, weight=w, label_smoothing=eps)
    (-1.7 * ref).backward()
    ref = ref.detach()
    loss, dl, W = mixed_ce_model(logits, y, y2, torch.ones(B), w, eps, dloss=-1.7)
    assert abs(float(loss) - float(ref)) <= 1e-13 * max(abs(float(ref)), 1.0)
    assert float((dl - lr.grad).abs().max()) <= 1e-13 * (1.0 if w is None else float(w.max())) / W * B


# ------------------------------------------------------------------------------------------------------
# Mixer.draw
# ------------------------------------------------------------------------------------------------------
def _mixer(S=224, mixup=0.8, cutmix=1.0, prob=1.0, seed=7, rank=0):
    from d2r_amd.mix import Mixer
    return Mixer(S, mixup, cutmix, prob, seed=seed, rank=rank)


def _a(desc):
    return desc[:, 1].contiguous().view(torch.float32)


def test_draw_is_reproducible_and_differs_between_ranks_and_seeds():
    from d2r_amd.augment import photo_stream_seed, stream_seed
    from d2r_amd.mix import mix_stream_seed
    d0, l0 = _mixer().draw(16)
    d1, l1 = _mixer().draw(16)
    assert torch.equal(d0, d1) and torch.equal(l0, l1)
    assert d0.dtype == torch.int32 and tuple(d0.shape) == (16, 8) and l0.dtype == torch.float32 and tuple(l0.shape) == (16,)
    d2, l2 = _mixer(rank=1).draw(16)
    d3, l3 = _mixer(seed=8).draw(16)
    assert not torch.equal(d0, d2) and not torch.equal(l0, l2) and not torch.equal(d0, d3) and not torch.equal(d2, d3)
    m = _mixer()
    first, second = m.draw(16), m.draw(16)
    assert not torch.equal(first[0], second[0])  # the stream moves on
    assert m.generator.initial_seed() == mix_stream_seed(7, 0)
    seeds = {f(s, r) for f in (mix_stream_seed, stream_seed, photo_stream_seed) for s in (0, 7) for r in (0, 1)}
    assert len(seeds) == 12  # a stream of its own for every (construction, seed, rank)
    assert mix_stream_seed(2 ** 32 + 7, 3) == mix_stream_seed(7, 3) and 0 <= mix_stream_seed(2 ** 32 - 1, 2 ** 24 - 1) < 2 ** 64
    with pytest.raises(ValueError):
        mix_stream_seed(0, 1 << 24)


def test_draw_leaves_the_default_generator_and_the_augmenters_alone():
    from d2r_amd.augment import Augmenter
    aug = Augmenter(224, 0.5, 0.5, seed=7, rank=0, brightness=0.4)
    torch.manual_seed(123)
    before = torch.get_rng_state().clone(), aug.generator.get_state().clone(), aug.photo_generator.get_state().clone()
    m = _mixer()
    m.draw(32)
    m.draw(5)
    assert torch.equal(before[0], torch.get_rng_state())
    assert torch.equal(before[1], aug.generator.get_state()) and torch.equal(before[2], aug.photo_generator.get_state())


def test_draw_consumes_the_same_stream_whatever_the_settings():
    states = []
    for mixup, cutmix, prob in ((0.8, 1.0, 1.0), (0.8, 0.0, 1.0), (0.0, 1.0, 0.3), (0.0, 0.0, 1.0), (0.2, 5.0, 0.0)):
        m = _mixer(mixup=mixup, cutmix=cutmix, prob=prob)
        m.draw(16)
        m.draw(3)
        states.append((m.generator.get_state(), m.batches))
    assert all(torch.equal(states[0][0], s) and n == 2 for s, n in states)
    # the gamma generator is seeded anew for every batch: what a batch draws does not depend on what earlier batches consumed
    a, b = _mixer(mixup=0.8), _mixer(mixup=0.8)
    a.draw(16), b.draw(999)
    a.gamma_generator.manual_seed(1)
    a.draw(4), b.draw(4)
    assert torch.equal(a.last_lam0, b.last_lam0)
    # ... and the partner permutation (u0) is the same one under every setting that mixes every sample
    assert torch.equal(_mixer(mixup=0.8, cutmix=0.0).draw(16)[0][:, 0], _mixer(mixup=0.0, cutmix=2.0).draw(16)[0][:, 0])


@pytest.mark.parametrize("B", [1, 2, 16, 257])
def test_partners_are_a_permutation(B):
    desc, _ = _mixer().draw(B)
    assert sorted(desc[:, 0].tolist()) == list(range(B))
    assert bool((desc[:, 6:] == 0).all())


def test_prob_zero_and_alphas_zero_give_identity_descriptors():
    for m in (_mixer(prob=0.0), _mixer(mixup=0.0, cutmix=0.0)):
        desc, lam = m.draw(16)
        assert desc[:, 0].tolist() == list(range(16))
        assert bool((_a(desc) == 1.0).all()) and bool((desc[:, 2:] == 0).all()) and bool((lam == 1.0).all())
    desc, lam = _mixer(prob=0.5).draw(400)  # in between: both kinds occur, and an unmixed sample is the identity
    off = lam == 1.0
    assert 100 < int(off.sum()) < 300
    assert desc[off, 0].tolist() == torch.arange(400)[off].tolist() and bool((desc[off][:, 2:] == 0).all())


def test_mixup_alone_has_empty_boxes_and_a_equal_to_lam():
    desc, lam = _mixer(mixup=0.8, cutmix=0.0).draw(500)
    assert bool((desc[:, 2:6] == 0).all())
    assert torch.equal(_a(desc), lam) and bool((lam >= 0).all()) and bool((lam <= 1).all())
    assert float(lam.min()) < 0.1 and float(lam.max()) > 0.9 and 0.4 < float(lam.mean()) < 0.6


@pytest.mark.parametrize("S", [1, 7, 224])
def test_cutmix_alone_has_a_one_boxes_inside_the_image_and_the_exact_share(S):
    desc, lam = _mixer(S=S, mixup=0.0, cutmix=1.0).draw(500)
    x0, y0, w, h = (desc[:, k].long() for k in (2, 3, 4, 5))
    assert bool((_a(desc) == 1.0).all())
    assert bool((x0 >= 0).all()) and bool((y0 >= 0).all()) and bool((w >= 0).all()) and bool((h >= 0).all())
    assert bool((x0 + w <= S).all()) and bool((y0 + h <= S).all())
    want = (1.0 - (w * h).double() / float(S * S)).to(torch.float32)
    assert torch.equal(lam, want)
    if S == 224:
        assert int((w * h > 0).sum()) > 400 and int(((w < S) & (w > 0)).sum()) > 300  # real boxes, most of them clipped or partial


def test_both_on_mixes_either_way_per_sample():
    desc, lam = _mixer().draw(400)
    cut = desc[:, 4] * desc[:, 5] > 0
    blend = _a(desc) != 1.0
    assert not bool((cut & blend).any())
    assert 120 < int(cut.sum()) < 280 and 120 < int(blend.sum()) < 280
    assert torch.equal(lam[blend], _a(desc)[blend])


def test_beta_mean_at_alpha_one():
    """20,000 draws of Beta(1, 1) = U(0, 1): sigma of the mean = sqrt(1/12 / 20000) ~ 0.002; the bound is 0.02."""
    m = _mixer(mixup=1.0, cutmix=1.0, seed=11)
    m.draw(20000)
    lam0 = m.last_lam0
    assert tuple(lam0.shape) == (20000, 2) and bool((lam0 >= 0).all()) and bool((lam0 <= 1).all())
    for k in (0, 1):
        assert abs(float(lam0[:, k].mean()) - 0.5) < 0.02, float(lam0[:, k].mean())
        assert abs(float(lam0[:, k].var()) - 1.0 / 12.0) < 0.005
    m = _mixer(mixup=0.4, cutmix=1.0, seed=11)  # Beta(0.4, 0.4): mean 0.5, variance 1 / (4 (2 * 0.4 + 1)) = 0.1389
    m.draw(20000)
    assert abs(float(m.last_lam0[:, 0].mean()) - 0.5) < 0.02 and abs(float(m.last_lam0[:, 0].var()) - 0.25 / 1.8) < 0.01


def test_mixer_refuses_bad_settings_and_describes_itself():
    from d2r_amd.mix import Mixer
    for bad in (dict(S=0), dict(S=4097), dict(S=224.0), dict(mixup_alpha=-0.1), dict(cutmix_alpha=float("inf")),
                dict(mixup_alpha=float("nan")), dict(prob=-0.1), dict(prob=1.1), dict(rank=1 << 24)):
        with pytest.raises(ValueError):
            Mixer(**{"S": 224, **bad})
    text = _mixer().describe()
    assert "MixUp" in text and "CutMix" in text and "Beta(0.8, 0.8)" in text and "only the image is mixed" in text
    assert "CutMix" not in _mixer(cutmix=0.0).describe().split("only the image")[0]


# ------------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------------
def test_cli_types_refuse_bad_values():
    from d2r_amd.run import build_parser, main
    p = build_parser()
    a = p.parse_args([])
    assert a.aug_mixup == 0.0 and a.aug_cutmix == 0.0 and a.aug_mix_prob is None
    a = p.parse_args(["--aug_mixup", "0.8", "--aug_cutmix", "1.0", "--aug_mix_prob", "0.5"])
    assert (a.aug_mixup, a.aug_cutmix, a.aug_mix_prob) == (0.8, 1.0, 0.5)
    for flag, bads in (("--aug_mixup", ("-0.1", "inf", "nan", "x")), ("--aug_cutmix", ("-1", "inf", "nan")),
                       ("--aug_mix_prob", ("-0.1", "1.1", "nan"))):
        for bad in bads:
            with pytest.raises(SystemExit):
                p.parse_args([flag, bad])
    for argv in (["--aug_mix_prob", "0.5"], ["--aug_mix_prob", "1"], ["--aug_mix_prob", "0.5", "--aug_mixup", "0"]):
        with pytest.raises(SystemExit, match="--aug_mix_prob"):
            main(argv)


class _StubTrainer:
    made = []

    def __init__(self, **kwargs):
        self.kwargs, self.samples_per_sec = kwargs, None
        _StubTrainer.made.append(self)

    def train(self, clip_sd, bert_sd):
        pass

    def _load_checkpoint(self, path):
        pass

    def predict(self, loader, path):
        pass


def test_run_builds_a_mixer_only_when_a_flag_is_on(monkeypatch, tmp_path, caplog):
    """run.main's wiring on synthetic data with the model and the trainer stubbed: flags off, no `mixer` keyword at all; a flag on,
    the trainer gets a Mixer with the flags' values and the (seed, rank) stream; --only_test builds none and says so."""
    from d2r_amd import modules as M, run, train as T
    from d2r_amd.mix import Mixer, mix_stream_seed
    monkeypatch.setattr(M, "UnimoModelF", lambda **kwargs: object())
    monkeypatch.setattr(T, "MSDTrainer", _StubTrainer)
    monkeypatch.setattr(run, "set_seed", lambda seed: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--device", "cpu", "--seed", "5", "--num_workers", "0", "--train_samples", "8", "--eval_samples", "8", "--batch_size", "4",
            "--image_size", "64", "--patch_size", "32"]

    def main(extra):
        del _StubTrainer.made[:]
        run.main(base + extra)
        assert len(_StubTrainer.made) == 1
        return _StubTrainer.made[0].kwargs

    assert "mixer" not in main([])
    m = main(["--aug_mixup", "0.8", "--aug_cutmix", "1.0"])["mixer"]
    assert isinstance(m, Mixer) and (m.S, m.mixup_alpha, m.cutmix_alpha, m.prob) == (64, 0.8, 1.0, 1.0)
    assert m.generator.initial_seed() == mix_stream_seed(5, 0)
    m = main(["--aug_cutmix", "0.5", "--aug_mix_prob", "0.25"])["mixer"]
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob) == (0.0, 0.5, 0.25)
    m = main(["--aug_mixup", "0.2"])["mixer"]
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob) == (0.2, 0.0, 1.0)
    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        kwargs = main(["--aug_mixup", "0.8", "--aug_cutmix", "1.0", "--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert "mixer" not in kwargs
    assert sum("--aug_mixup / --aug_cutmix / --aug_mix_prob are ignored with --only_test" in r.getMessage() for r in caplog.records) == 1


def test_functional_refuses_half_a_pair_without_a_gpu():
    """labels_b without lam (or the reverse) never reaches the library; the library's own refusal needs no launch either."""
    from d2r_amd import _lib
    from d2r_amd import functional as F
    logits, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    for kw in (dict(labels_b=y), dict(lam=torch.ones(2))):
        with pytest.raises(_lib.D2RError, match="go together"):
            F.cross_entropy(logits, y, **kw)
    lib = _lib.load()
    assert lib.d2r_ce_mix_fwd(1, 1, 1, None, None, 0.0, 2, 3, 1, None) != 0 and b"labels_b and lam" in lib.d2r_last_error()
    assert lib.d2r_ce_mix_bwd(1, 1, None, 1, None, 0.0, 2, 3, 1, 1, None) != 0 and b"labels_b and lam" in lib.d2r_last_error()
    assert lib.d2r_ce_mix_fwd(1, 1, 1, 1, None, 1.0, 2, 3, 1, None) != 0 and b"label_smoothing" in lib.d2r_last_error()
