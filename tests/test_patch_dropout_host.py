"""Host side of PatchDropout (--patch_dropout), no GPU: the K rule, the draw against a restatement of its stated rule, the sampler's
own generator, the CLI flag, the model hook, and the C ABI (the three *_keep entry points declared, listed and exported; the host
checks of the kept positions, which run before any launch and therefore without a device)."""
import ctypes
import logging
import os
import re

import pytest
import torch

from test_augment_host import _StubSplit, _StubTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("d2r_patchify_keep", "d2r_clip_embed_finish_keep", "d2r_clip_embed_bwd_keep")


# ---- the K rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,K", [(49, 0.5, 24), (49, 0.25, 36), (196, 0.75, 49), (10, 0.9, 1), (4, 0.99, 1)])
def test_kept_patches_is_open_clips_rule(n, p, K):
    from d2r_amd.patch_dropout import PatchDropout, kept_patches
    assert kept_patches(n, p) == K == max(1, int(n * (1.0 - p)))
    assert PatchDropout(p, n).K == K


def test_rates_outside_the_half_open_interval_are_refused():
    from d2r_amd.patch_dropout import PatchDropout, kept_patches
    assert kept_patches(49, 0.0) == 49
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            kept_patches(49, bad)
        with pytest.raises(ValueError):
            PatchDropout(bad, 49)
    with pytest.raises(ValueError):
        PatchDropout(0.0, 49)  # off is "no sampler", not a sampler that keeps everything
    with pytest.raises(ValueError):
        kept_patches(0, 0.5)


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def _restated_draw(gen, B, n, K):
    """The rule of the interface, sample by sample: one torch.rand(B, np); sample b keeps argsort(u[b], stable)[:K], ascending."""
    u = torch.rand(B, n, generator=gen)
    rows = []
    for b in range(B):
        order = torch.argsort(u[b], stable=True)[:K]
        rows.append(sorted(int(i) for i in order))
    return rows, u


@pytest.mark.parametrize("B,n,p", [(1, 9, 0.5), (5, 49, 0.5), (3, 196, 0.75), (4, 10, 0.9), (2, 577, 0.25)])
def test_draw_follows_the_stated_rule(B, n, p):
    from d2r_amd.patch_dropout import PatchDropout, patch_dropout_stream_seed
    s = PatchDropout(p, n, seed=7, rank=2)
    gen = torch.Generator().manual_seed(patch_dropout_stream_seed(7, 2))
    for _ in range(3):  # consecutive batches continue one stream, one rand call each
        keep = s.draw(B)
        want, u = _restated_draw(gen, B, n, s.K)
        assert keep.dtype == torch.int32 and tuple(keep.shape) == (B, s.K) and keep.is_contiguous() and keep.device.type == "cpu"
        assert keep.tolist() == want
        for b in range(B):
            row = keep[b].tolist()
            assert all(0 <= i < n for i in row) and all(a < c for a, c in zip(row, row[1:])) and len(row) == s.K
            kept = torch.zeros(n, dtype=torch.bool)
            kept[keep[b].long()] = True
            if s.K < n:  # the K smallest values of u[b]
                assert float(u[b][kept].max()) <= float(u[b][~kept].min())
    assert torch.equal(s.generator.get_state(), gen.get_state()), "a draw consumed more than its one torch.rand(B, np)"


def test_samples_of_a_batch_are_drawn_independently():
    from d2r_amd.patch_dropout import PatchDropout
    keep = PatchDropout(0.5, 49, seed=1).draw(16)
    assert len({tuple(r) for r in keep.tolist()}) == 16


def test_sampler_has_a_generator_of_its_own():
    from d2r_amd import functional as F
    from d2r_amd.augment import stream_seed
    from d2r_amd.mix import mix_stream_seed
    from d2r_amd.patch_dropout import PatchDropout, patch_dropout_stream_seed
    from d2r_amd.text_augment import text_stream_seed
    torch.manual_seed(123)
    state = torch.get_rng_state()
    draws = {pair: PatchDropout(0.5, 49, *pair).draw(4) for pair in ((1, 0), (1, 1), (2, 0))}
    assert torch.equal(torch.get_rng_state(), state), "building a sampler or drawing moved torch's default generator"
    assert torch.equal(draws[(1, 0)], PatchDropout(0.5, 49, 1, 0).draw(4)), "the same (seed, rank) must give the same stream"
    assert not torch.equal(draws[(1, 0)], draws[(1, 1)]), "two ranks drew the same patches"
    assert not torch.equal(draws[(1, 0)], draws[(2, 0)])
    for pair in draws:  # a stream-seed function distinct from the existing ones
        others = {stream_seed(*pair), mix_stream_seed(*pair), text_stream_seed(*pair), F.drop_path_stream_seed(*pair)}
        assert patch_dropout_stream_seed(*pair) not in others
    assert len({patch_dropout_stream_seed(s, r) for s in range(4) for r in range(4)}) == 16
    assert patch_dropout_stream_seed(1 + 2 ** 32, 3) == patch_dropout_stream_seed(1, 3)  # seed mod 2^32, as the other streams
    with pytest.raises(ValueError):
        patch_dropout_stream_seed(1, 1 << 24)
    h, d = PatchDropout(0.5, 49, 1, 0).sample(4, "cpu")
    assert torch.equal(h, draws[(1, 0)]) and torch.equal(d, h)


def test_describe_names_the_numbers():
    from d2r_amd.patch_dropout import PatchDropout
    text = PatchDropout(0.75, 196).describe()
    assert "P = 0.75" in text and "K = 49" in text and "np = 196" in text and "50 image tokens" in text


# ---- model hook --------------------------------------------------------------------------------------------------------------
def test_set_patch_dropout_installs_and_clears_the_sampler():
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.patch_dropout import PatchDropout
    assert default_args().patch_dropout == 0
    tc = TextConfig(num_hidden_layers=1, hidden_size=768, vocab_size=64, max_position_embeddings=16)
    vc = VisionConfig(num_hidden_layers=1, image_size=96, patch_size=32)
    model = M.UnimoModel(default_args(DR_step=3), vc, tc)
    emb = model.vision_embeddings
    assert emb.patch_dropout is None
    torch.manual_seed(5)
    state = torch.get_rng_state()
    s = model.set_patch_dropout(0.5, seed=3, rank=1)
    assert isinstance(s, PatchDropout) and emb.patch_dropout is s and (s.num_patches, s.K) == (9, 4)
    assert torch.equal(s.draw(2), PatchDropout(0.5, 9, 3, 1).draw(2))
    assert model.set_patch_dropout(0.0) is None and emb.patch_dropout is None
    assert torch.equal(torch.get_rng_state(), state)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            model.set_patch_dropout(bad)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_flag_is_parsed_and_checked(capsys):
    from d2r_amd.run import build_parser
    assert build_parser().parse_args([]).patch_dropout == 0.0
    assert build_parser().parse_args(["--patch_dropout", "0.5"]).patch_dropout == 0.5
    for bad in ("-0.1", "1", "nan", "inf"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--patch_dropout", bad])
        assert "--patch_dropout" in capsys.readouterr().err


def test_run_passes_the_flag_on_and_ignores_it_with_only_test(monkeypatch, tmp_path, caplog):
    from d2r_amd import data as D, modules as M, run, train as T
    for name in ("train.json", "dev.json", "test.json"):
        (tmp_path / name).write_text("[]")
    monkeypatch.setattr(D, "MSDDataset", _StubSplit)
    monkeypatch.setattr(M, "UnimoModelF", lambda **kwargs: object())
    monkeypatch.setattr(T, "MSDTrainer", _StubTrainer)
    monkeypatch.setattr(run, "set_seed", lambda seed: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--data_path", str(tmp_path), "--img_path", str(tmp_path), "--bert_name", str(tmp_path), "--device", "cpu", "--num_workers", "0"]

    def main(extra):
        del _StubTrainer.made[:]
        run.main(base + extra)
        assert len(_StubTrainer.made) == 1
        return _StubTrainer.made[0].kwargs["args"]

    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        assert main(["--patch_dropout", "0.5"]).patch_dropout == 0.5
        assert main([]).patch_dropout == 0.0
    assert not any("--patch_dropout is ignored" in r.getMessage() for r in caplog.records)
    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        args = main(["--patch_dropout", "0.5", "--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert args.patch_dropout == 0.0
    assert sum("--patch_dropout is ignored with --only_test" in r.getMessage() for r in caplog.records) == 1


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_listed_and_exported():
    from d2r_amd import _lib
    text = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    assert "K25" in text
    kinds = {"int": _lib.i32, "void*": _lib.vp, "float*": _lib.vp, "int32_t*": _lib.vp}
    counts = {"d2r_patchify_keep": 11, "d2r_clip_embed_finish_keep": 11, "d2r_clip_embed_bwd_keep": 11}
    for name in NAMES:
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/d2r_hip.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        types = [a.replace("const ", "").rsplit(" ", 1)[0] for a in args]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib.i32 and len(argtypes) == len(args) == counts[name]
        assert argtypes == [kinds[t] for t in types], (name, types)
        assert hasattr(_lib.load(), name)
    for name in NAMES:  # host copy and device copy of the kept positions stand next to each other
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert re.search(r"const int32_t\* h_keep,\s*const int32_t\* keep,", m.group(1))


def _keep(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def test_kept_positions_are_checked_on_the_host_before_any_launch():
    """Every call below is refused on the host copy (nothing is dereferenced on the device side: the addresses are host memory that
    no kernel ever sees), and the message names the entry point."""
    from d2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    B, n, D = 2, 4, 8  # a 2 x 2 grid of 4 x 4 patches

    def calls(h, K, dtype=0, hk="given"):
        hp = ctypes.addressof(h) if hk == "given" else None
        return {"d2r_patchify_keep": lambda: lib.d2r_patchify_keep(dtype, a, B, 8, 8, 4, hp, a, K, a, None),
                "d2r_clip_embed_finish_keep": lambda: lib.d2r_clip_embed_finish_keep(dtype, a, a, a, hp, a, B, K, n, D, None),
                "d2r_clip_embed_bwd_keep": lambda: lib.d2r_clip_embed_bwd_keep(dtype, a, hp, a, B, K, n, D, a, a, None)}

    bad_sets = {"an index == np": ([[0, 4], [0, 1]], 2), "a negative index": ([[-1, 2], [0, 1]], 2),
                "a repeated index": ([[0, 1], [2, 2]], 2), "a descending pair": ([[0, 1], [3, 2]], 2),
                "K = 0": ([[0], [0]], 0), "K = np + 1": ([[0, 1, 2, 3, 3], [0, 1, 2, 3, 3]], 5)}
    for what, (rows, K) in bad_sets.items():
        for name, fn in calls(_keep(rows), K).items():
            assert fn() == -1, (what, name)
            assert name.encode() in lib.d2r_last_error(), (what, name, lib.d2r_last_error())
    good = _keep([[0, 2], [1, 3]])
    for name, fn in calls(good, 2, dtype=3).items():
        assert fn() == -1 and name.encode() in lib.d2r_last_error(), name
    for name, fn in calls(good, 2, hk=None).items():
        assert fn() == -1 and name.encode() in lib.d2r_last_error(), name
    assert lib.d2r_patchify_keep(0, None, B, 8, 8, 4, ctypes.addressof(good), a, 2, a, None) == -1
    assert lib.d2r_patchify_keep(0, a, B, 8, 8, 3, ctypes.addressof(good), a, 2, a, None) == -1  # H % p
    assert lib.d2r_clip_embed_finish_keep(0, a, None, a, ctypes.addressof(good), a, B, 2, n, D, None) == -1
    assert lib.d2r_clip_embed_bwd_keep(0, a, ctypes.addressof(good), a, B, 2, n, D, None, a, None) == -1
    assert lib.d2r_clip_embed_bwd_keep(0, a, ctypes.addressof(good), a, 0, 2, n, D, a, a, None) == -1  # B < 1
