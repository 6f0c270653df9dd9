"""Host side of stochastic depth (--drop_path), no GPU: the per-layer schedule, the CLI flag, DropPath's own seed generator, and the
C ABI (d2r_drop_path declared, listed and exported; the encoder-layer descriptor grown at its end only; refusals before any launch)."""
import ctypes
import logging
import os
import re

import pytest
import torch

from test_augment_host import _StubSplit, _StubTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- schedule ----------------------------------------------------------------------------------------------------------------
def test_schedule_grows_linearly_with_depth():
    from d2r_amd.modules import drop_path_schedule
    r = drop_path_schedule(0.1, 12)
    assert len(r) == 12 and r[0] == 0.0 and r[-1] == pytest.approx(0.1, abs=1e-15)
    assert all(b - a == pytest.approx(0.1 / 11, abs=1e-15) for a, b in zip(r, r[1:]))
    assert drop_path_schedule(0.1, 1) == [0.0]
    assert drop_path_schedule(0.0, 12) == [0.0] * 12 and drop_path_schedule(0.3, 0) == []
    assert drop_path_schedule(0.2, 2) == [0.0, 0.2]
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            drop_path_schedule(bad, 12)


def test_set_drop_path_touches_the_two_towers_only():
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    assert default_args().drop_path == 0.0
    tc = TextConfig(num_hidden_layers=3, hidden_size=768, vocab_size=64, max_position_embeddings=16)
    vc = VisionConfig(num_hidden_layers=3, image_size=64, patch_size=32)
    model = M.UnimoModel(default_args(DR_step=3), vc, tc)
    layers = [m for m in model.modules() if isinstance(m, (M.BertLayer, M.CLIPEncoderLayer))]
    assert len(layers) == 8 and all(l.p_path == 0.0 for l in layers)
    rates = model.set_drop_path(0.2)
    assert rates == ([0.0, 0.1, 0.2], [0.0, 0.1, 0.2])
    assert [l.p_path for l in model.encoder.text_layer] == [0.0, 0.1, 0.2]
    assert [l.p_path for l in model.encoder.vision_layers] == [0.0, 0.1, 0.2]
    assert all(l.p_path == 0.0 for l in list(model.self_text) + list(model.self_vision))
    model.set_drop_path(0.0)
    assert all(l.p_path == 0.0 for l in layers)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_flag_is_parsed_and_checked(capsys):
    from d2r_amd.run import build_parser
    assert build_parser().parse_args([]).drop_path == 0.0
    assert build_parser().parse_args(["--drop_path", "0.2"]).drop_path == 0.2
    for bad in ("-0.1", "1.0", "nan"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--drop_path", bad])
        assert "--drop_path" in capsys.readouterr().err


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
        assert main(["--drop_path", "0.2"]).drop_path == 0.2
        assert main([]).drop_path == 0.0
    assert not any("--drop_path is ignored" in r.getMessage() for r in caplog.records)
    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        args = main(["--drop_path", "0.2", "--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert args.drop_path == 0.0
    assert sum("--drop_path is ignored with --only_test" in r.getMessage() for r in caplog.records) == 1


# ---- generator ---------------------------------------------------------------------------------------------------------------
def _draws(F, seed, rank, n=4):
    F.seed_drop_path(seed, rank)
    return [F._next_drop_path_seed() for _ in range(n)]


def test_seeds_come_from_a_generator_of_their_own(monkeypatch):
    from d2r_amd import functional as F
    from d2r_amd.augment import stream_seed
    monkeypatch.setattr(F, "_drop_path_generator", None)  # restored afterwards: other tests keep their stream
    torch.manual_seed(123)
    state = torch.get_rng_state()
    lazy = [F._next_drop_path_seed() for _ in range(4)]  # never seeded: from torch.initial_seed() and rank 0
    assert torch.equal(torch.get_rng_state(), state), "drawing DropPath seeds moved torch's default generator"
    assert lazy == _draws(F, 123, 0) and all(0 <= s < 2 ** 63 for s in lazy)
    streams = {pair: tuple(_draws(F, *pair)) for pair in ((1, 0), (1, 1), (2, 0))}
    assert torch.equal(torch.get_rng_state(), state), "seeding DropPath moved torch's default generator"
    assert len(set(streams.values())) == 3
    assert all(len(set(s)) == len(s) for s in streams.values())
    assert streams[(1, 0)] == tuple(_draws(F, 1, 0)), "the same (seed, rank) must give the same stream"
    for pair, s in streams.items():  # the augmenter's stream for the same pair is another one
        assert F.drop_path_stream_seed(*pair) != stream_seed(*pair)
        g = torch.Generator().manual_seed(stream_seed(*pair))
        assert tuple(int(torch.empty((), dtype=torch.int64).random_(generator=g).item()) for _ in s) != s
    assert F.drop_path_stream_seed(1 + 2 ** 32, 3) == F.drop_path_stream_seed(1, 3)  # seed mod 2^32, as the augmenter's
    with pytest.raises(ValueError):
        F.seed_drop_path(1, 1 << 24)


def test_eval_mode_and_rate_zero_draw_nothing(monkeypatch):
    from d2r_amd import functional as F
    monkeypatch.setattr(F, "_next_drop_path_seed", lambda: pytest.fail("a DropPath seed was drawn"))
    x = torch.ones(2, 3)
    assert F.drop_path(x, 0.5, False) is x and F.drop_path(x, 0.0, True) is x
    with pytest.raises(ValueError):
        F.drop_path(x, 1.0, True)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
_OLD_FIELDS = (["dtype", "pre_ln", "act", "B", "L", "E", "H", "F", "eps", "scale", "mask", "w_qkv", "w_o", "w_1", "w_2", "b_qkv", "b_o", "b_1",
                "b_2", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "gw_qkv", "gw_o", "gw_1", "gw_2", "gb_qkv", "gb_o", "gb_1", "gb_2", "gln1_g",
                "gln1_b", "gln2_g", "gln2_b", "x", "y", "qkv", "ctx", "h1", "n1", "f_pre", "f", "h2", "lse", "mean1", "rstd1", "mean2",
                "rstd2", "dy", "dx", "scratch", "scratch_bytes", "splitk_ws", "splitk_bytes", "wgrad_stream", "defer_wgrad", "o_dy",
                "defer_ln", "o_lnws", "p_attn", "p_hidden", "seed_attn", "seed_hidden"])
# offsets of the descriptor before p_path / seed_path were appended (LP64: 8 ints, 2 floats, 41 pointers, ...)
_OLD_OFFSETS = dict(dtype=0, pre_ln=4, act=8, B=12, L=16, E=20, H=24, F=28, eps=32, scale=36, mask=40, w_qkv=48, scratch=368,
                    scratch_bytes=376, splitk_ws=384, splitk_bytes=392, wgrad_stream=400, defer_wgrad=408, o_dy=416, defer_ln=448,
                    o_lnws=456, p_attn=472, p_hidden=476, seed_attn=480, seed_hidden=488)


def test_drop_path_is_declared_listed_and_exported():
    from d2r_amd import _lib
    header = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    assert re.search(r"\bint d2r_drop_path\(int dtype, const void\* x, const void\* add, void\* y, int64_t B, int64_t per_sample,\s*"
                     r"float p_path,\s*uint64_t seed_path, float p_elem, uint64_t seed_elem, void\* stream\);", header)
    res, argtypes = _lib.SIGNATURES["d2r_drop_path"]
    assert res is ctypes.c_int and argtypes == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_float, ctypes.c_uint64,
                                                ctypes.c_void_p]
    assert hasattr(_lib.load(), "d2r_drop_path")


def test_descriptor_grew_at_its_end_only():
    from d2r_amd._lib import EncoderLayerDesc as D
    names = [f[0] for f in D._fields_]
    assert names == _OLD_FIELDS + ["p_path", "seed_path"]
    for name, off in _OLD_OFFSETS.items():
        assert getattr(D, name).offset == off, name
    pointers = _OLD_FIELDS[_OLD_FIELDS.index("mask"):_OLD_FIELDS.index("scratch") + 1]
    assert [getattr(D, n).offset for n in pointers] == list(range(40, 40 + 8 * len(pointers), 8))
    assert D.p_path.offset == 504 and D.p_path.size == 4 and D.seed_path.offset == 512 and D.seed_path.size == 16
    assert ctypes.sizeof(D) == 528
    d = D()
    assert d.p_path == 0.0 and list(d.seed_path) == [0, 0]  # a zero-initialised tail means off
    header = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    tail = header[header.index("uint64_t seed_attn, seed_hidden[2];"):header.index("} d2r_encoder_layer_desc;")]
    assert re.search(r"float p_path;\s*uint64_t seed_path\[2\];\s*$", tail)


def _f(x):
    return ctypes.c_float(x)


def test_drop_path_checks_its_arguments_before_any_launch():
    from d2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16  # never dereferenced: every call below is refused or a no-op

    def call(x=a, y=a, B=2, n=8, p_path=0.5, p_elem=0.1, dtype=0):
        return lib.d2r_drop_path(dtype, x, None, y, B, n, _f(p_path), 1, _f(p_elem), 2, None)

    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert call(p_path=bad) == -1 and b"d2r_drop_path" in lib.d2r_last_error() and b"[0, 1)" in lib.d2r_last_error()
        assert call(p_elem=bad) == -1
    assert call(x=None) == -1 and call(y=None) == -1 and b"d2r_drop_path" in lib.d2r_last_error()
    assert call(B=-1) == -1 and call(n=-1) == -1 and call(dtype=3) == -1
    assert call(B=1 << 40, n=1 << 40) == -1 and b"overflows" in lib.d2r_last_error()
    assert call(B=0) == 0 and call(n=0) == 0  # nothing to do, nothing launched


def test_encoder_layer_refuses_a_bad_p_path():
    from d2r_amd import _lib
    lib = _lib.load()
    for fn in (lib.d2r_encoder_layer_fwd, lib.d2r_encoder_layer_bwd):
        for bad in (-0.1, 1.0, float("nan")):
            d = _lib.EncoderLayerDesc()
            d.dtype, d.act, d.B, d.L, d.E, d.H, d.F, d.p_path = _lib.BF16, _lib.ACT_GELU, 2, 37, 768, 12, 3072, bad
            assert fn(ctypes.byref(d), None) == -1 and b"p_path" in lib.d2r_last_error(), bad
        d.p_path = 0.5  # a good value gets past that check: the next complaint is about the null parameters
        assert fn(ctypes.byref(d), None) == -1 and b"null parameter" in lib.d2r_last_error()
