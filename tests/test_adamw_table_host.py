"""CPU: the host side of per-parameter AdamW hyper-parameters (FusedAdamW(layer_lr_decay=..., decay_exempt_1d=...)) - the layer
scale of every live parameter name, the segment table built from (fake) store entries, the argument checks of the three C entry
points (all before anything is enqueued: no GPU is needed) and the CLI type functions."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _live_names(n_text, n_vision):
    """Live parameter names of a UnimoModelF with n_text text and n_vision vision encoder layers.  UnimoEncoder builds both towers
    with the same depth (as the reference does), so the model is built with the larger one and the surplus layers are taken off."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.params import is_dead_param
    L = max(n_text, n_vision)
    tc = TextConfig(num_hidden_layers=L, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=L, image_size=64, patch_size=32)
    model = M.UnimoModelF(default_args(DR_step=3, device="cpu"), vc, tc)
    enc = model.model.encoder
    del enc.text_layer[n_text:]
    del enc.vision_layers[n_vision:]
    return [n for n, p in model.named_parameters() if p.requires_grad and not is_dead_param(n)]


def _closed_form(name, nt, nv, d):
    parts = name.split(".")
    if parts[:2] == ["model", "text_embeddings"]:
        return d ** (nt + 1)
    if parts[:3] == ["model", "encoder", "text_layer"]:
        return d ** (nt + 1 - (int(parts[3]) + 1))
    if parts[:2] in (["model", "vision_embeddings"], ["model", "vision_pre_layrnorm"]):
        return d ** (nv + 1)
    if parts[:3] == ["model", "encoder", "vision_layers"]:
        return d ** (nv + 1 - (int(parts[3]) + 1))
    return 1.0


def test_layer_lr_scale_of_every_live_parameter():
    from d2r_amd.params import layer_lr_scale, tower_layers
    names = _live_names(2, 3)
    assert tower_layers(names) == (2, 3)
    d = 0.5  # powers of two: the closed form is exact
    seen = set()
    for n in names:
        got = layer_lr_scale(n, 2, 3, d)
        assert got == _closed_form(n, 2, 3, d), (n, got)
        assert layer_lr_scale(n, 2, 3, 1.0) == 1.0, n
        seen.add(got)
    assert seen == {1.0, 0.5, 0.25, 0.125, 0.0625}, seen  # text: 1/8 (embeddings), 1/4, 1/2; vision: 1/16, 1/8, 1/4, 1/2; 1 above
    by_sub = lambda sub: {layer_lr_scale(n, 2, 3, d) for n in names if sub in n}
    assert by_sub("glac.text_cls_pool") == {1.0}  # contains "text", is part of the interaction modules
    assert by_sub("model.self_text.0.") == {1.0} and by_sub("model.self_vision.0.") == {1.0}
    assert by_sub("model.vision_pre_layrnorm.") == {d ** 4}
    assert by_sub("model.text_embeddings.") == {d ** 3}
    assert by_sub("model.encoder.text_layer.1.") == {d} and by_sub("model.encoder.vision_layers.0.") == {d ** 3}
    assert all(layer_lr_scale(n, 2, 3, d) == 1.0 for n in names if n.startswith("fc"))
    assert all(any(k in n for n in names) for k in ("glac.text_cls_pool", "model.self_text.0.", "model.vision_pre_layrnorm."))
    # anchored: the same words elsewhere in a name do not count
    assert layer_lr_scale("model.itr_module.x.model.encoder.text_layer.0.w", 2, 3, d) == 1.0
    assert layer_lr_scale("model.text_embeddings_extra.w", 2, 3, d) == 1.0


def _fake_entries():
    """(name, param, offset, numel, group): odd sizes (1 and 6 occur in the real model), tight packing (b|c|d), alignment gaps."""
    mk = lambda *shape: torch.zeros(*shape)
    return [("a.weight", mk(3, 5), 0, 15, 0),      # gap of 1 up to 16
            ("a.bias", mk(5), 16, 5, 0),           # gap of 3
            ("b.weight", mk(2, 3), 24, 6, 0),      # tight: c follows at once
            ("c.weight", mk(1, 1), 30, 1, 0),
            ("d.scale", mk(()), 31, 1, 0),         # 0-d
            ("e.weight", mk(4, 2), 32, 8, 1),      # same hyper-parameters as f, other group than d
            ("f.weight", mk(2, 2, 2), 40, 8, 1),
            ("f.bias", mk(6), 48, 6, 1)], 56       # gap of 2 at the end of the buffer


def test_build_adamw_table_covers_merges_and_keeps_gaps():
    from d2r_amd.params import build_adamw_table
    entries, n = _fake_entries()
    rule = lambda name, p, g: (1.0, 0.0 if p.dim() <= 1 else 0.01)
    segs = build_adamw_table(entries, n, rule)
    ends = [s[0] for s in segs]
    assert ends[-1] == n and all(b > a for a, b in zip([0] + ends, ends))
    # a.weight + its gap | a.bias + its gap | b.weight, c.weight merged | d.scale | e, f merged (their gaps too) | f.bias + end gap
    assert segs == [(16, 1.0, 0.01, 0), (24, 1.0, 0.0, 0), (31, 1.0, 0.01, 0), (32, 1.0, 0.0, 0), (48, 1.0, 0.01, 1), (56, 1.0, 0.0, 1)]
    # every element of every parameter lies in a segment with the parameter's own values; the 1-D rule is p.dim() <= 1
    for name, p, off, numel, g in entries:
        for i in (off, off + numel - 1):
            s = next(s for s in segs if i < s[0])
            assert s[3] == g and s[2] == (0.0 if p.dim() <= 1 else 0.01), (name, i, s)
    # equal neighbours merge down to one segment per group; different scales split again
    assert build_adamw_table(entries, n, lambda *_: (1.0, 0.01)) == [(32, 1.0, 0.01, 0), (56, 1.0, 0.01, 1)]
    by_name = build_adamw_table(entries, n, lambda name, p, g: (0.5 if name.startswith("b.") else 1.0, 0.0))
    assert by_name == [(24, 1.0, 0.0, 0), (30, 0.5, 0.0, 0), (32, 1.0, 0.0, 0), (56, 1.0, 0.0, 1)]
    with pytest.raises(ValueError):
        build_adamw_table(entries, 50, rule)  # the last parameter does not fit
    with pytest.raises(ValueError):
        build_adamw_table(entries[1:], n, rule)  # nothing covers [0, 16)


def _table(rows):
    from d2r_amd import _lib
    return (_lib.AdamwSeg * max(1, len(rows)))(*[_lib.AdamwSeg(*r) for r in rows])


GOOD = [(8, 1.0, 0.01, 0, 0), (20, 0.5, 0.0, 1, 0), (21, 0.0, 0.5, 0, 0), (64, 1.0, 0.0, 1, 0)]


def test_table_check_accepts_and_refuses():
    from d2r_amd import _lib
    lib = _lib.load()
    assert _lib.ADAMW_MAX_SEGMENTS == 4096 and _lib.ADAMW_MAX_GROUPS == 8 and ctypes.sizeof(_lib.AdamwSeg) == 24
    assert lib.d2r_adamw_table_check(_table(GOOD), 4, 64, 2) == 0

    def bad(row, **change):
        rows = [list(r) for r in GOOD]
        for k, val in change.items():
            rows[row][("end", "lr_scale", "weight_decay", "group", "reserved").index(k)] = val
        return [tuple(r) for r in rows]

    cases = [("unsorted ends", bad(1, end=8), 4, 64, 2, b"segment 1"),
             ("ends going back", bad(2, end=19), 4, 64, 2, b"segment 2"),
             ("a first end of 0", bad(0, end=0), 4, 64, 2, b"segment 0"),
             ("last end != n", GOOD, 4, 65, 2, b"segment 3"),
             ("last end != n (short table)", GOOD, 3, 64, 2, b"segment 2"),
             ("NaN scale", bad(1, lr_scale=float("nan")), 4, 64, 2, b"segment 1"),
             ("inf scale", bad(3, lr_scale=float("inf")), 4, 64, 2, b"segment 3"),
             ("negative scale", bad(0, lr_scale=-0.5), 4, 64, 2, b"segment 0"),
             ("negative decay", bad(2, weight_decay=-1e-3), 4, 64, 2, b"segment 2"),
             ("NaN decay", bad(2, weight_decay=float("nan")), 4, 64, 2, b"segment 2"),
             ("group too large", bad(3, group=2), 4, 64, 2, b"segment 3"),
             ("negative group", bad(0, group=-1), 4, 64, 2, b"segment 0"),
             ("reserved", bad(1, reserved=7), 4, 64, 2, b"segment 1"),
             ("nseg 0", GOOD, 0, 64, 2, b"nseg"),
             ("nseg above the maximum", GOOD, _lib.ADAMW_MAX_SEGMENTS + 1, 64, 2, b"nseg"),
             ("no groups", GOOD, 4, 64, 0, b"ngroups"),
             ("too many groups", GOOD, 4, 64, _lib.ADAMW_MAX_GROUPS + 1, b"ngroups")]
    for what, rows, nseg, n, ngroups, word in cases:
        assert lib.d2r_adamw_table_check(_table(rows), nseg, n, ngroups) == -1, what
        err = lib.d2r_last_error()
        assert b"d2r_adamw_table_check" in err and word in err, (what, err)
    assert lib.d2r_adamw_table_check(None, 4, 64, 2) == -1
    # the largest table passes
    big = [(i + 1, 1.0, 0.0, i % 8, 0) for i in range(_lib.ADAMW_MAX_SEGMENTS)]
    assert lib.d2r_adamw_table_check(_table(big), len(big), len(big), 8) == 0


def test_step_entry_points_refuse_before_enqueuing():
    """Host memory stands in for the device buffers: every call here must be refused by the argument checks, so nothing is ever
    launched on it (and no GPU is needed)."""
    from d2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 96)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    tab = _table(GOOD)
    t = ctypes.addressof(tab)
    lr = (ctypes.c_float * 2)(1e-3, 1e-3)

    def eager(w=p, g=p, m=p, v=p, begin=0, end=64, table=t, nseg=4, n=64, lr_=lr, ngroups=2, step=1, ema=None, omd=0.0):
        return lib.d2r_adamw_step_table(w, g, m, v, None, 1, begin, end, table, nseg, n, lr_, ngroups, 0.9, 0.999, 1e-8, step, 1.0,
                                        None, None, ema, omd, None)

    def dev(w=p, g=p, m=p, v=p, begin=0, end=64, table=t, nseg=4, n=64, hyper=p, ngroups=2, ema=None, d_omd=None):
        return lib.d2r_adamw_step_table_dev(w, g, m, v, None, 1, begin, end, table, nseg, n, hyper, ngroups, 0.9, 0.999, 1e-8, None,
                                            None, ema, d_omd, None)

    for fn, name in ((eager, b"d2r_adamw_step_table"), (dev, b"d2r_adamw_step_table_dev")):
        for what, kw in [("null w", dict(w=None)), ("null g", dict(g=None)), ("null m", dict(m=None)), ("null v", dict(v=None)),
                         ("null table", dict(table=None)), ("begin % 4", dict(begin=2)), ("begin % 4 (odd)", dict(begin=5)),
                         ("end < begin", dict(begin=8, end=4)), ("negative begin", dict(begin=-4)), ("end beyond the table", dict(end=65)),
                         ("nseg 0", dict(nseg=0)), ("nseg above the maximum", dict(nseg=_lib.ADAMW_MAX_SEGMENTS + 1)),
                         ("no groups", dict(ngroups=0)), ("too many groups", dict(ngroups=_lib.ADAMW_MAX_GROUPS + 1)),
                         ("misaligned w", dict(w=p + 4)), ("ema is w", dict(ema=p, d_omd=p) if fn is dev else dict(ema=p, omd=0.5))]:
            assert fn(**kw) == -1, (name, what)
            assert name in lib.d2r_last_error(), (name, what, lib.d2r_last_error())
    assert eager(lr_=None) == -1 and eager(step=0) == -1
    assert eager(ema=p + 64, omd=1.5) == -1 and eager(ema=p + 64, omd=float("nan")) == -1
    assert dev(hyper=None) == -1
    assert dev(ema=p + 64, d_omd=None) == -1
    assert all(x == 0.0 for x in buf), "a refused call wrote"
    # an empty range is accepted and launches nothing
    assert eager(begin=8, end=8) == 0 and dev(begin=64, end=64) == 0


def test_cli_flags_and_constructor_refuse_bad_values():
    from d2r_amd.params import FusedAdamW
    from d2r_amd.run import build_parser
    p = build_parser()
    a = p.parse_args([])
    assert a.layer_lr_decay == 1.0 and a.wd_exempt_1d is False and a.weight_decay == 1e-2
    a = p.parse_args(["--layer_lr_decay", "0.8", "--wd_exempt_1d", "--weight_decay", "0.05"])
    assert a.layer_lr_decay == 0.8 and a.wd_exempt_1d is True and a.weight_decay == 0.05
    assert p.parse_args(["--weight_decay", "0"]).weight_decay == 0.0 and p.parse_args(["--layer_lr_decay", "1"]).layer_lr_decay == 1.0
    for flag, values in (("--layer_lr_decay", ("0", "-0.5", "1.0001", "nan", "inf")), ("--weight_decay", ("-1e-9", "nan", "inf", "-inf"))):
        for bad in values:
            with pytest.raises(SystemExit):
                p.parse_args([flag, bad])
    for bad in (0.0, -0.1, 1.5, math.nan, math.inf):
        with pytest.raises(ValueError, match="layer_lr_decay"):
            FusedAdamW(None, lr=1e-3, layer_lr_decay=bad)  # refused before the store is looked at
    for bad in (-1e-3, math.nan, math.inf):
        with pytest.raises(ValueError, match="weight_decay"):
            FusedAdamW(None, lr=1e-3, weight_decay=bad)
