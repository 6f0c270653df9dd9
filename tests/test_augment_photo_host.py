"""Photometric augmentation on the host: image.reference_photo anchored on Pillow's ImageEnhance and on colorsys, the
draws of Augmenter.draw_photo and its second generator (the crop / flip stream and torch's default generator left alone), the entry
point in the header, the library and d2r_amd._lib with its argument checks (no launch happens), the six command-line flags and
run.main's wiring."""
import colorsys
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

OFF = (1.0, 1.0, 1.0, 0.0, 0, 0, 0, 0, 0)  # brightness, contrast, saturation, hue, gray, ex0, ey0, ew, eh


def _photo(**kw):
    names = ("brightness", "contrast", "saturation", "hue", "gray", "ex0", "ey0", "ew", "eh")
    assert set(kw) <= set(names)
    return tuple(kw.get(n, d) for n, d in zip(names, OFF))


@pytest.fixture(scope="module")
def image32():
    """uint8 planar [3, 32, 32], uniform random, and its values in [0, 1] the way reference_photo returns them un-normalised."""
    return np.random.default_rng(22).integers(0, 256, (3, 32, 32), dtype=np.uint8)


def _unit(I, crop, photo, box=None):
    """reference_photo with mean 0 and std 1: the values in [0, 1] before the normalisation."""
    S = crop.shape[1]
    return I.reference_photo(crop, box or (0, 0, S, S, 0), photo, S, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@pytest.mark.parametrize("factor", [0.6, 1.4])
@pytest.mark.parametrize("option", ["brightness", "contrast", "saturation"])
def test_reference_photo_agrees_with_pillows_image_enhance(image32, option, factor):
    """Within 1.5 / 255 of Pillow's ImageEnhance.Brightness / Contrast / Color on the same image (Pillow rounds to uint8 and uses an
    integer mean; a restatement of K22 measured at most 1.18 / 255)."""
    from PIL import Image, ImageEnhance
    from d2r_amd import image as I
    pil = Image.fromarray(np.ascontiguousarray(image32.transpose(1, 2, 0)), "RGB")
    enhance = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}[option]
    want = np.asarray(enhance(pil).enhance(factor)).transpose(2, 0, 1).astype(np.float64) / 255.0
    got = _unit(I, image32, _photo(**{option: factor}))
    err = float(np.abs(got - want).max()) * 255.0
    print(f"{option} {factor}: max |reference_photo - Pillow| = {err:.3f} / 255")
    assert err <= 1.5, (option, factor, err)
    assert float(np.abs(got - image32 / 255.0).max()) > 0.05, "the option changed nothing"


@pytest.mark.parametrize("delta", [-0.5, -0.1, 0.0, 0.07, 0.5])
def test_reference_photo_hue_agrees_with_colorsys(image32, delta):
    from d2r_amd import image as I
    crop = image32.copy()
    crop[:, 0, :6] = np.array([[0, 255, 128, 255, 0, 200], [0, 255, 128, 0, 255, 200], [0, 255, 128, 0, 255, 10]], np.uint8)  # greys, primaries, ties
    got = _unit(I, crop, _photo(hue=delta))
    x = crop.astype(np.float64) / 255.0
    want = np.empty_like(x)
    for i in range(32):
        for j in range(32):
            h, s, v = colorsys.rgb_to_hsv(*x[:, i, j])
            want[:, i, j] = colorsys.hsv_to_rgb((h + delta) % 1.0, s, v)
    err = float(np.abs(got - want).max())
    print(f"hue {delta}: max |reference_photo - colorsys| = {err:.3g}")
    assert err <= 1e-12, (delta, err)
    if delta == 0.0:
        np.testing.assert_array_equal(got, x)
    else:
        assert float(np.abs(got - x).max()) > 0.05


def test_identity_factors_return_the_input_and_only_the_box_is_reference_augment(image32):
    from d2r_amd import image as I
    S = 32
    raw = np.tile(np.arange(256, dtype=np.float64) / 255.0, (3, 1))
    np.testing.assert_array_equal(_unit(I, image32, OFF), image32 / 255.0)
    mean, std = np.asarray(I.CLIP_MEAN)[:, None, None], np.asarray(I.CLIP_STD)[:, None, None]
    for box in ((0, 0, S, S, 0), (3, 5, 20, 11, 1), (31, 0, 1, 32, 0)):
        want = (I.reference_augment(image32, box, S, raw) - mean) / std
        np.testing.assert_array_equal(I.reference_photo(image32, box, OFF, S), want)
        np.testing.assert_array_equal(I.reference_photo(image32, box, OFF, S, I.CLIP_MEAN, I.CLIP_STD), want)
    # grayscale: three equal channels of 0.299 R + 0.587 G + 0.114 B; erase: zeros inside, untouched outside
    g = _unit(I, image32, _photo(gray=1))
    x = image32 / 255.0
    np.testing.assert_allclose(g[0], 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2], rtol=0, atol=1e-15)
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[0], g[2])
    e = I.reference_photo(image32, (0, 0, S, S, 0), _photo(ex0=4, ey0=9, ew=7, eh=3), S)
    plain = I.reference_photo(image32, (0, 0, S, S, 0), OFF, S)
    inside = np.zeros((S, S), bool)
    inside[9:12, 4:11] = True
    assert bool((e[:, inside] == 0.0).all()) and np.array_equal(e[:, ~inside], plain[:, ~inside])
    # contrast moves every pixel toward / away from the mean of g after the brightness step
    c = _unit(I, image32, _photo(brightness=0.5, contrast=0.25))
    m = (0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]).mean() * 0.5
    np.testing.assert_allclose(c, 0.25 * 0.5 * x + 0.75 * m, rtol=0, atol=1e-15)
    for bad in (_photo(brightness=-0.1), _photo(contrast=float("nan")), _photo(saturation=float("inf")), _photo(hue=0.51), _photo(gray=2),
                _photo(ex0=30, ew=3, eh=1), _photo(ew=-1, eh=1), _photo(ew=1, eh=0)):
        with pytest.raises(ValueError):
            I.reference_photo(image32, (0, 0, S, S, 0), bad, S)


def _fields(d):
    f = d[:, :4].contiguous().view(torch.float32).double()
    return f[:, 0], f[:, 1], f[:, 2], f[:, 3], d[:, 4].long(), d[:, 5].long(), d[:, 6].long(), d[:, 7].long(), d[:, 8].long()


def test_draws_keep_their_ranges_and_the_erase_box_lies_inside_the_crop():
    from d2r_amd.augment import Augmenter
    S, n = 224, 4096
    aug = Augmenter(S, seed=3, brightness=0.4, contrast=1.5, saturation=0.25, hue=0.1, grayscale_p=0.1, erase_p=0.25)
    assert aug.photometric
    d = aug.draw_photo(n)
    assert d.shape == (n, 12) and d.dtype == torch.int32 and d.is_contiguous() and bool((d[:, 9:] == 0).all())
    b, c, s, h, gray, ex0, ey0, ew, eh = _fields(d)
    f32 = lambda v: float(np.float32(v))  # noqa: E731  the descriptor holds the fp32 rounding of the float64 draw
    for v, J in ((b, 0.4), (c, 1.5), (s, 0.25)):
        lo, hi = max(0.0, 1.0 - J), 1.0 + J
        assert float(v.min()) >= f32(lo) and float(v.max()) <= f32(hi), (J, float(v.min()), float(v.max()))
        assert float(v.min()) < lo + 0.02 * (hi - lo) and float(v.max()) > hi - 0.02 * (hi - lo), "the range is not used"
    assert float(h.min()) >= -f32(0.1) and float(h.max()) <= f32(0.1) and float(h.min()) < -0.095 and float(h.max()) > 0.095
    assert bool(((gray == 0) | (gray == 1)).all())
    sd = lambda p: 5 * (n * p * (1 - p)) ** 0.5  # noqa: E731  five binomial standard deviations
    assert abs(int(gray.sum()) - 0.1 * n) <= sd(0.1)
    on = ew > 0
    assert abs(int(on.sum()) - 0.25 * n) <= sd(0.25)
    assert bool((d[~on][:, 5:9] == 0).all())
    assert bool(((ex0 >= 0) & (ey0 >= 0) & (ew >= 1) & (eh >= 1) & (ex0 + ew <= S) & (ey0 + eh <= S))[on].all())
    # sides are rounded, so w * h is within (w + h + 1) / 2 of the drawn area (as in test_augment_host.py); a side clamped to S only shrinks a box
    area, ratio = (ew * eh).double()[on], (eh.double() / ew.double())[on]
    slack = ((ew + eh + 1).double() / 2)[on]
    assert bool((area >= 0.02 * S * S - slack).all()) and bool((area <= 0.33 * S * S + slack).all())
    assert float(area.min()) < 0.04 * S * S and float(area.max()) > 0.31 * S * S
    assert float(ratio.min()) >= 0.28 and float(ratio.max()) <= 3.5 and float(ratio.min()) < 0.35 and float(ratio.max()) > 3.0
    assert int(ex0[on].min()) == 0 or int(ex0[on].min()) < 4
    assert bool((ex0 + ew == S)[on].any()) or int((ex0 + ew)[on].max()) > S - 4
    # tiny crops: every box inside, always erased with erase_p = 1; options at 0 give exact identities
    for S in (1, 2, 5):
        d = Augmenter(S, seed=S, erase_p=1.0).draw_photo(500)
        b, c, s, h, gray, ex0, ey0, ew, eh = _fields(d)
        assert bool(((ex0 >= 0) & (ey0 >= 0) & (ew >= 1) & (eh >= 1) & (ex0 + ew <= S) & (ey0 + eh <= S)).all())
        assert bool(((b == 1) & (c == 1) & (s == 1) & (h == 0) & (gray == 0)).all())
    # a jitter above 1 clamps the lower end at 0
    b = _fields(Augmenter(8, brightness=3.0).draw_photo(2000))[0]
    assert float(b.min()) >= 0.0 and float(b.min()) < 0.1 and float(b.max()) > 3.9


def test_second_generator_seeds_streams_and_leaves_the_first_and_the_default_generator_alone():
    from d2r_amd.augment import Augmenter, photo_stream_seed, stream_seed
    on = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, grayscale_p=0.1, erase_p=0.25)
    torch.manual_seed(123)
    before = torch.get_rng_state()
    plain = Augmenter(224, 0.5, 0.5, seed=7)
    a, b = Augmenter(224, 0.5, 0.5, seed=7, **on), Augmenter(224, 0.5, 0.5, seed=7, **on)
    assert plain.photo_generator is None and not plain.photometric
    assert a.photo_generator.initial_seed() == photo_stream_seed(7, 0) and a.generator.initial_seed() == stream_seed(7, 0)
    # the crop / flip stream is what it was
    assert torch.equal(plain.draw(32), a.draw(32))
    da, db = [a.draw_photo(32) for _ in range(3)], [b.draw_photo(32) for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(da, db))
    assert not torch.equal(da[0], da[1]), "successive batches get the same descriptors"
    assert torch.equal(plain.draw(32), a.draw(32)), "the photometric draws moved the crop / flip stream"
    other_rank, other_seed = Augmenter(224, seed=7, rank=1, **on), Augmenter(224, seed=8, **on)
    assert not torch.equal(da[0], other_rank.draw_photo(32)) and not torch.equal(da[0], other_seed.draw_photo(32))
    assert torch.equal(torch.get_rng_state(), before), "drawing moved torch's default generator"
    # the settings do not change how much of the stream a batch consumes
    c, e = Augmenter(224, seed=7, hue=0.2), Augmenter(224, seed=7, **on)
    c.draw_photo(5), e.draw_photo(5)
    assert torch.equal(c.photo_generator.get_state(), e.photo_generator.get_state())
    seeds = {photo_stream_seed(s, r) for s in (0, 1, 2023, 2 ** 32 - 1) for r in (0, 1, 7, 2 ** 24 - 1)}
    assert len(seeds) == 16 and all(0 <= s < 2 ** 64 for s in seeds)
    assert not seeds & {stream_seed(s, r) for s in (0, 1, 2023, 2 ** 32 - 1) for r in (0, 1, 7, 2 ** 24 - 1)}
    with pytest.raises(RuntimeError):
        plain.draw_photo(4)
    for bad in (dict(brightness=-0.1), dict(contrast=float("nan")), dict(saturation=float("inf")), dict(hue=0.6), dict(hue=-0.1),
                dict(grayscale_p=1.5), dict(erase_p=-0.5)):
        with pytest.raises(ValueError):
            Augmenter(224, **bad)
    with pytest.raises(ValueError, match="rescale"):
        Augmenter(224, hue=0.1, norm=((0.5,) * 3, (0.5,) * 3, 1 / 256))
    Augmenter(224, norm=((0.5,) * 3, (0.5,) * 3, 1 / 256))  # nothing photometric on: any rescale
    assert "brightness" not in plain.describe() and plain.describe() == Augmenter(224, 0.5, 0.5).describe()
    text = a.describe()
    assert text.startswith(plain.describe()) and all(w in text for w in ("brightness 0.4", "hue 0.1", "grayscale", "erasing", "0.25"))


def test_entry_points_are_declared_documented_exported_and_typed():
    from d2r_amd import _lib
    text = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "size_t": _lib.sz}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, count in (("d2r_clip_cache_augment_photo", "int", 16), ("d2r_clip_cache_augment_photo_ws_bytes", "size_t", 2)):
        m = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/d2r_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert name in comments
        res, argtypes = _lib.SIGNATURES[name]
        assert res is kinds[ret] and len(argtypes) == len(args) == count
        for a, t in zip(args, argtypes):
            if "*" in a:
                assert t is _lib.vp or issubclass(t, ctypes._Pointer), (a, t)
            else:
                assert t is kinds[a.split()[-2]], (a, t)
        assert hasattr(lib, name)
    argtypes = _lib.SIGNATURES["d2r_clip_cache_augment_photo"][1]
    assert argtypes[4] == ctypes.POINTER(_lib.ClipAugmentDesc) and argtypes[6] == ctypes.POINTER(_lib.ClipPhotoDesc)
    assert "d2r_clip_photo_desc" in hdr and ctypes.sizeof(_lib.ClipPhotoDesc) == 48
    assert [f[0] for f in _lib.ClipPhotoDesc._fields_] == ["brightness", "contrast", "saturation", "hue", "gray", "ex0", "ey0", "ew", "eh",
                                                          "reserved"]
    assert all(f[1] is _lib.f32 for f in _lib.ClipPhotoDesc._fields_[:4]) and all(f[1] is _lib.i32 for f in _lib.ClipPhotoDesc._fields_[4:9])
    _lib.load()
    ws = _lib._FN["d2r_clip_cache_augment_photo_ws_bytes"]
    # one partial sum per 256 pixel quads of a sample: ceil(S * ceil(S / 4) / 256) floats
    assert ws(1, 1) == 4 and ws(4, 16) == 16 and ws(1, 224) == 4 * 49 and ws(32, 224) == 32 * 4 * 49 and ws(0, 16) == 0 and ws(1, 0) == 0


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Everything is checked on the host copies: these calls never reach a launch (the device pointers are dummies)."""
    from d2r_amd import image as I
    lib = I._lib.load()
    fake, S = 1 << 20, 16
    ok_box, ok = (0, 0, S, S, 0), OFF

    def call(photos, boxes=None, idx=None, rows=5, S=S, h_photo=True, photo=fake, ws=fake, ws_bytes=None, reserved=None, norm=None,
             rescale=1 / 255, cache=fake):
        B = len(photos)
        h = np.asarray(idx if idx is not None else list(range(B)), np.int64)
        d = np.zeros((B, 8), np.int32)
        d[:, :5] = np.asarray(boxes or [ok_box] * B, np.int32)
        p = I.photo_desc(photos).numpy().copy()
        if reserved is not None:
            p[-1, 9 + reserved] = 1
        nm = (ctypes.c_float * 6)(*(norm or (I.CLIP_MEAN + I.CLIP_STD)))
        need = lib.d2r_clip_cache_augment_photo_ws_bytes(B, S)
        rc = lib.d2r_clip_cache_augment_photo(cache, rows, h.ctypes.data, fake, ctypes.cast(d.ctypes.data, ctypes.POINTER(I._lib.ClipAugmentDesc)),
                                              fake, ctypes.cast(p.ctypes.data, ctypes.POINTER(I._lib.ClipPhotoDesc)) if h_photo else None,
                                              photo, B, S, nm, rescale, fake, ws, need if ws_bytes is None else ws_bytes, None)
        return rc, lib.d2r_last_error().decode()

    bad_fields = {"brightness": (-0.5, float("nan"), float("inf")), "contrast": (-1e-3, float("nan")), "saturation": (-2.0, float("-inf")),
                  "hue": (0.51, -0.6, float("nan")), "gray": (2, -1)}
    for name, values in bad_fields.items():
        for v in values:
            rc, err = call([ok, _photo(**{name: v})])
            assert rc == -1 and "sample 1" in err and name in err, (name, v, err)
    for box in (dict(ex0=-1, ew=2, eh=2), dict(ey0=-1, ew=2, eh=2), dict(ew=-1, eh=2), dict(ew=2, eh=0), dict(ex0=15, ew=2, eh=1),
                dict(ey0=15, ew=1, eh=2), dict(ew=S + 1, eh=1), dict(ex0=2 ** 31 - 1, ew=2, eh=1)):
        rc, err = call([ok, _photo(**box)])
        assert rc == -1 and "sample 1" in err and "erase box" in err, (box, err)
    for k in range(3):
        rc, err = call([ok, ok], reserved=k)
        assert rc == -1 and "reserved" in err, err
    # what K21 checks: indices, boxes, flip
    rc, err = call([ok, ok], idx=[0, 5])
    assert rc == -1 and "outside the 5 rows" in err
    rc, err = call([ok, ok], boxes=[ok_box, (13, 0, 4, 4, 0)])
    assert rc == -1 and "does not lie inside" in err
    rc, err = call([ok], boxes=[(0, 0, 4, 4, 2)])
    assert rc == -1 and "flip" in err
    # null descriptors, workspace, alignment, sizes, normalisation
    assert call([ok], h_photo=False)[0] == -1 and call([ok], photo=None)[0] == -1 and call([ok], ws=None)[0] == -1
    rc, err = call([ok, ok], ws_bytes=2 * 4 - 1)
    assert rc == -3 and "workspace" in err, (rc, err)  # D2R_ERR_WORKSPACE
    rc, err = call([ok], S=224, ws_bytes=4 * 48)
    assert rc == -3 and "workspace" in err
    assert call([ok], cache=fake + 8)[0] == -1 and "aligned" in call([ok], ws=fake + 2)[1] and "aligned" in call([ok], photo=fake + 1)[1]
    assert call([ok], S=0)[0] == -1 and call([ok], S=4097)[0] == -1
    for norm in ((0.5, 0.5, float("nan"), 1, 1, 1), (0.5, 0.5, 0.5, 1, 0.0, 1), (0.5, 0.5, 0.5, 1, 1, float("inf"))):
        assert call([ok], norm=norm)[0] == -1
    assert call([ok], rescale=0.0)[0] == -1 and call([ok], rescale=float("nan"))[0] == -1


def test_flag_ranges_and_refusal_on_synthetic_data():
    from d2r_amd.run import PHOTO_FLAGS, build_parser, main
    p = build_parser()
    d = p.parse_args([])
    assert PHOTO_FLAGS == ("aug_brightness", "aug_contrast", "aug_saturation", "aug_hue", "aug_grayscale", "aug_erase")
    assert all(getattr(d, f) == 0.0 for f in PHOTO_FLAGS)
    a = p.parse_args(["--aug_brightness", "0.4", "--aug_contrast", "1.5", "--aug_saturation", "0.4", "--aug_hue", "0.5", "--aug_grayscale", "1",
                      "--aug_erase", "0.25"])
    assert [getattr(a, f) for f in PHOTO_FLAGS] == [0.4, 1.5, 0.4, 0.5, 1.0, 0.25]
    for flag in ("--aug_brightness", "--aug_contrast", "--aug_saturation"):
        for bad in ("-0.1", "nan", "inf", "much"):
            with pytest.raises(SystemExit):
                p.parse_args([flag, bad])
    for bad in (["--aug_hue", "0.6"], ["--aug_hue", "-0.1"], ["--aug_hue", "nan"], ["--aug_grayscale", "1.5"], ["--aug_grayscale", "-0.1"],
                ["--aug_grayscale", "nan"], ["--aug_erase", "1.5"], ["--aug_erase", "-1"], ["--aug_erase", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for flag in PHOTO_FLAGS:
        with pytest.raises(SystemExit, match="synthetic"):
            main(["--" + flag, "0.3"])


class _StubCache:
    device = torch.device("cpu")

    def gather(self, h_idx, idx, augmenter=None):
        return h_idx, augmenter


class _StubSplit(torch.utils.data.Dataset):
    """What cache_loaders and run.main look at in an MSDDataset: a length and max_seq."""
    max_seq = 16

    def __init__(self, *args, **kwargs):
        pass

    def __len__(self):
        return 10

    def __getitem__(self, i):
        return i


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


def test_run_hands_the_photometric_augmenter_to_the_training_split_only(monkeypatch, tmp_path, caplog):
    """run.main with the dataset, the model and the trainer stubbed, and cache_loaders' for_loader / prefill stubbed (a stub cache):
    the cached training loader, or without the cache the trainer, receives an augmenter carrying the photometric settings; the dev /
    test loaders never do.  One photometric flag alone builds the augmenter, with identity boxes.  --only_test: none is built and a
    line says so.  A preprocessor whose rescale is not 1/255 is refused by name."""
    from d2r_amd import cache as C, data as D, image as I, modules as M, run, train as T
    from d2r_amd.augment import Augmenter, photo_stream_seed, stream_seed
    for name in ("train.json", "dev.json", "test.json"):
        (tmp_path / name).write_text("[]")
    monkeypatch.setattr(C.DeviceDatasetCache, "for_loader", staticmethod(lambda dl, device, split, logger=None: _StubCache()))
    monkeypatch.setattr(C, "prefill", lambda dl, cache, logger=None, split="": None)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 40, 1 << 40))
    monkeypatch.setattr(D, "MSDDataset", _StubSplit)
    monkeypatch.setattr(M, "UnimoModelF", lambda **kwargs: object())
    monkeypatch.setattr(T, "MSDTrainer", _StubTrainer)
    monkeypatch.setattr(run, "set_seed", lambda seed: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--data_path", str(tmp_path), "--img_path", str(tmp_path), "--bert_name", str(tmp_path), "--device", "cpu", "--seed", "5",
            "--num_workers", "0"]
    on = ["--aug_brightness", "0.4", "--aug_contrast", "0.3", "--aug_saturation", "0.2", "--aug_hue", "0.1", "--aug_grayscale", "0.15",
          "--aug_erase", "0.25"]

    def main(extra):
        del _StubTrainer.made[:]
        run.main(base + extra)
        assert len(_StubTrainer.made) == 1
        return _StubTrainer.made[0].kwargs

    def check(aug, crop=1.0, flip=0.0, settings=(0.4, 0.3, 0.2, 0.1, 0.15, 0.25)):
        assert isinstance(aug, Augmenter) and aug.photometric and (aug.S, aug.crop_scale, aug.flip_p) == (224, crop, flip)
        assert (aug.brightness, aug.contrast, aug.saturation, aug.hue, aug.grayscale_p, aug.erase_p) == settings
        assert aug.generator.initial_seed() == stream_seed(5, 0) and aug.photo_generator.initial_seed() == photo_stream_seed(5, 0)
        assert aug.norm == (I.CLIP_MEAN, I.CLIP_STD, I.RESCALE)

    state = torch.get_rng_state()
    kwargs = main(on + ["--cache_dataset", "device"])
    assert kwargs["augmenter"] is None, "the cached training loader augments its own batches"
    train, dev, test = kwargs["train_data"], kwargs["dev_data"], kwargs["test_data"]
    check(train.augmenter)
    assert dev.augmenter is None and test.augmenter is None
    assert all(a is train.augmenter for _, a in train) and all(a is None for _, a in dev) and all(a is None for _, a in test)
    boxes = train.augmenter.draw(4)
    assert bool((boxes[:, :5] == torch.tensor([0, 0, 224, 224, 0], dtype=torch.int32)).all()), "crop / flip are off: identity boxes"

    kwargs = main(on + ["--aug_crop_scale", "0.25", "--aug_flip", "0.75"])
    check(kwargs["augmenter"], 0.25, 0.75)
    assert not hasattr(kwargs["dev_data"], "augmenter") and not hasattr(kwargs["test_data"], "augmenter")

    kwargs = main(["--aug_erase", "0.5"])  # one flag alone creates the augmenter
    check(kwargs["augmenter"], settings=(0.0, 0.0, 0.0, 0.0, 0.0, 0.5))
    kwargs = main(["--aug_flip", "0.5"])  # none of the six: today's augmenter
    assert isinstance(kwargs["augmenter"], Augmenter) and not kwargs["augmenter"].photometric
    assert main([])["augmenter"] is None

    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        kwargs = main(on + ["--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert "augmenter" not in kwargs
    lines = [r.getMessage() for r in caplog.records if "ignored with --only_test" in r.getMessage()]
    assert len(lines) == 1 and all("--" + f in lines[0] for f in run.PHOTO_FLAGS), lines

    (tmp_path / "preprocessor_config.json").write_text('{"size": 224, "crop_size": 224, "rescale_factor": 0.00390625}')
    monkeypatch.setattr(run, "load_pretrained", lambda args, weights=True: (None, type("V", (), {"image_size": 224, "patch_size": 32})(), None, None))
    with pytest.raises(SystemExit, match="rescale_factor"):
        main(on + ["--pretrained", "--vit_name", str(tmp_path)])
    main(["--aug_flip", "0.5", "--pretrained", "--vit_name", str(tmp_path)])  # crop / flip go through the table: any rescale
    torch.set_rng_state(state)  # the shuffled stub loader drew from the default generator
