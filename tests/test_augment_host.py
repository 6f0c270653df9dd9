"""Image augmentation on the host: image.reference_augment against torch's own bilinear interpolate in float64, the boxes
Augmenter.draw produces, its generator (seeding rule, ranks, torch's default generator left alone), the entry point in the header,
the library and d2r_amd._lib with its argument checks (no launch happens), and the two command-line flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


def _boxes(S):
    """full, 1 x 1, 1 x h, w x 1, the four corners and one interior box of an S x S crop (duplicates dropped at tiny S)."""
    m = max(S // 2, 1)
    boxes = [(0, 0, S, S), (S // 2, S // 3, 1, 1), (S - 1, 0, 1, S), (0, S - 1, S, 1), (min(1, S - 1), 0, 1, m), (0, min(1, S - 1), m, 1),
             (0, 0, m, m), (S - m, 0, m, m), (0, S - m, m, m), (S - m, S - m, m, m)]
    if S >= 4:
        boxes.append((1, 2, S - 3, S - 3))
    if S >= 7:
        boxes.append((2, 1, 3, 5))
    return sorted(set(boxes))


def _oracle(crop, table, box, S):
    x0, y0, w, h, flip = box
    T = torch.stack([torch.from_numpy(table[c].astype(np.float64))[torch.from_numpy(crop[c].astype(np.int64))] for c in range(3)])
    out = F.interpolate(T[:, y0:y0 + h, x0:x0 + w].double()[None], size=(S, S), mode="bilinear", align_corners=False)[0]
    return (out.flip(-1) if flip else out).numpy()


@pytest.mark.parametrize("S", [1, 2, 7, 16])
def test_reference_augment_is_torchs_bilinear_interpolate_of_the_box(S):
    from d2r_amd import image as I
    rng = np.random.default_rng(S)
    crop = rng.integers(0, 256, (3, S, S), dtype=np.uint8)
    tables = [I.normalize_table(), (rng.standard_normal((3, 256)) * 50).astype(np.float32)]
    n = 0
    for table in tables:
        for x0, y0, w, h in _boxes(S):
            for flip in (0, 1):
                got = I.reference_augment(crop, (x0, y0, w, h, flip), S, table)
                want = _oracle(crop, table, (x0, y0, w, h, flip), S)
                assert got.shape == (3, S, S) and got.dtype == np.float64
                err = float(np.abs(got - want).max())
                assert err <= 1e-12, (S, (x0, y0, w, h, flip), err)
                n += 1
    assert n >= 4
    # the identity box returns the table's values themselves
    got = I.reference_augment(crop, (0, 0, S, S, 0), S, tables[0])
    np.testing.assert_array_equal(got, np.stack([tables[0][c][crop[c]] for c in range(3)]).astype(np.float64))
    for bad in ((-1, 0, 1, 1, 0), (0, 0, S + 1, 1, 0), (0, 0, 0, 1, 0), (1, 0, S, 1, 0), (0, 0, 1, 1, 2)):
        with pytest.raises(ValueError):
            I.reference_augment(crop, bad, S, tables[0])


@pytest.mark.parametrize("LO", [0.08, 0.5, 1.0])
def test_draw_boxes_lie_inside_the_crop_and_keep_the_area_range(LO):
    """Area range: before rounding the sides are a = sqrt(area * r), b = sqrt(area / r) with a * b = area in [LO, 1] * S^2.  A side
    longer than S is clamped to S; that only happens when area / r > S^2 (or area * r > S^2), where the other side is
    sqrt(area * r) >= sqrt(3/4 * area) with area > 3/4 * S^2, so the clamped sides a', b' have a' * b' >= min(LO, 3/4) * S^2.
    Rounding moves each side by at most 1/2: w >= a' - 1/2, h >= b' - 1/2, so w * h >= a' * b' - (a' + b') / 2 + 1/4 and
    a' + b' <= w + h + 1.  Hence min(LO, 3/4) * S^2 - (w + h + 1) / 2 + 1/4 <= w * h <= S^2 (the upper end is the clamp)."""
    from d2r_amd.augment import Augmenter
    S, n = 224, 10000
    d = Augmenter(S, LO, 0.0, seed=3).draw(n)
    assert d.shape == (n, 8) and d.dtype == torch.int32 and d.is_contiguous()
    x0, y0, w, h, flip = (d[:, k].long() for k in range(5))
    assert bool((d[:, 5:] == 0).all()) and bool((flip == 0).all())
    assert bool(((x0 >= 0) & (y0 >= 0) & (w >= 1) & (h >= 1) & (x0 + w <= S) & (y0 + h <= S)).all())
    if LO == 1.0:
        assert bool(((x0 == 0) & (y0 == 0) & (w == S) & (h == S)).all()), "crop_scale 1 with flip 0 is the identity"
        return
    area = (w * h).double()
    lower = min(LO, 0.75) * S * S - (w + h + 1).double() / 2 + 0.25
    assert bool((area >= lower).all()) and bool((area <= S * S).all())
    # the range is used, not only respected: small and large boxes, wide and tall ones, every offset side
    assert float(area.min()) < (LO + 0.05) * S * S and float(area.max()) > 0.95 * S * S
    ratio = w.double() / h.double()
    assert float(ratio.min()) < 0.8 and float(ratio.max()) > 1.25
    assert int(x0.max()) > 0 and int(y0.max()) > 0 and bool((x0 + w == S).any()) and bool((x0 == 0).any())


def test_draw_at_a_tiny_crop_and_flip_rate():
    from d2r_amd.augment import Augmenter
    for S in (1, 2, 5):
        d = Augmenter(S, 0.08, 1.0, seed=S).draw(2000).long()
        assert bool(((d[:, 0] >= 0) & (d[:, 1] >= 0) & (d[:, 2] >= 1) & (d[:, 3] >= 1) & (d[:, 0] + d[:, 2] <= S) &
                     (d[:, 1] + d[:, 3] <= S)).all())
        assert bool((d[:, 4] == 1).all())
    n = 10000
    flips = int(Augmenter(224, 1.0, 0.5, seed=11).draw(n)[:, 4].sum())
    sd = math.sqrt(n * 0.5 * 0.5)  # binomial standard deviation
    assert abs(flips - n * 0.5) <= 5 * sd, flips


def test_generators_equal_seeds_equal_streams_ranks_differ_default_generator_untouched():
    from d2r_amd.augment import Augmenter, stream_seed
    torch.manual_seed(123)
    before = torch.get_rng_state()
    a, b = Augmenter(224, 0.5, 0.5, seed=7, rank=0), Augmenter(224, 0.5, 0.5, seed=7, rank=0)
    other_rank, other_seed = Augmenter(224, 0.5, 0.5, seed=7, rank=1), Augmenter(224, 0.5, 0.5, seed=8, rank=0)
    da = [a.draw(32) for _ in range(3)]
    db = [b.draw(32) for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(da, db))
    assert not torch.equal(da[0], da[1]), "successive batches get the same boxes"
    assert not torch.equal(da[0], other_rank.draw(32)) and not torch.equal(da[0], other_seed.draw(32))
    assert torch.equal(torch.get_rng_state(), before), "drawing moved torch's default generator"
    # the settings do not change how much of the stream a batch consumes
    c, e = Augmenter(224, 1.0, 0.0, seed=7), Augmenter(224, 0.5, 0.5, seed=7)
    c.draw(5), e.draw(5)
    assert torch.equal(c.generator.get_state(), e.generator.get_state())
    seeds = {stream_seed(s, r) for s in (0, 1, 2023, 2 ** 32 - 1) for r in (0, 1, 7, 2 ** 24 - 1)}
    assert len(seeds) == 16 and all(0 <= s < 2 ** 63 for s in seeds)
    assert stream_seed(2023, 0) != 2023
    for bad in (dict(crop_scale=0.0), dict(crop_scale=1.5), dict(flip_p=-0.1), dict(flip_p=1.1)):
        with pytest.raises(ValueError):
            Augmenter(224, **bad)
    with pytest.raises(ValueError):
        stream_seed(1, 2 ** 24)


def test_entry_point_is_declared_documented_exported_and_typed():
    from d2r_amd import _lib
    text = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+d2r_clip_cache_augment\s*\(([^)]*)\)\s*;", hdr)
    assert m, "d2r_clip_cache_augment is not declared in include/d2r_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert "d2r_clip_cache_augment" in comments and "d2r_clip_augment_desc" in hdr
    res, argtypes = _lib.SIGNATURES["d2r_clip_cache_augment"]
    assert res is _lib.i32 and len(argtypes) == len(args) == 11
    for a, t in zip(args, argtypes):
        if "*" in a:
            assert t is _lib.vp or issubclass(t, ctypes._Pointer), (a, t)
        else:
            assert t is {"int": _lib.i32, "int64_t": _lib.i64}[a.split()[-2]], (a, t)
    assert argtypes[4] == ctypes.POINTER(_lib.ClipAugmentDesc) and ctypes.sizeof(_lib.ClipAugmentDesc) == 32
    assert [f[0] for f in _lib.ClipAugmentDesc._fields_[:5]] == ["x0", "y0", "w", "h", "flip"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "d2r_clip_cache_augment")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Indices and boxes are checked on their host copies: these calls never reach a launch (the device pointers are dummies)."""
    from d2r_amd import image as I
    lib = I._lib.load()
    fake, S = 1 << 20, 16

    def call(idx, boxes, rows=5, cache=fake, h_aug=True, S=S, aug=fake):
        h = np.asarray(idx, np.int64)
        d = np.zeros((len(h), 8), np.int32)
        d[:, :5] = np.asarray(boxes, np.int32)
        hp = ctypes.cast(d.ctypes.data, ctypes.POINTER(I._lib.ClipAugmentDesc)) if h_aug else None
        rc = lib.d2r_clip_cache_augment(cache, rows, h.ctypes.data, fake, hp, aug, len(h), S, fake, fake, None)
        return rc, lib.d2r_last_error().decode()

    ok = (0, 0, S, S, 0)
    for idx in ([0, 5], [-1, 0]):
        rc, err = call(idx, [ok, ok])
        assert rc == -1 and "outside the 5 rows" in err, (idx, err)
    for box in ((-1, 0, 4, 4, 0), (0, -1, 4, 4, 0), (0, 0, 0, 4, 0), (0, 0, 4, 0, 0), (13, 0, 4, 4, 0), (0, 13, 4, 4, 0),
                (0, 0, S + 1, 1, 0), (2 ** 31 - 1, 0, 2, 1, 0)):
        rc, err = call([1, 2], [ok, box])
        assert rc == -1 and "sample 1" in err and "does not lie inside" in err, (box, err)
    for flip in (2, -1):
        rc, err = call([1], [(0, 0, 4, 4, flip)])
        assert rc == -1 and "flip" in err, err
    assert call([0], [ok], h_aug=False)[0] == -1 and call([0], [ok], aug=None)[0] == -1
    rc, err = call([0], [ok], cache=fake + 8)
    assert rc == -1 and "aligned" in err
    assert call([0], [(0, 0, 1, 1, 0)], S=0)[0] == -1 and call([0], [(0, 0, 1, 1, 0)], S=4097)[0] == -1


def test_flag_ranges_and_refusal_on_synthetic_data():
    from d2r_amd.run import build_parser, main
    p = build_parser()
    d = p.parse_args([])
    assert d.aug_crop_scale == 1.0 and d.aug_flip == 0.0
    a = p.parse_args(["--aug_crop_scale", "0.08", "--aug_flip", "0.5"])
    assert a.aug_crop_scale == 0.08 and a.aug_flip == 0.5
    assert p.parse_args(["--aug_crop_scale", "1", "--aug_flip", "1"]).aug_flip == 1.0
    assert p.parse_args(["--aug_flip", "0"]).aug_flip == 0.0
    for bad in (["--aug_crop_scale", "0"], ["--aug_crop_scale", "-0.5"], ["--aug_crop_scale", "1.01"], ["--aug_crop_scale", "nan"],
                ["--aug_flip", "-0.01"], ["--aug_flip", "1.5"], ["--aug_flip", "nan"], ["--aug_flip", "half"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for flags in (["--aug_crop_scale", "0.5"], ["--aug_flip", "0.5"]):
        with pytest.raises(SystemExit, match="synthetic"):
            main(flags)


class _StubCache:
    device = torch.device("cpu")

    def gather(self, h_idx, idx, augmenter=None):
        return h_idx, augmenter


def test_cached_loader_passes_its_augmenter_to_every_gather():
    from d2r_amd.augment import Augmenter
    from d2r_amd.cache import CachedLoader
    from d2r_amd.data import make_loader
    aug = Augmenter(8, 0.5, 0.5)
    dl = make_loader(list(range(10)), 5, False, 0)
    with_aug, without = CachedLoader(dl, _StubCache(), aug), CachedLoader(dl, _StubCache())
    assert with_aug.augmenter is aug and without.augmenter is None
    assert all(a is aug for _, a in with_aug) and all(a is None for _, a in without)


class _StubSplit(torch.utils.data.Dataset):
    """What cache_loaders and run.main look at in an MSDDataset: a length and max_seq."""
    max_seq = 16

    def __init__(self, *args, **kwargs):
        pass

    def __len__(self):
        return 10

    def __getitem__(self, i):
        return i


class _StubCollate:
    S = 8

    def __call__(self, items):
        return items


def test_cache_loaders_hand_the_augmenter_to_the_named_split_only(monkeypatch):
    """cache_loaders with stubbed for_loader / prefill / free memory: every split is prefilled, and only the split that
    `augmenters` names gets the augmenter - the others' gathers are called without one."""
    from d2r_amd import cache as C
    from d2r_amd.augment import Augmenter
    from d2r_amd.data import make_loader
    prefilled = []
    monkeypatch.setattr(C.DeviceDatasetCache, "for_loader", staticmethod(lambda dl, device, split, logger=None: _StubCache()))
    monkeypatch.setattr(C, "prefill", lambda dl, cache, logger=None, split="": prefilled.append(split))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 40, 1 << 40))
    loaders = {split: make_loader(_StubSplit(), 5, split == "train", 0, drop_last=split == "train", collate_fn=_StubCollate())
               for split in ("train", "dev", "test")}
    aug = Augmenter(8, 0.5, 0.5)
    state = torch.get_rng_state()
    cached = C.cache_loaders(loaders, "cpu", augmenters={"train": aug})
    assert list(cached) == ["train", "dev", "test"] and prefilled == ["train", "dev", "test"]
    assert cached["train"].augmenter is aug and cached["dev"].augmenter is None and cached["test"].augmenter is None
    assert [a for _, a in cached["train"]] == [aug, aug]
    assert [a for _, a in cached["dev"]] == [None, None] and [a for _, a in cached["test"]] == [None, None]
    plain = C.cache_loaders(loaders, "cpu")
    assert all(dl.augmenter is None for dl in plain.values())
    torch.set_rng_state(state)  # the shuffled stub loader drew from the default generator


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


def test_run_gives_the_augmenter_to_the_cached_training_loader_or_to_the_trainer(monkeypatch, tmp_path, caplog):
    """run.main's wiring with the dataset, the model, the trainer and cache_loaders stubbed.  With the cache: augmenters is
    {"train": augmenter} and the trainer gets none (the cached loader augments).  Without it: the trainer gets the augmenter.
    Flags at their defaults: no augmenter anywhere.  --only_test: none is built, and a line says the flags are ignored."""
    import logging
    from d2r_amd import cache as C, data as D, modules as M, run, train as T
    from d2r_amd.augment import Augmenter, stream_seed
    for name in ("train.json", "dev.json", "test.json"):
        (tmp_path / name).write_text("[]")
    calls = []

    def cache_loaders(loaders, device, logger=None, augmenters=None):
        calls.append((list(loaders), augmenters))
        return loaders

    monkeypatch.setattr(C, "cache_loaders", cache_loaders)
    monkeypatch.setattr(D, "MSDDataset", _StubSplit)
    monkeypatch.setattr(M, "UnimoModelF", lambda **kwargs: object())
    monkeypatch.setattr(T, "MSDTrainer", _StubTrainer)
    monkeypatch.setattr(run, "set_seed", lambda seed: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--data_path", str(tmp_path), "--img_path", str(tmp_path), "--bert_name", str(tmp_path), "--device", "cpu", "--seed", "5",
            "--num_workers", "0"]
    on = ["--aug_crop_scale", "0.25", "--aug_flip", "0.75"]

    def main(extra):
        del calls[:], _StubTrainer.made[:]
        run.main(base + extra)
        assert len(_StubTrainer.made) == 1
        return _StubTrainer.made[0].kwargs

    def check(aug):
        assert isinstance(aug, Augmenter) and (aug.S, aug.crop_scale, aug.flip_p) == (224, 0.25, 0.75)
        assert aug.generator.initial_seed() == stream_seed(5, 0)

    kwargs = main(on + ["--cache_dataset", "device"])
    assert len(calls) == 1 and calls[0][0] == ["train", "dev", "test"] and list(calls[0][1]) == ["train"]
    check(calls[0][1]["train"])
    assert kwargs["augmenter"] is None

    kwargs = main(on)
    assert calls == []
    check(kwargs["augmenter"])

    kwargs = main(["--cache_dataset", "device"])
    assert len(calls) == 1 and calls[0][1] is None and kwargs["augmenter"] is None
    assert main([])["augmenter"] is None

    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        kwargs = main(on + ["--cache_dataset", "device", "--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert calls == [] and "augmenter" not in kwargs
    assert sum("--aug_crop_scale / --aug_flip are ignored with --only_test" in r.getMessage() for r in caplog.records) == 1
