"""--cache_dataset device on the MI355X.  Every comparison is exact: the uint8 crops d2r_clip_preprocess_u8 writes against
image.reference_preprocess, the pixel values d2r_clip_cache_gather builds against d2r_clip_preprocess, d2r_gather_rows against
index_select, the batches of CachedLoader against the plain loader's over three epochs in both --image_decode modes, and the
weights and dev metrics of a training run with the cache against the same run without (dropout on)."""
import json
import logging
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from make_clip_golden import fixture_image
from test_clip_data import make_msd_dir

from d2r_amd import D2RError
from d2r_amd import image as I

pytestmark = pytest.mark.gpu

GUARD = 4096
N = 11  # samples of the generated training split: batches of 4 end in a short one


def make_dir(root):
    """make_msd_dir's MVSA-style directory with the kinds of file a real image set holds: landscape and portrait JPEGs of mixed
    sizes, one smaller than the crop (upscaled), one progressive JPEG, one grayscale JPEG, one PNG, and a sample without a file
    (inf.png stands in)."""
    from PIL import Image
    sizes = [(240, 320), (431, 277), (80, 100), (300, 224), (517, 333), (224, 224), (160, 600), (333, 517), (250, 260), (97, 451),
             (611, 613)]
    data, img, vocab = make_msd_dir(str(root), n=N, sizes=sizes)
    Image.fromarray(fixture_image(5, 312, 290)).save(os.path.join(img, "s1.jpg"), quality=85, progressive=True)
    Image.fromarray(fixture_image(6, 290, 370)[:, :, 0]).save(os.path.join(img, "s4.jpg"), quality=92)
    Image.fromarray(fixture_image(7, 190, 275)).save(os.path.join(img, "s6.jpg"), format="PNG")
    for name in ("train.json", "dev.json", "test.json"):
        with open(os.path.join(data, name)) as f:
            samples = json.load(f)
        for s in samples:
            if s["id"] == "s8":
                s["id"] = "gone"
        with open(os.path.join(data, name), "w") as f:
            json.dump(samples, f)
    return data, img, vocab


def _tokenizer(vocab):
    transformers = pytest.importorskip("transformers")
    return transformers.BertTokenizer.from_pretrained(vocab, do_lower_case=True)


def _images(tmp_path):
    from d2r_amd.data import MSDDataset
    data, img, vocab = make_dir(tmp_path)
    ds = MSDDataset(os.path.join(data, "train.json"), img, _tokenizer(vocab), max_seq=16)
    images = [ds.load_image(name) for name in ds.imgs]
    assert ds.fallbacks == 1 and len({im.shape for im in images}) >= 10
    assert any(im.shape[0] > im.shape[1] for im in images) and any(im.shape[0] < im.shape[1] for im in images)
    return images


def _on_device(images, S, dev):
    packed = I.PackedImages.from_images(images, S, S)
    h_desc, h_tab = packed.host_parts()
    nd = len(images) * I.DESC_DTYPE.itemsize
    meta = packed.meta.to(dev)
    return packed.pixels.to(dev), h_desc, meta[:nd], h_tab, meta[nd:].view(torch.int32)


def _guarded_cache(rows, S, dev, fill=0xA5):
    rb = I.cache_row_bytes(S)
    buf = torch.full((rows * rb + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + rows * rb].view(rows, rb)


@pytest.mark.parametrize("S", [224, 30, 31])
def test_preprocess_u8_writes_the_reference_crops_into_the_named_rows_only(gpu, tmp_path, S):
    images = _images(tmp_path)
    B, rows = len(images), len(images) + 4
    args = _on_device(images, S, gpu)
    h_slots = torch.tensor([(7 * b + 3) % rows for b in range(B)], dtype=torch.int64)
    assert len(set(h_slots.tolist())) == B
    runs = []
    for _ in range(2):
        buf, cache = _guarded_cache(rows, S, gpu)
        I.clip_preprocess_u8(*args, S, cache, h_slots, h_slots.to(gpu))
        torch.cuda.synchronize()
        runs.append(buf.cpu())
    assert torch.equal(runs[0], runs[1]), "a second run differs"
    buf = runs[0]
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all()), "write outside the cache"
    rb, n = I.cache_row_bytes(S), 3 * S * S
    got = buf[GUARD:-GUARD].view(rows, rb).numpy()
    for b, im in enumerate(images):
        crop, _ = I.reference_preprocess(im, S, S)
        row = got[int(h_slots[b])]
        np.testing.assert_array_equal(row[:n].reshape(3, S, S), crop.transpose(2, 0, 1), err_msg=f"image {b} {im.shape}")
        assert (row[n:] == 0xA5).all(), "the row's padding was written"
    for r in set(range(rows)) - set(h_slots.tolist()):
        assert (got[r] == 0xA5).all(), f"row {r} was not named"


def test_preprocess_u8_refused_calls_write_nothing(gpu, tmp_path):
    S = 30
    images = _images(tmp_path)[:4]
    args = _on_device(images, S, gpu)
    buf, cache = _guarded_cache(6, S, gpu)
    for slots in ([0, 1, 2, 6], [0, -1, 2, 3], [0, 3, 2, 3]):
        h = torch.tensor(slots, dtype=torch.int64)
        with pytest.raises(D2RError):
            I.clip_preprocess_u8(*args, S, cache, h, h.clamp(0, 5).to(gpu))
    d = args[1].copy()
    d[2]["row0"] = d[2]["row0"] + 1  # a descriptor check of d2r_clip_preprocess
    h = torch.arange(4, dtype=torch.int64)
    with pytest.raises(D2RError):
        I.clip_preprocess_u8(args[0], d, args[2], args[3], args[4], S, cache, h, h.to(gpu))
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a refused call wrote"
    I.clip_preprocess_u8(*args, S, cache, h, h.to(gpu))  # the same arguments, valid slots: accepted
    torch.cuda.synchronize()
    assert not bool((cache[:4, :3 * S * S] == 0xA5).all())


@pytest.mark.parametrize("S", [224, 30, 31])
def test_cache_gather_equals_clip_preprocess_under_a_permutation_with_repeats(gpu, tmp_path, S):
    images = _images(tmp_path)
    B = len(images)
    args = _on_device(images, S, gpu)
    lut = torch.from_numpy(I.normalize_table()).to(gpu)
    want = I.clip_preprocess(*args, S, lut)
    cache = torch.zeros(B, I.cache_row_bytes(S), dtype=torch.uint8, device=gpu)
    h = torch.arange(B, dtype=torch.int64)
    I.clip_preprocess_u8(*args, S, cache, h, h.to(gpu))
    h_idx = torch.tensor([3, 0, 10, 3, 3, 7, 1, 9, 2, 10, 5, 4, 6, 8, 0], dtype=torch.int64)
    n_out = h_idx.numel() * 3 * S * S
    out_buf = torch.full((n_out + 2 * GUARD,), float("nan"), device=gpu)
    out = I.clip_cache_gather(cache, h_idx, h_idx.to(gpu), S, lut, out=out_buf[GUARD:GUARD + n_out])
    torch.cuda.synchronize()
    assert torch.equal(out.view(-1, 3, S, S), want[h_idx.to(gpu)])
    assert bool(torch.isnan(out_buf[:GUARD]).all()) and bool(torch.isnan(out_buf[GUARD + n_out:]).all()), "write outside out"
    assert torch.isfinite(out).all()
    # odd batch offsets and an unaligned out (S odd: image bases are not 16-byte aligned either)
    out2 = I.clip_cache_gather(cache, h_idx[:3], h_idx[:3].to(gpu), S, lut, out=out_buf[GUARD + 1:GUARD + 1 + 9 * S * S])
    torch.cuda.synchronize()
    assert torch.equal(out2.view(3, 3, S, S), want[h_idx[:3].to(gpu)])
    # refused before the launch
    out_buf.fill_(7.0)
    for bad in ([0, B], [-1, 2]):
        hb = torch.tensor(bad, dtype=torch.int64)
        with pytest.raises(D2RError):
            I.clip_cache_gather(cache, hb, hb.clamp(0, B - 1).to(gpu), S, lut, out=out_buf[GUARD:GUARD + 2 * 3 * S * S])
    torch.cuda.synchronize()
    assert bool((out_buf == 7.0).all())


@pytest.mark.parametrize("offset", [0, 8, 4, 1], ids=lambda o: f"base+{o}")
@pytest.mark.parametrize("width", [8, 24, 1024])
def test_gather_rows_equals_index_select(gpu, width, offset):
    rows, B = 53, 37
    g = torch.Generator().manual_seed(width + offset)
    base = torch.randint(0, 256, (rows * width + 64,), dtype=torch.uint8, generator=g).to(gpu)
    src = base[offset:offset + rows * width].view(rows, width)
    h_idx = torch.randint(0, rows, (B,), generator=g)
    h_idx[:3] = torch.tensor([rows - 1, 0, rows - 1])
    idx = h_idx.to(gpu)
    dst_buf = torch.full((B * width + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=gpu)
    out = I.gather_rows(src, h_idx, idx, out=dst_buf[GUARD + offset:GUARD + offset + B * width].view(B, width))
    torch.cuda.synchronize()
    assert torch.equal(out, src.index_select(0, idx))
    assert bool((dst_buf[:GUARD + offset] == 0x5A).all()) and bool((dst_buf[GUARD + offset + B * width:] == 0x5A).all())
    with pytest.raises(D2RError):
        I.gather_rows(src, torch.tensor([rows]), idx[:1])


def test_gather_rows_of_token_tensors(gpu):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 30000, (40, 128), generator=g).to(gpu)
    labels = torch.randint(0, 3, (40,), generator=g).to(gpu)
    h_idx = torch.randperm(40, generator=g)[:32]
    idx = h_idx.to(gpu)
    a, b = I.gather_rows(ids, h_idx, idx), I.gather_rows(labels, h_idx, idx)
    assert a.shape == (32, 128) and b.shape == (32,) and a.dtype == b.dtype == torch.int64
    assert torch.equal(a, ids[idx]) and torch.equal(b, labels[idx])


def _host_decoded(ds):
    """How many of the dataset's images the device decoder does not take (d2r_amd.jpeg.route; a missing file becomes inf.png)."""
    from d2r_amd.jpeg import route
    n = 0
    for name in ds.imgs:
        path = os.path.join(ds.img_path, name)
        if not os.path.exists(path):
            path = os.path.join(ds.img_path, "inf.png")
        with open(path, "rb") as f:
            n += route(f.read())[0] is None
    return n


class _Catch(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, rec):
        self.lines.append(rec.getMessage())


def _logger(name):
    logger = logging.getLogger(name)
    catch = _Catch()
    logger.addHandler(catch)
    logger.setLevel(logging.INFO)
    return logger, catch


def _loader(data, img, tok, split, shuffle, decode, S=224, workers=2, max_seq=16):
    from d2r_amd.data import MSDDataset, make_loader
    ds = MSDDataset(os.path.join(data, split + ".json"), img, tok, max_seq=max_seq, image_decode=decode)
    return make_loader(ds, 4, shuffle, workers, drop_last=shuffle, collate_fn=I.ClipCollate(S, S, image_decode=decode))


def _plain_to_device(batch, dev):
    return tuple(t.to(dev, non_blocking=True) if isinstance(t, torch.Tensor) else t.to_pixel_values(dev) for t in batch)


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled_drop_last", "sequential_short_last"])
@pytest.mark.parametrize("decode", ["host", "device"])
def test_cached_loader_yields_the_plain_loaders_batches(gpu, tmp_path, monkeypatch, decode, shuffle):
    from d2r_amd.cache import CachedBatch, CachedLoader, DeviceDatasetCache, prefill, release_workers
    from d2r_amd.data import MSDDataset
    from d2r_amd.train import MSDTrainer
    data, img, vocab = make_dir(tmp_path)
    tok = _tokenizer(vocab)
    plain = _loader(data, img, tok, "train", shuffle, decode)
    torch.manual_seed(9)
    want = []
    for epoch in range(3):
        want.append([tuple(t.cpu() for t in _plain_to_device(b, gpu)) for b in plain])
    after_plain = torch.get_rng_state()
    release_workers(plain)
    assert [len(e) for e in want] == [2 if shuffle else 3] * 3 and (shuffle or want[0][-1][0].shape[0] == 3)

    wrapped = _loader(data, img, tok, "train", shuffle, decode)
    next(iter(wrapped))  # the loader to be replaced already holds persistent workers
    assert len(multiprocessing.active_children()) >= 2
    logger, catch = _logger(f"cache-test-{decode}-{shuffle}")
    cache = DeviceDatasetCache.for_loader(wrapped, gpu, "train", logger)
    torch.manual_seed(9)
    before = torch.get_rng_state()
    prefill(wrapped, cache, logger, "train")
    assert torch.equal(torch.get_rng_state(), before), "the prefill moved the default generator"
    assert not multiprocessing.active_children(), "worker processes survived the prefill"
    assert cache.fallbacks == 1 and cache.nbytes == N * (150528 + 3 * 8 * 16 + 8)
    log = "\n".join(catch.lines)
    n_host = N if decode == "host" else _host_decoded(wrapped.dataset)
    assert decode == "host" or 3 <= n_host <= N - 5  # the progressive JPEG, the PNG and inf.png at least; most files on the device
    assert "train split prefill images: %d decoded on the device, %d on the host" % (N - n_host, n_host) in log, log
    assert "0 device decode(s) with corrupt data" in log
    assert "train split cached on the device: 11 images, 1 inf.png fallback(s), %d bytes held, prefill" % cache.nbytes in log

    def boom(self, name):
        raise AssertionError("an image was decoded after the prefill")

    monkeypatch.setattr(MSDDataset, "load_image", boom)
    cached = CachedLoader(wrapped, cache)
    trainer = MSDTrainer.__new__(MSDTrainer)  # only its _to_device hook is used
    trainer.args = type("A", (), {"device": str(gpu)})()
    assert len(cached) == len(plain)
    for epoch in range(3):
        got = list(cached)
        assert len(got) == len(want[epoch])
        for g, w in zip(got, want[epoch]):
            assert isinstance(g, CachedBatch) and len(g) == 6 and g.cached_images == w[0].shape[0]
            moved = trainer._to_device(g)
            for a, b, c in zip(g, moved, w):
                assert a.is_cuda and b.data_ptr() == a.data_ptr()
                assert a.dtype == c.dtype and a.shape == c.shape and torch.equal(a.cpu(), c)
    assert torch.equal(torch.get_rng_state(), after_plain), "CachedLoader consumed the default generator differently"
    assert not multiprocessing.active_children()


def _small_model(dtype, dev):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    tc = TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    vc = VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)
    args = default_args(DR_step=3, compute_dtype=dtype, device=str(dev), num_epochs=2, batch_size=4, warmup_ratio=0.0,
                        save_path=None, lr=1e-4)
    return M.UnimoModelF(args, vc, tc), args


@pytest.mark.parametrize("dtype,decode", [(torch.bfloat16, "device"), (torch.float32, "host")], ids=["bf16_device_decode", "fp32_host_decode"])
def test_training_with_the_cache_is_bit_identical_to_training_without(gpu, tmp_path, dtype, decode):
    """Two epochs of MSDTrainer with dropout on, with persistent loader workers: the same seed gives the same weights and the same
    dev metrics whether the batches come from the loaders or from the device cache (leans on the step's bit reproducibility, which
    test_gpu_trainer asserts)."""
    from d2r_amd.cache import cache_loaders
    from d2r_amd.train import MSDTrainer
    data, img, vocab = make_dir(tmp_path)
    tok = _tokenizer(vocab)
    results = []
    for use_cache in (False, True):
        torch.manual_seed(31)
        torch.cuda.manual_seed_all(31)
        model, args = _small_model(dtype, gpu)
        logger, catch = _logger(f"cache-trainer-{dtype}-{use_cache}")
        loaders = {"train": _loader(data, img, tok, "train", True, decode, S=64),
                   "dev": _loader(data, img, tok, "dev", False, decode, S=64)}
        if use_cache:
            loaders = cache_loaders(loaders, str(gpu), logger)
        tr = MSDTrainer(train_data=loaders["train"], dev_data=loaders["dev"], test_data=None, model=model, args=args, logger=logger,
                        writer=None)
        tr.train(None, None)
        torch.cuda.synchronize()
        metrics = [l for l in catch.lines if l.startswith("  ") and " = " in l and not l.startswith("  Num") and "Batch size" not in l
                   and "Learning rate" not in l and "Evaluate begin" not in l]
        losses = [l.split("samples/s")[0] for l in catch.lines if l.startswith("step ")]
        results.append((tr.store.flat_w.clone(), metrics, losses, catch.lines))
        if not use_cache:
            from d2r_amd.cache import release_workers
            for dl in loaders.values():
                release_workers(dl)
    (w0, m0, l0, _), (w1, m1, l1, lines) = results
    assert len(m0) == 2 * 6 and any("f_score" in l for l in m0) and any("loss" in l for l in m0), m0
    assert len(l0) == 2 and l0 == l1, (l0, l1)
    assert m0 == m1, (m0, m1)
    assert torch.equal(w0, w1), "the cached run's weights differ in %d elements" % int((w0 != w1).sum())
    assert sum("8 images from the device cache" in l for l in lines) == 2, [l for l in lines if "images" in l]


def _cli(args, tmp_path, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "d2r_amd.run", *args,
                        "--save_path", str(tmp_path / "out") + "/"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


def test_cli_trains_from_the_device_cache(gpu, tmp_path):
    pytest.importorskip("transformers")
    data, img, vocab = make_dir(tmp_path / "ds")
    common = ["--data_path", data, "--img_path", img, "--bert_name", vocab, "--encoder_layers", "1", "--batch_size", "4",
              "--num_workers", "2", "--max_seq", "32", "--cache_dataset", "device"]
    log = _cli(common + ["--num_epochs", "2", "--image_decode", "device"], tmp_path)
    for split, n in (("train", 11), ("dev", 5), ("test", 6)):
        assert f"{split} split cached on the device: {n} images" in log, log[-4000:]
        assert f"{split} split prefill images:" in log
    assert "epoch 1 images: 8 images from the device cache" in log and "epoch 2 images: 8 images from the device cache" in log
    assert "Dev Eval results" in log and "Test Eval results" in log and "decoded on the device" in log
    # a single prediction pass gains nothing from a cache: logged and ignored
    log = _cli(common + ["--only_test", "--load_path", str(tmp_path / "out" / "best_model.pth")], tmp_path)
    assert "--cache_dataset device is ignored with --only_test" in log and "cached on the device" not in log
    assert "Running prediction" in log
