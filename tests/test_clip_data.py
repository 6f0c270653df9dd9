"""Real-data layer on the host: the float64 restatement of Pillow's bicubic weights, the numpy two-pass resampler and the table of
the normalisation (d2r_amd.image) against Pillow and the processor fixture; MSDDataset / ClipCollate on a generated MVSA-style
directory; the argument checks of d2r_clip_preprocess (no launch happens); the CLI defaults."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from make_clip_golden import CASES, PIXEL_VALUE_CASES, expected_crop, fixture_image

from d2r_amd import image as I

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "cat", "dog", "is", "happy", "sad", "not", "a", "very", "good", "day",
         "##s", "!", ".", ","]
TEXTS = ["The cat is happy!", "a very sad dog.", "Not a good day", "dogs , cats", "the the the the the the the the the the the",
         "HAPPY Day", "zebra", ""]


def make_msd_dir(root, n=12, sizes=None):
    """An MVSA-style directory: train/dev/test.json, <id>.jpg images of mixed sizes, inf.png, a tiny BERT vocab.txt; the
    sample with id 'gone' has no image file.  Returns (data_path, img_path, vocab_dir)."""
    from PIL import Image
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    os.makedirs(os.path.join(root, "bert"), exist_ok=True)
    with open(os.path.join(root, "bert", "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    sizes = sizes or [(240 + 37 * i, 320 - 11 * i) for i in range(n)]
    samples = []
    for i in range(n):
        H, W = sizes[i % len(sizes)]
        Image.fromarray(fixture_image(100 + i, H, W)).save(os.path.join(root, "img", f"s{i}.jpg"), quality=90)
        samples.append({"id": f"s{i}", "text": TEXTS[i % len(TEXTS)], "emotion_label": i % 3})
    Image.fromarray(fixture_image(99, 250, 260)).save(os.path.join(root, "img", "inf.png"))
    for name, part in (("train.json", samples), ("dev.json", samples[: n // 2]), ("test.json", samples[n // 2:])):
        with open(os.path.join(root, name), "w") as f:
            json.dump(part, f)
    return root, os.path.join(root, "img"), os.path.join(root, "bert")


SIZE_PAIRS = [((480, 640), (224, 298)), ((640, 480), (298, 224)), ((80, 100), (224, 280)), ((224, 224), (224, 224)),
              ((225, 224), (224, 224)), ((300, 224), (224, 224)), ((160, 1200), (224, 1680)), ((1500, 2000), (224, 298)),
              ((517, 333), (347, 224)), ((1, 1), (5, 7)), ((3, 2), (224, 224)), ((2, 3), (1, 1)), ((999, 1601), (384, 615)),
              ((333, 517), (384, 596)), ((384, 385), (384, 384)), ((50, 4000), (224, 17920 // 10)), ((4000, 50), (17, 3)),
              ((257, 255), (256, 256)), ((100, 100), (101, 99)), ((100, 100), (33, 66)), ((37, 41), (41, 37)),
              ((720, 1280), (224, 398)), ((1080, 1920), (384, 682)), ((600, 800), (300, 400)), ((611, 613), (224, 224)),
              ((64, 64), (128, 128)), ((128, 128), (64, 64)), ((451, 97), (224, 41)), ((97, 451), (1041, 224)),
              ((2048, 1536), (298, 224))]


@pytest.mark.parametrize("src,dst", SIZE_PAIRS)
def test_resample_matches_pillow_bicubic(src, dst):
    """The float64 weights (Pillow's operation order) + the numpy fixed-point passes == Image.resize(BICUBIC), byte for byte."""
    from PIL import Image
    H, W = src
    img = fixture_image(H * 7 + W, H, W)
    ref = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BICUBIC))
    np.testing.assert_array_equal(I.resample(img, *dst), ref)


def test_weights_are_pillows_not_pairwise():
    """A pairwise (np.sum) normalisation flips integer weights for some sizes: the sequential sum is required."""
    bounds, k = I.bicubic_weights(1500, 224, 0, 224)
    assert bounds.dtype == np.int32 and k.dtype == np.int32 and k.shape == (224, 2 * 14 + 1)
    assert np.all(bounds[:, 1] <= k.shape[1]) and np.all(bounds[:, 0] + bounds[:, 1] <= 1500)
    assert np.all(np.abs(k.sum(1) - (1 << 22)) <= k.shape[1])  # weights of a pixel sum to one within rounding


def test_host_pipeline_reproduces_fixture():
    g = load_golden("clip_preprocess")
    table = I.normalize_table()
    for name, (H, W, S, seed) in CASES.items():
        crop, pv = I.reference_preprocess(fixture_image(seed, H, W), S, S, table)
        np.testing.assert_array_equal(crop, expected_crop(g, name), err_msg=name)
        if name in PIXEL_VALUE_CASES:
            assert pv.dtype == np.float32 and np.array_equal(pv, g["pixel_values_" + name]), name


def test_normalize_table_formula():
    """float32(float64(v) / 255), then (r - mean) / std in fp32 (the fixture's pixel values pin it); other formulas differ."""
    t = I.normalize_table()
    assert t.shape == (3, 256) and t.dtype == np.float32
    naive = ((np.arange(256)[None] / 255.0 - np.array(I.CLIP_MEAN)[:, None]) / np.array(I.CLIP_STD)[:, None]).astype(np.float32)
    assert not np.array_equal(t, naive)


def test_size_and_crop_rule():
    assert I.resize_shape(480, 640, 224) == (224, 298) and I.resize_shape(640, 480, 224) == (298, 224)
    assert I.resize_shape(517, 333, 224) == (347, 224) and I.resize_shape(224, 224, 224) == (224, 224)
    assert I.crop_origin(347, 224, 224) == (61, 0)
    with pytest.raises(ValueError):
        I.crop_origin(200, 300, 224)


def test_plan_batch_layout():
    imgs = [fixture_image(1, 480, 640), fixture_image(2, 1500, 2000), fixture_image(3, 80, 100)]
    pixels, desc, tab = I.plan_batch(imgs, 224, 224)
    assert pixels.dtype == np.uint8 and pixels.size == sum(im.size for im in imgs)
    assert desc.dtype.itemsize == ctypes.sizeof(I._lib.ClipImageDesc) == 72
    for d, im in zip(desc, imgs):
        o = int(d["src_offset"])
        np.testing.assert_array_equal(pixels[o:o + im.size], im.reshape(-1))
        assert (int(d["H"]), int(d["W"])) == im.shape[:2]
        xs = tab[d["bx"]:d["bx"] + 448].reshape(224, 2)
        ys = tab[d["by"]:d["by"] + 448].reshape(224, 2)
        assert xs[:, 0].min() >= 0 and (xs[:, 0] + xs[:, 1]).max() <= d["W"]
        assert ys[:, 0].min() == d["row0"] and (ys[:, 0] + ys[:, 1]).max() == d["row0"] + d["nrows"]
    ends = desc["ws_offset"] + desc["nrows"].astype(np.int64) * 224 * 3
    assert np.all(desc["ws_offset"][1:] >= ends[:-1]) and np.all(desc["ws_offset"] % 16 == 0)


def _tokenizer(vocab_dir):
    transformers = pytest.importorskip("transformers")
    return transformers.BertTokenizer.from_pretrained(vocab_dir, do_lower_case=True)


def test_msd_dataset_samples(tmp_path):
    from PIL import Image
    from d2r_amd.data import MSDDataset
    data, img, vocab = make_msd_dir(str(tmp_path), n=8)
    # the four kinds of file the loader meets: JPEG, PNG, grayscale, RGBA (the .jpg name does not decide the decoder)
    Image.fromarray(fixture_image(5, 90, 70)).save(os.path.join(img, "s1.jpg"), format="PNG")
    Image.fromarray(fixture_image(6, 90, 70)[:, :, 0]).save(os.path.join(img, "s2.jpg"), quality=95)
    rgba = np.concatenate([fixture_image(7, 60, 50), np.full((60, 50, 1), 9, np.uint8)], axis=2)
    Image.fromarray(rgba, "RGBA").save(os.path.join(img, "s3.jpg"), format="PNG")
    with open(os.path.join(data, "train.json")) as f:
        samples = json.load(f)
    samples[4]["id"] = "gone"
    with open(os.path.join(data, "train.json"), "w") as f:
        json.dump(samples, f)
    ds = MSDDataset(os.path.join(data, "train.json"), img, _tokenizer(vocab), max_seq=8)
    assert len(ds) == 8
    ids, mask, seg, img_mask, label, image = ds[0]  # "The cat is happy!"
    assert ids.tolist() == [2, 5, 6, 8, 9, 17, 3, 0] and mask.tolist() == [1] * 7 + [0]
    assert seg.tolist() == [0] * 8 and img_mask.tolist() == [1] * 50 and int(label) == 0
    assert all(t.dtype == torch.long for t in (ids, mask, seg, img_mask, label))
    assert image.dtype == np.uint8 and image.shape == (240, 320, 3)
    ids = ds[4][0]  # eleven words, truncated to max_seq - 2 between [CLS] and [SEP]
    assert ids.tolist() == [2] + [5] * 6 + [3]
    assert ds[7][0].tolist() == [2, 3] + [0] * 6 and ds[7][1].tolist() == [1, 1] + [0] * 6  # empty text
    assert ds[1][5].shape == (90, 70, 3)
    gray = ds[2][5]
    assert gray.shape == (90, 70, 3) and np.array_equal(gray[:, :, 0], gray[:, :, 1])
    np.testing.assert_array_equal(ds[3][5], rgba[:, :, :3])
    assert ds.fallbacks == 1  # ds[4] above: 'gone' has no image
    fb = ds[4][5]  # inf.png instead, counted
    assert ds.fallbacks == 2
    np.testing.assert_array_equal(fb, np.asarray(Image.open(os.path.join(img, "inf.png")).convert("RGB")))


def test_collate_layout(tmp_path):
    from d2r_amd.data import MSDDataset, make_loader
    data, img, vocab = make_msd_dir(str(tmp_path), n=6)
    ds = MSDDataset(os.path.join(data, "train.json"), img, _tokenizer(vocab), max_seq=16)
    dl = make_loader(ds, 4, False, 0, collate_fn=I.ClipCollate(224, 224))
    batch = next(iter(dl))
    ids, mask, seg, img_mask, labels, packed = batch
    assert ids.shape == (4, 16) and mask.shape == (4, 16) and seg.shape == (4, 16) and img_mask.shape == (4, 50)
    assert labels.tolist() == [0, 1, 2, 0] and isinstance(packed, I.PackedImages) and len(packed) == 4
    h_desc, h_tab = packed.host_parts()
    assert packed.pixels.dtype == torch.uint8 and h_tab.dtype == torch.int32
    assert packed.meta.numel() == 4 * 72 + 4 * h_tab.numel()
    for i, d in enumerate(h_desc):
        im = ds[i][5]
        o = int(d["src_offset"])
        assert np.array_equal(packed.pixels[o:o + im.size].numpy(), im.reshape(-1))
    pv = packed.to_pixel_values_cpu()
    assert pv.shape == (4, 3, 224, 224) and pv.dtype == torch.float32
    for i in range(4):
        assert torch.equal(pv[i], torch.from_numpy(I.reference_preprocess(ds[i][5], 224, 224)[1]))
    if torch.cuda.is_available():
        assert packed.pin_memory().pixels.is_pinned()


def test_preprocess_refuses_bad_descriptors_before_any_launch():
    """Every bound is checked on the host copies: these calls are refused with D2R_ERR_INVALID / _WORKSPACE and never reach a
    launch (the device pointers are dummies; nothing is dereferenced)."""
    lib = I._lib.load()
    pixels, desc, tab = I.plan_batch([fixture_image(1, 480, 640), fixture_image(2, 80, 100)], 224, 224)
    fake = 1 << 20

    def run(d, t=tab, src_bytes=pixels.size, ws=None, S=224):
        hd = ctypes.cast(d.ctypes.data, ctypes.POINTER(I._lib.ClipImageDesc))
        need = lib.d2r_clip_preprocess_ws_bytes(hd, len(d), S)
        rc = lib.d2r_clip_preprocess(fake, src_bytes, hd, fake, len(d), S, t.ctypes.data, fake, t.size, fake, fake, fake,
                                     need if ws is None else ws, None)
        return rc, lib.d2r_last_error().decode()

    assert lib.d2r_clip_preprocess_ws_bytes(ctypes.cast(desc.ctypes.data, ctypes.POINTER(I._lib.ClipImageDesc)), 2, 224) == \
        int(desc["ws_offset"][1]) + int(desc["nrows"][1]) * 224 * 3
    cases = []
    d = desc.copy(); d[1]["src_offset"] += 1; cases.append((d, "outside the"))
    d = desc.copy(); d[0]["left"] = d[0]["rw"] - 223; cases.append((d, "does not fit"))
    d = desc.copy(); d[0]["rh"] = 200; cases.append((d, "does not fit"))
    d = desc.copy(); d[0]["nrows"] += 1; cases.append((d, "source rows"))
    d = desc.copy(); d[1]["cy"] = tab.size - 10; cases.append((d, "table span"))
    d = desc.copy(); d[1]["ws_offset"] = 0; cases.append((d, "overlaps"))
    d = desc.copy(); d[0]["kx"] = 2; cases.append((d, "taps"))
    for d, msg in cases:
        rc, err = run(d)
        assert rc == -1 and msg in err, (rc, err)
    t = tab.copy(); t[desc[0]["bx"] + 2 * 5] = 639  # a column's support past the right edge
    rc, err = run(desc, t)
    assert rc == -1 and "column 5" in err
    t = tab.copy(); t[desc[1]["by"] + 2 * 7] = -1
    rc, err = run(desc, t)
    assert rc == -1 and "row 7" in err
    rc, err = run(desc, ws=int(desc["ws_offset"][1]) + 100)
    assert rc == -3 and "workspace" in err
    rc, err = run(desc, src_bytes=pixels.size - 1)
    assert rc == -1


def test_processor_settings(tmp_path):
    cfg = {"crop_size": {"height": 336, "width": 336}, "size": {"shortest_edge": 336}, "do_resize": True, "do_center_crop": True,
           "do_rescale": True, "do_normalize": True, "do_convert_rgb": True, "resample": 3, "rescale_factor": 0.00392156862745098,
           "image_mean": [0.5, 0.5, 0.5], "image_std": [0.25, 0.25, 0.25]}
    path = tmp_path / "preprocessor_config.json"
    path.write_text(json.dumps(cfg))
    assert I.processor_settings(str(tmp_path)) == (336, 336, (0.5,) * 3, (0.25,) * 3, 1 / 255)
    for key, bad in (("resample", 2), ("do_center_crop", False), ("do_normalize", False), ("size", {"height": 3, "width": 3}),
                     ("crop_size", {"height": 400, "width": 400})):
        path.write_text(json.dumps(dict(cfg, **{key: bad})))
        with pytest.raises(ValueError):
            I.processor_settings(str(tmp_path))


def test_cli_defaults_select_the_synthetic_path(tmp_path):
    from d2r_amd.run import build_parser, dataset_files
    a = build_parser().parse_args([])
    assert a.data_path is None and a.img_path is None and a.pretrained is False
    a = build_parser().parse_args(["--data_path", "d", "--img_path", "i", "--pretrained"])
    assert (a.data_path, a.img_path, a.pretrained) == ("d", "i", True)
    for name in ("train.json", "valid.json", "test.json"):  # HFM names its dev split valid.json
        (tmp_path / name).write_text("[]")
    assert dataset_files(str(tmp_path))[1].endswith("valid.json")
    (tmp_path / "test.json").unlink()
    with pytest.raises(SystemExit):
        dataset_files(str(tmp_path))
