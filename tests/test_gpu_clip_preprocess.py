"""d2r_clip_preprocess on the MI355X: bit-identical to CLIPImageProcessor (tests/golden/clip_preprocess.npz) one image per call,
as mixed-size batches and as a batch of 32; nothing written outside the output and the workspace; refused calls write nothing;
the real-data loader path through the model and through the CLI."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from make_clip_golden import CASES, PIXEL_VALUE_CASES, expected_crop, fixture_image
from test_clip_data import make_msd_dir

from d2r_amd import D2RError
from d2r_amd import image as I

pytestmark = pytest.mark.gpu

GUARD = 4096


def _expected(g, names):
    t = I.normalize_table()
    return np.stack([np.stack([t[c][expected_crop(g, n)[:, :, c]] for c in range(3)]) for n in names])


def _run(names, dev, guard=False):
    """Preprocess the fixture images `names` (one S) in one call; with guard=True, output and workspace sit inside NaN / 0xA5
    guard bands that are checked afterwards."""
    S = CASES[names[0]][2]
    packed = I.PackedImages.from_images([fixture_image(CASES[n][3], CASES[n][0], CASES[n][1]) for n in names], S, S)
    h_desc, h_tab = packed.host_parts()
    pixels, meta = packed.pixels.to(dev), packed.meta.to(dev)
    nd = len(names) * I.DESC_DTYPE.itemsize
    lut = torch.from_numpy(I.normalize_table()).to(dev)
    if not guard:
        out = I.clip_preprocess(pixels, h_desc, meta[:nd], h_tab, meta[nd:].view(torch.int32), S, lut)
        torch.cuda.synchronize()
        return out.cpu()
    n_out = len(names) * 3 * S * S
    out_buf = torch.full((n_out + 2 * GUARD,), float("nan"), device=dev)
    need = int(I._lib.load().d2r_clip_preprocess_ws_bytes(
        I.C.cast(h_desc.ctypes.data, I.C.POINTER(I._lib.ClipImageDesc)), len(names), S))
    ws_buf = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    I.clip_preprocess(pixels, h_desc, meta[:nd], h_tab, meta[nd:].view(torch.int32), S, lut, out=out_buf[GUARD:GUARD + n_out],
                      ws=ws_buf[GUARD:GUARD + need])
    torch.cuda.synchronize()
    o, w = out_buf.cpu(), ws_buf.cpu()
    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[GUARD + n_out:]).all(), "write outside the output"
    assert (w[:GUARD] == 0xA5).all() and (w[GUARD + need:] == 0xA5).all(), "write outside the workspace"
    return o[GUARD:GUARD + n_out].view(len(names), 3, S, S)


@pytest.mark.parametrize("name", list(CASES))
def test_one_image_per_call_is_bit_identical(gpu, name):
    g = load_golden("clip_preprocess")
    out = _run([name], gpu).numpy()
    np.testing.assert_array_equal(out, _expected(g, [name]))
    if name in PIXEL_VALUE_CASES:
        assert np.array_equal(out[0], g["pixel_values_" + name])


@pytest.mark.parametrize("S", [224, 384])
def test_mixed_batch_is_bit_identical(gpu, S):
    g = load_golden("clip_preprocess")
    names = [n for n, c in CASES.items() if c[2] == S]
    out = _run(names, gpu, guard=True).numpy()
    np.testing.assert_array_equal(out, _expected(g, names))


def test_batch_of_32_is_bit_identical(gpu):
    g = load_golden("clip_preprocess")
    pool = [n for n, c in CASES.items() if c[2] == 224]
    names = [pool[(7 * i) % len(pool)] for i in range(32)]
    out = _run(names, gpu, guard=True).numpy()
    np.testing.assert_array_equal(out, _expected(g, names))


def test_refused_calls_write_nothing(gpu):
    S = 224
    imgs = [fixture_image(1, 480, 640), fixture_image(2, 80, 100)]
    pixels_h, desc, tab_h = I.plan_batch(imgs, S, S)
    pixels = torch.from_numpy(pixels_h).to(gpu)
    lut = torch.from_numpy(I.normalize_table()).to(gpu)
    h_tab = torch.from_numpy(tab_h)
    tab = h_tab.to(gpu)
    need = int(desc["ws_offset"][1]) + int(desc["nrows"][1]) * S * 3
    out = torch.full((2, 3, S, S), 7.0, device=gpu)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=gpu)

    def call(d, ws_t=ws, h_t=h_tab):
        dd = torch.from_numpy(d.view(np.uint8).copy()).to(gpu)
        I.clip_preprocess(pixels, d, dd, h_t, tab, S, lut, out=out, ws=ws_t)

    bad = []
    d = desc.copy(); d[1]["src_offset"] = pixels_h.size; bad.append(d)
    d = desc.copy(); d[0]["top"] = 1; bad.append(d)              # crop past the resized image's bottom (rh == S)
    d = desc.copy(); d[0]["row0"] = d[0]["row0"] + 1; bad.append(d)
    d = desc.copy(); d[1]["bx"] = tab_h.size; bad.append(d)
    for d in bad:
        with pytest.raises(D2RError):
            call(d)
    t = tab_h.copy(); t[desc[1]["bx"] + 1] = 0  # image 1's first column gets no taps
    with pytest.raises(D2RError):
        call(desc, h_t=torch.from_numpy(t))
    with pytest.raises(D2RError, match="workspace"):
        call(desc, ws_t=ws[:need - 1])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all()), "a refused call wrote"
    call(desc)  # the same arguments unmodified are accepted
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def _model(dev, S=224):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    torch.manual_seed(3)
    tc = TextConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=2, image_size=S, patch_size=32)
    model = M.UnimoModelF(default_args(device=str(dev)), vc, tc).to(dev)
    model.set_compute_dtype(torch.float32).eval()
    return model


def test_loader_batch_logits_match_cpu_preprocessing(gpu, tmp_path):
    """A real-data batch (JPEGs of mixed sizes through MSDDataset + ClipCollate + pinning) gives the same images and logits whether
    the preprocessing runs on the GPU (the trainer's path) or in numpy on the host."""
    transformers = pytest.importorskip("transformers")
    from d2r_amd.data import MSDDataset, make_loader
    from d2r_amd.params import ParamStore
    from d2r_amd.train import MSDTrainer
    data, img, vocab = make_msd_dir(str(tmp_path), n=8)
    tok = transformers.BertTokenizer.from_pretrained(vocab, do_lower_case=True)
    dl = make_loader(MSDDataset(os.path.join(data, "train.json"), img, tok, max_seq=32), 8, False, 2,
                     collate_fn=I.ClipCollate(224, 224))
    batch = next(iter(dl))
    assert batch[5].pixels.is_pinned()
    model = _model(gpu)
    ParamStore(model, torch.float32)
    trainer = MSDTrainer.__new__(MSDTrainer)  # only its _to_device hook is used
    trainer.args = types.SimpleNamespace(device=str(gpu))
    on_gpu = trainer._to_device(batch)
    on_cpu = tuple(t.to(gpu) for t in batch[:5]) + (batch[5].to_pixel_values_cpu().to(gpu),)
    assert torch.equal(on_gpu[5], on_cpu[5])
    with torch.no_grad():
        outs = [model(input_ids=b[0], attention_mask=b[1], token_type_ids=b[2], labels=b[4], images=b[5]) for b in (on_gpu, on_cpu)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0][1], outs[1][1]) and torch.isfinite(outs[0][1]).all()


def _cli(args, tmp_path, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "d2r_amd.run", *args,
                        "--save_path", str(tmp_path / "out") + "/"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


def test_cli_trains_on_an_mvsa_directory(gpu, tmp_path):
    pytest.importorskip("transformers")
    data, img, vocab = make_msd_dir(str(tmp_path / "ds"), n=12)
    log = _cli(["--data_path", data, "--img_path", img, "--bert_name", vocab, "--num_epochs", "1", "--encoder_layers", "2",
                "--batch_size", "4", "--num_workers", "2", "--max_seq", "32"], tmp_path)
    assert "Dev Eval results" in log and "Test Eval results" in log and "f_score" in log


def test_cli_pretrained_ingests_every_key(gpu, tmp_path):
    transformers = pytest.importorskip("transformers")
    data, img, vocab = make_msd_dir(str(tmp_path / "ds"), n=8)
    torch.manual_seed(0)
    bert_dir, clip_dir = str(tmp_path / "bert"), str(tmp_path / "clip")
    tok = transformers.BertTokenizer.from_pretrained(vocab, do_lower_case=True)
    transformers.BertModel(transformers.BertConfig(vocab_size=len(tok), num_hidden_layers=2)).save_pretrained(bert_dir)
    tok.save_pretrained(bert_dir)
    ccfg = transformers.CLIPConfig(vision_config=dict(num_hidden_layers=2, image_size=224, patch_size=32),
                                   text_config=dict(num_hidden_layers=1, hidden_size=32, intermediate_size=37, num_attention_heads=2,
                                                    vocab_size=99), projection_dim=32)
    transformers.CLIPModel(ccfg).save_pretrained(clip_dir)
    transformers.CLIPImageProcessor().save_pretrained(clip_dir)
    log = _cli(["--data_path", data, "--img_path", img, "--bert_name", bert_dir, "--vit_name", clip_dir, "--pretrained",
                "--num_epochs", "1", "--batch_size", "4", "--num_workers", "0", "--max_seq", "32"], tmp_path)
    assert "Test Eval results" in log
