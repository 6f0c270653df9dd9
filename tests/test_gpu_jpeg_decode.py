"""d2r_jpeg_decode on the MI355X: bit-identical to Pillow (``np.asarray(Image.open(p).convert("RGB"))``) on the test_jpeg_host
matrix one image per call, as one mixed batch and as a batch of 32 images of 0.3-2 MP; nothing written outside the output, the
status array and the workspace; refused calls write nothing; a corrupted entropy segment sets its image's status and leaves the
other images bit-exact; --image_decode device gives the same pixel values and logits as the host decode, and the CLI runs."""
import os
import types

import numpy as np
import pytest
import torch

from test_clip_data import make_msd_dir
from test_gpu_clip_preprocess import _cli, _model
from test_jpeg_host import device_cases, encode, pillow_rgb

from d2r_amd import D2RError
from d2r_amd import jpeg as J

pytestmark = pytest.mark.gpu

GUARD = 4096


def _decode(datas, dev):
    """Decodes `datas` in one call with output, status and workspace inside guard bands that are checked afterwards: (list of
    uint8 [H, W, 3], status int32 [B], stats int32 [B, 2])."""
    infos = [J.parse(d) for d in datas]
    sizes = [i.H * i.W * 3 for i in infos]
    offsets = np.cumsum([0] + sizes)
    data, desc, segs, tab = J.plan_jpeg_batch(infos, offsets[:-1] + GUARD)
    B, total, need = len(infos), int(offsets[-1]), J.ws_bytes(desc)
    meta = J._meta(desc, segs, tab)
    dmeta = meta.to(dev)
    nd, ns = desc.nbytes, segs.nbytes
    dst = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.full((need + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.full((B + 128,), -7, dtype=torch.int32, device=dev)
    stats = torch.full((2 * B + 128,), -7, dtype=torch.int32, device=dev)
    J.jpeg_decode(torch.from_numpy(data).to(dev), desc, dmeta[:nd], segs, dmeta[nd:nd + ns], meta[nd + ns:].view(torch.int32),
                  dmeta[nd + ns:].view(torch.int32), dst[:total + GUARD], status=status[64:64 + B], stats=stats[64:64 + 2 * B],
                  ws=ws[GUARD:GUARD + need])
    torch.cuda.synchronize()
    o, w, s, st = dst.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy()
    assert (o[:GUARD] == 0xA5).all() and (o[GUARD + total:] == 0xA5).all(), "write outside the output"
    assert (w[:GUARD] == 0x5A).all() and (w[GUARD + need:] == 0x5A).all(), "write outside the workspace"
    assert (s[:64] == -7).all() and (s[64 + B:] == -7).all() and (st[:64] == -7).all() and (st[64 + 2 * B:] == -7).all()
    imgs = [o[GUARD + offsets[b]:GUARD + offsets[b + 1]].reshape(infos[b].H, infos[b].W, 3) for b in range(B)]
    return imgs, s[64:64 + B], st[64:64 + 2 * B].reshape(B, 2)


CASES = device_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_one_image_per_call_is_bit_identical_to_pillow(gpu, name):
    imgs, status, stats = _decode([CASES[name]], gpu)
    assert status[0] == 0
    np.testing.assert_array_equal(imgs[0], pillow_rgb(CASES[name]))
    assert stats[0, 0] >= 1


def test_mixed_batch_is_bit_identical(gpu):
    names = list(CASES)
    imgs, status, _ = _decode([CASES[n] for n in names], gpu)
    assert not status.any()
    for n, im in zip(names, imgs):
        np.testing.assert_array_equal(im, pillow_rgb(CASES[n]), err_msg=n)


def _sizes(n, seed):
    """n (H, W) pairs of 0.3-2 MP, aspect 3:4 .. 16:9 either way (the CLIP probe's sizes)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        mp = rng.uniform(0.3e6, 2.0e6)
        aspect = rng.uniform(0.75, 16 / 9)
        h = int(np.sqrt(mp / aspect))
        w = int(mp / h)
        out.append((h, w) if rng.integers(2) else (w, h))
    return out


def test_batch_of_32_large_images_is_bit_identical(gpu):
    datas = [encode(3000 + i, h, w, quality=90, subsampling=(2, 2, 1, 0)[i % 4], **({"optimize": True} if i % 5 == 0 else {}),
                    **({"restart_marker_rows": 2} if i % 7 == 0 else {})) for i, (h, w) in enumerate(_sizes(32, 5))]
    imgs, status, stats = _decode(datas, gpu)
    assert not status.any()
    for i, (d, im) in enumerate(zip(datas, imgs)):
        np.testing.assert_array_equal(im, pillow_rgb(d), err_msg=f"image {i}")
    print("sync rounds per image (max over workgroups):", stats[:, 0].tolist(), "boundary re-decodes:", stats[:, 1].tolist())


def test_refused_calls_write_nothing(gpu):
    infos = [J.parse(CASES["q90_420"]), J.parse(CASES["rst_blocks_422"])]
    sizes = [i.H * i.W * 3 for i in infos]
    data_h, desc, segs, tab_h = J.plan_jpeg_batch(infos, [0, sizes[0]])
    data = torch.from_numpy(data_h).to(gpu)
    h_tab = torch.from_numpy(tab_h)
    tab = h_tab.to(gpu)
    need = J.ws_bytes(desc)
    dst = torch.full((sum(sizes),), 7, dtype=torch.uint8, device=gpu)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=gpu)
    status = torch.full((2,), 99, dtype=torch.int32, device=gpu)

    def call(d, s=segs, ws_t=ws):
        J.jpeg_decode(data, d, torch.from_numpy(d.view(np.uint8).copy()).to(gpu), s, torch.from_numpy(s.view(np.uint8).copy()).to(gpu),
                      h_tab, tab, dst, status=status, ws=ws_t)

    bad = []
    d = desc.copy(); d[1]["dst_offset"] += 1; bad.append((d, segs))
    d = desc.copy(); d[0]["dc"][0] = tab_h.size; bad.append((d, segs))
    d = desc.copy(); d[1]["nseg"] -= 1; bad.append((d, segs))
    s = segs.copy(); s[-1]["bits"] += 64; bad.append((desc, s))
    for d, s in bad:
        with pytest.raises(D2RError):
            call(d, s)
    with pytest.raises(D2RError, match="workspace"):
        call(desc, ws_t=ws[:need - 1])
    for bad_status in (status[:1], status.to(torch.int64), status.cpu()):  # the library writes B int32 through the pointer
        with pytest.raises(ValueError):
            J.jpeg_decode(data, desc, torch.from_numpy(desc.view(np.uint8).copy()).to(gpu), segs,
                          torch.from_numpy(segs.view(np.uint8).copy()).to(gpu), h_tab, tab, dst, status=bad_status, ws=ws)
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((ws == 0x5A).all()) and bool((status == 99).all()), "a refused call wrote"
    call(desc)
    torch.cuda.synchronize()
    assert not bool(status.any())
    np.testing.assert_array_equal(dst[:sizes[0]].cpu().numpy().reshape(infos[0].H, infos[0].W, 3), pillow_rgb(CASES["q90_420"]))


def _corrupt(data: bytes) -> bytes:
    """`data` with 64 bytes in the middle of its largest restart segment replaced by 32 stuffed 0xFF bytes (FF 00): 256 one-bits,
    which no Huffman code of a JPEG table matches.  The markers are untouched, so the host accepts the file."""
    info = J.parse(data)
    sos = data.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    big = int(np.argmax([s.size for s in info.segments]))
    pos, seg = start, 0
    while seg < big:  # skip to the start of segment `big` in the stuffed bytes
        if data[pos] == 0xFF and 0xD0 <= data[pos + 1] <= 0xD7:
            seg += 1
            pos += 2
        else:
            pos += 1
    a = pos + info.segments[big].size // 2
    while data[a - 1] == 0xFF:
        a += 1
    out = data[:a] + b"\xff\x00" * 32 + data[a + 64:]
    assert J.route(out)[0] is not None and b"\xff\xd0" not in data[a:a + 66] and b"\xff\xd9" not in data[a:a + 66]
    return out


@pytest.mark.parametrize("restart", [False, True])
def test_corrupt_segment_sets_status_and_spares_the_batch(gpu, restart):
    kw = {"restart_marker_rows": 1} if restart else {}
    good = [encode(40 + i, 300 + 17 * i, 411 - 9 * i, quality=90, **kw) for i in range(3)]
    bad = _corrupt(encode(50, 640, 480, quality=95, **kw))
    imgs, status, _ = _decode([good[0], bad, good[1], good[2]], gpu)
    assert status[1] & J.STATUS_BAD_CODE and status[[0, 2, 3]].tolist() == [0, 0, 0]
    for g, im in zip(good, [imgs[0], imgs[2], imgs[3]]):
        np.testing.assert_array_equal(im, pillow_rgb(g))


def test_loader_device_decode_matches_host_decode(gpu, tmp_path):
    """The same MVSA-layout directory through MSDDataset(image_decode="host" / "device") + ClipCollate + the trainer's _to_device
    hook: identical pixel values and identical logits of one forward."""
    transformers = pytest.importorskip("transformers")
    from d2r_amd.data import MSDDataset, make_loader
    from d2r_amd.image import ClipCollate
    from d2r_amd.params import ParamStore
    from d2r_amd.train import MSDTrainer
    data, img, vocab = make_msd_dir(str(tmp_path), n=8)
    with open(os.path.join(img, "s3.jpg"), "wb") as f:  # one progressive file: decoded on the host inside a device batch
        f.write(encode(7, 260, 300, quality=90, progressive=True))
    tok = transformers.BertTokenizer.from_pretrained(vocab, do_lower_case=True)
    trainer = MSDTrainer.__new__(MSDTrainer)  # only its _to_device hook is used
    trainer.args = types.SimpleNamespace(device=str(gpu))
    batches = {}
    for mode in ("host", "device"):
        dl = make_loader(MSDDataset(os.path.join(data, "train.json"), img, tok, max_seq=32, image_decode=mode), 8, False, 2,
                         collate_fn=ClipCollate(224, 224))
        raw = next(iter(dl))
        batches[mode] = trainer._to_device(raw)
        if mode == "device":
            assert isinstance(raw[5], J.PackedJpegImages) and (raw[5].n_device, raw[5].n_host) == (7, 1)
            torch.cuda.synchronize()
            assert not raw[5].status.any()
    assert torch.equal(batches["host"][5], batches["device"][5])
    model = _model(gpu)
    ParamStore(model, torch.float32)
    with torch.no_grad():
        outs = [model(input_ids=b[0], attention_mask=b[1], token_type_ids=b[2], labels=b[4], images=b[5]) for b in batches.values()]
    torch.cuda.synchronize()
    assert torch.equal(outs[0][1], outs[1][1]) and torch.isfinite(outs[0][1]).all()


def test_cli_trains_with_device_decode(gpu, tmp_path):
    pytest.importorskip("transformers")
    data, img, vocab = make_msd_dir(str(tmp_path / "ds"), n=12)
    log = _cli(["--data_path", data, "--img_path", img, "--bert_name", vocab, "--num_epochs", "1", "--encoder_layers", "2",
                "--batch_size", "4", "--num_workers", "2", "--max_seq", "32", "--image_decode", "device"], tmp_path)
    assert "Test Eval results" in log and "12 decoded on the device, 0 on the host" in log
