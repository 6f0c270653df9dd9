"""Host side of the device JPEG decoder (d2r_amd.jpeg), on a CPU: the numpy restatement of the decode (reference_decode) is
bit-identical to Pillow on every file the parser accepts; the parser routes every file of the matrix to the intended side; the
numpy unstuffing and restart splitting agree with a byte loop; descriptors that would escape their buffers are refused before
anything is launched.  The JPEGs are made at test time with Pillow from make_clip_golden.fixture_image seeds."""
import ctypes
import io

import numpy as np
import pytest

from make_clip_golden import fixture_image

from d2r_amd import jpeg as J


def encode(seed, H, W, gray=False, fmt="JPEG", **kw):
    from PIL import Image
    img = fixture_image(seed, H, W)
    im = Image.fromarray(img[:, :, 0] if gray else img)
    if kw.pop("cmyk", False):
        im = im.convert("CMYK")
    b = io.BytesIO()
    im.save(b, format=fmt, **kw)
    return b.getvalue()


def pillow_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


SAMPLING = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "gray": dict(gray=True)}
SIZES = [(1, 1), (2, 2), (3, 5), (7, 13), (17, 9), (1000, 3), (3, 1000), (31, 47), (50, 66)]


def device_cases():
    """name -> bytes of every file the device decodes."""
    out = {}
    for q in (1, 50, 90, 100):
        for s, kw in SAMPLING.items():
            out[f"q{q}_{s}"] = encode(10 + q, 45, 61, quality=q, **kw)
    for (H, W) in SIZES:
        for s, kw in SAMPLING.items():
            out[f"size{H}x{W}_{s}"] = encode(H * 7 + W, H, W, quality=85, **kw)
    for s, kw in SAMPLING.items():
        out[f"optimize_{s}"] = encode(3, 70, 90, quality=75, optimize=True, **kw)
        out[f"rst_blocks_{s}"] = encode(4, 70, 90, quality=80, restart_marker_blocks=1, **kw)
        out[f"rst_rows_{s}"] = encode(5, 70, 90, quality=80, restart_marker_rows=1, **kw)
        out[f"rst3_{s}"] = encode(6, 41, 150, quality=95, restart_marker_blocks=3, **kw)
    out["rst_blocks_tiny"] = encode(7, 3, 5, quality=90, restart_marker_blocks=1, subsampling=2)
    return out


def with_sampling(data: bytes, y: int) -> bytes:
    """`data` with the luma sampling byte of its SOF0 replaced (chroma stays 1 x 1): only the routing reads it."""
    i = data.index(b"\xff\xc0") + 4 + 7
    return data[:i] + bytes([y]) + data[i + 1:]


def with_size(data: bytes, H: int, W: int) -> bytes:
    """`data` with the height and width of its SOF0 replaced."""
    i = data.index(b"\xff\xc0") + 5
    return data[:i] + H.to_bytes(2, "big") + W.to_bytes(2, "big") + data[i + 4:]


def with_dc_counts(data: bytes, counts) -> bytes:
    """`data` with the 16 code-length counts of its first DHT table (the luminance DC table) replaced; the symbol count must stay."""
    i = data.index(b"\xff\xc4") + 5
    assert sum(counts) == sum(data[i:i + 16])
    return data[:i] + bytes(counts) + data[i + 16:]


def host_cases():
    """name -> bytes of files that go to Pillow on the host."""
    good = encode(8, 40, 56, quality=90)
    return {
        "progressive": encode(9, 40, 56, quality=90, progressive=True),
        "cmyk": encode(10, 40, 56, quality=90, cmyk=True),
        "png_named_jpg": encode(11, 40, 56, fmt="PNG"),
        "truncated": good[:len(good) // 2],
        "no_eoi": good[:-2],
        "adobe_rgb": encode(12, 40, 56, quality=90, keep_rgb=True),
        "411": with_sampling(encode(13, 40, 56, quality=90), 0x41),
        "440": with_sampling(encode(14, 40, 56, quality=90), 0x12),
        "empty": b"",
        "bomb": with_size(encode(15, 16, 16, quality=90), 20000, 20000),       # Pillow: DecompressionBombError -> inf.png
        "all_ones_code": with_dc_counts(encode(16, 40, 56, gray=True, quality=90), [0, 0, 4, 8] + [0] * 12),  # JERR_BAD_HUFF_TABLE
    }


@pytest.fixture(scope="module")
def dev_cases():
    return device_cases()


@pytest.mark.parametrize("name", list(device_cases()))
def test_reference_decode_is_bit_identical_to_pillow(name, dev_cases):
    data = dev_cases[name]
    info, why = J.route(data)
    assert info is not None, f"{name} should decode on the device, the parser says: {why}"
    np.testing.assert_array_equal(J.reference_decode(data), pillow_rgb(data))


def test_host_cases_are_refused_by_pillow_where_they_should_be():
    from PIL import Image
    for name in ("bomb", "all_ones_code", "truncated"):
        with pytest.raises(Exception):
            with Image.open(io.BytesIO(host_cases()[name])) as im:
                im.convert("RGB")


def test_pixel_limit_follows_pillow(monkeypatch):
    from PIL import Image
    data = encode(17, 40, 56, quality=90)
    ok = with_size(data, 9000, 9000)        # 81 MP: inside 2 x MAX_IMAGE_PIXELS and the device limit
    assert J.route(ok)[0] is not None
    monkeypatch.setattr(Image, "MAX_IMAGE_PIXELS", 40_000_000)
    assert J.route(ok)[0] is None            # above twice a lowered limit: Pillow would refuse it, so it goes to the host
    monkeypatch.setattr(Image, "MAX_IMAGE_PIXELS", None)
    assert J.route(ok)[0] is not None
    assert J.route(with_size(data, 65535, 65535))[0] is None  # no Pillow limit, but above the device's 2^28 pixels


@pytest.mark.parametrize("name", list(host_cases()))
def test_host_files_are_routed_to_the_host(name):
    data = host_cases()[name]
    info, why = J.route(data)
    assert info is None and why
    with pytest.raises(J.HostPath):
        J.reference_decode(data)


def test_routing_details(dev_cases):
    i = J.parse(dev_cases["size2x2_420"])
    assert (i.hs, i.vs, i.fancy) == (2, 2, 0)  # a chroma plane of 1 sample: libjpeg replicates instead of fancy upsampling
    i = J.parse(dev_cases["size17x9_422"])
    assert (i.hs, i.vs, i.fancy) == (2, 1, 1)
    i = J.parse(dev_cases["rst_blocks_420"])
    assert i.restart == 1 and len(i.segments) == i.mcux * i.mcuy
    assert J.parse(dev_cases["size1000x3_gray"]).ncomp == 1


def naive_split(scan: bytes):
    """The byte loop: drop the zero after every 0xFF, cut at RSTn."""
    segs, cur, i = [], bytearray(), 0
    while i < len(scan):
        if scan[i] == 0xFF and i + 1 < len(scan):
            if scan[i + 1] == 0x00:
                cur.append(0xFF)
                i += 2
                continue
            if 0xD0 <= scan[i + 1] <= 0xD7:
                segs.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
        cur.append(scan[i])
        i += 1
    segs.append(bytes(cur))
    return segs


@pytest.mark.parametrize("seed", range(6))
def test_unstuff_and_restart_split_match_a_byte_loop(seed):
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(int(rng.integers(1, 9))):
        body = rng.choice(np.array([0, 1, 0x7F, 0xFE, 0xFF], np.uint8), size=int(rng.integers(0, 60)), p=[.2, .2, .2, .1, .3])
        stuffed = bytearray()
        for v in body:
            stuffed += bytes([v, 0]) if v == 0xFF else bytes([v])
        parts.append(bytes(stuffed))
    scan = b"".join(p + (bytes([0xFF, 0xD0 + k % 8]) if k + 1 < len(parts) else b"") for k, p in enumerate(parts))
    arr = np.frombuffer(scan, np.uint8)
    ff = np.flatnonzero(arr[:-1] == 0xFF)
    nxt = arr[ff + 1]
    segs = J.unstuff(arr, ff[nxt == 0], ff[(nxt >= 0xD0) & (nxt <= 0xD7)])
    assert [s.tobytes() for s in segs] == naive_split(scan)


def test_segments_of_a_real_file_match_a_byte_loop(dev_cases):
    data = dev_cases["rst_rows_420"]
    info = J.parse(data)
    sos = data.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    assert [s.tobytes() for s in info.segments] == naive_split(data[start:data.rindex(b"\xff\xd9")])


def test_plan_layout(dev_cases):
    infos = [J.parse(dev_cases[n]) for n in ("q90_420", "rst_rows_gray", "optimize_444")]
    data, desc, segs, tab = J.plan_jpeg_batch(infos, [0, 10000, 20000])
    assert data.size % 4 == 0 and (segs["offset"] % 4 == 0).all()
    for d, info in zip(desc, infos):
        s = segs[d["seg0"]:d["seg0"] + d["nseg"]]
        for row, seg in zip(s, info.segments):
            assert row["bits"] == seg.size * 8
            assert data[row["offset"]:row["offset"] + seg.size].tobytes() == seg.tobytes()
            assert not data[row["offset"] + seg.size:row["offset"] + seg.size + J.SEG_PAD].any()
        assert d["nchunk"] == sum(max(1, -(-int(r["bits"]) // J.CHUNK_BITS)) for r in s)
    assert (np.diff(desc["ws_rec"]) > 0).all() and desc["ws_coef"][0] >= desc["ws_rec"][-1] + 48 * desc["nchunk"][-1]
    assert J.ws_bytes(desc) == desc["ws_plane"][-1] + 64 * J._blocks(desc[-1])


def _call(data, desc, segs, tab, dst_bytes, ws_bytes, data_bytes=None):
    """d2r_jpeg_decode with device pointers that are never dereferenced: only the host-side checks run (they refuse)."""
    lib = J._lib.load()
    fake = 1 << 20
    return lib.d2r_jpeg_decode(fake, data.size if data_bytes is None else data_bytes,
                               ctypes.cast(desc.ctypes.data, ctypes.POINTER(J._lib.JpegImageDesc)), fake, len(desc),
                               ctypes.cast(segs.ctypes.data, ctypes.POINTER(J._lib.JpegSegment)), fake, len(segs), tab.ctypes.data, fake,
                               tab.size, fake, dst_bytes, fake, None, fake, ws_bytes, None)


def test_descriptors_that_escape_their_buffers_are_refused(dev_cases):
    infos = [J.parse(dev_cases[n]) for n in ("q90_420", "rst_blocks_422")]
    dst = [0, infos[0].H * infos[0].W * 3]
    data, desc, segs, tab = J.plan_jpeg_batch(infos, dst)
    dst_bytes = dst[1] + infos[1].H * infos[1].W * 3
    ws = J.ws_bytes(desc)
    bad = []
    d = desc.copy(); d[1]["dst_offset"] += 1; bad.append((d, segs, {}))                       # output past dst_bytes
    d = desc.copy(); d[1]["dst_offset"] = 5; bad.append((d, segs, {}))                        # overlaps image 0's pixels
    d = desc.copy(); d[0]["ac"][1] = tab.size - 10; bad.append((d, segs, {}))                  # Huffman table past the table
    d = desc.copy(); d[0]["qt"][0] = -1; bad.append((d, segs, {}))
    d = desc.copy(); d[0]["mcu_map"][0] = 0x13; bad.append((d, segs, {}))                      # block column 1 of a 1-wide comp.
    d = desc.copy(); d[0]["bw"][0] -= 2; bad.append((d, segs, {}))
    d = desc.copy(); d[1]["nseg"] -= 1; bad.append((d, segs, {}))                              # segments vs restart interval
    d = desc.copy(); d[0]["nchunk"] += 1; bad.append((d, segs, {}))
    d = desc.copy(); d[1]["ws_plane"] = d[0]["ws_plane"]; bad.append((d, segs, {}))           # overlapping workspace
    d = desc.copy(); d[0]["hs"], d[0]["vs"] = 1, 2; bad.append((d, segs, {}))                  # 4:4:0
    s = segs.copy(); s[-1]["bits"] += 8 * 8; bad.append((desc, s, {}))                         # last segment past the data
    s = segs.copy(); s[1]["offset"] += 2; bad.append((desc, s, {}))                            # misaligned
    s = segs.copy(); s[2]["chunk0"] += 1; bad.append((desc, s, {}))
    last = segs[-1]
    bad.append((desc, segs, {"data_bytes": int(last["offset"]) + -(-int(last["bits"]) // 8) + J.SEG_PAD - 1}))  # padding cut short
    for d, s, kw in bad:
        # a workspace of 0 bytes: were a check missing, the call would still be refused (-3), never launched
        assert _call(data, d, s, tab, dst_bytes, 0, **kw) == -1, J._lib.load().d2r_last_error()
    assert _call(data, desc, segs, tab, dst_bytes, ws - 1) == -3  # D2R_ERR_WORKSPACE
    assert b"workspace" in J._lib.load().d2r_last_error()


def test_dataset_returns_parsed_jpegs_in_device_mode(tmp_path):
    transformers = pytest.importorskip("transformers")
    import torch
    from test_clip_data import make_msd_dir
    from d2r_amd.data import MSDDataset
    from d2r_amd.image import ClipCollate, PackedImages
    data, img, vocab = make_msd_dir(str(tmp_path), n=6)
    with open(f"{img}/s1.jpg", "wb") as f:
        f.write(encode(1, 40, 50, quality=90, progressive=True))
    tok = transformers.BertTokenizer.from_pretrained(vocab, do_lower_case=True)
    host = MSDDataset(f"{data}/train.json", img, tok, max_seq=16)
    dev = MSDDataset(f"{data}/train.json", img, tok, max_seq=16, image_decode="device")
    items = [dev[i][5] for i in range(6)]
    assert isinstance(items[0], J.JpegInfo) and isinstance(items[1], np.ndarray)  # the progressive file is decoded here
    for i in range(6):
        ref = host[i][5]
        got = items[i] if isinstance(items[i], np.ndarray) else J.reference_decode(
            open(f"{img}/s{i}.jpg", "rb").read())
        np.testing.assert_array_equal(got, ref)
    packed = ClipCollate(224, 224)([dev[i] for i in range(6)])[5]
    assert isinstance(packed, J.PackedJpegImages) and (packed.n_device, packed.n_host) == (5, 1)
    assert isinstance(ClipCollate(224, 224)([host[i] for i in range(2)])[5], PackedImages)
    # in device mode a batch of host-decoded images only is still counted as such
    only_host = ClipCollate(224, 224, image_decode="device")([dev[1], dev[1]])[5]
    assert isinstance(only_host, J.PackedJpegImages) and (only_host.n_device, only_host.n_host) == (0, 2)
    import logging
    log = J.DecodeLog(logging.getLogger("test"))
    log.note((torch.zeros(1), packed))
    log.note((only_host,))
    assert (log.device, log.host) == (5, 3)
    with pytest.raises(ValueError):
        MSDDataset(f"{data}/train.json", img, tok, image_decode="gpu")
    assert torch.is_tensor(packed.host_pixels)


def test_cli_flag_defaults_to_host():
    from d2r_amd.run import build_parser
    assert build_parser().parse_args([]).image_decode == "host"
    assert build_parser().parse_args(["--image_decode", "device"]).image_decode == "device"
