"""Device JPEG decoding (d2r_jpeg_decode) vs decoding in the loader workers.

  --kernel-only : d2r_jpeg_decode on one batch of 32 q90 JPEGs of 0.3-2 MP, 50 times (run it under `rocprofv3 --kernel-trace --stats`
                  for the per-kernel times)
  (default)     : for that batch: bytes shipped per batch (decoded pixels vs JPEG segments + descriptors), host parse ms per image,
                  Pillow decode ms per image, event-timed d2r_jpeg_decode, the synchronisation rounds; then loader samples/s over
                  the 480-JPEG set of clip_preprocess_probe.py (same sizes, seeds and quality): MSDDataset + ClipCollate + the device
                  path with image_decode="host" vs "device", at 4 / 8 / 15 workers, over --epochs epochs after a warm-up epoch
                  (the prefetching workers fill their queues at every epoch start: the figure includes that, a lower bound).

    python tests/probes/jpeg_decode_probe.py [--kernel-only] [--images 480] [--workers 4,8,15] [--epochs 6]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from clip_preprocess_probe import _Tok, event_ms, sizes  # noqa: E402
from d2r_amd import image as I  # noqa: E402
from d2r_amd import jpeg as J  # noqa: E402
from d2r_amd.data import MSDDataset  # noqa: E402
from make_clip_golden import fixture_image  # noqa: E402


def jpeg_bytes(seed, h, w):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(fixture_image(seed, h, w)).save(b, format="JPEG", quality=90)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--images", type=int, default=480)
    ap.add_argument("--workers", default="4,8,15")
    ap.add_argument("--epochs", type=int, default=6, help="timed epochs over the images, after one that starts the workers")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    datas = [jpeg_bytes(1000 + i, h, w) for i, (h, w) in enumerate(sizes(a.batch))]
    infos = [J.parse(d) for d in datas]
    offsets = np.cumsum([0] + [i.H * i.W * 3 for i in infos])
    data_h, desc, segs, tab = J.plan_jpeg_batch(infos, offsets[:-1])
    meta_h = J._meta(desc, segs, tab)
    data, meta = torch.from_numpy(data_h).to(dev), meta_h.to(dev)
    dst = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=dev)
    ws = torch.empty(J.ws_bytes(desc), dtype=torch.uint8, device=dev)
    status = torch.empty(a.batch, dtype=torch.int32, device=dev)
    stats = torch.empty(2 * a.batch, dtype=torch.int32, device=dev)
    nd, ns = desc.nbytes, segs.nbytes

    def run():
        J.jpeg_decode(data, desc, meta[:nd], segs, meta[nd:nd + ns], meta_h[nd + ns:].view(torch.int32), meta[nd + ns:].view(torch.int32),
                      dst, status=status, stats=stats, ws=ws)

    if a.kernel_only:
        for _ in range(50):
            run()
        torch.cuda.synchronize()
        return
    ms = event_ms(run, 20)
    st = stats.view(-1, 2).cpu().numpy()
    assert not status.any()
    t = time.perf_counter()
    for d in datas:
        J.parse(d)
    parse_ms = (time.perf_counter() - t) / len(datas) * 1e3
    from PIL import Image
    t = time.perf_counter()
    for d in datas:
        with Image.open(io.BytesIO(d)) as im:
            np.asarray(im.convert("RGB"))
    pil_ms = (time.perf_counter() - t) / len(datas) * 1e3
    res = {"batch": a.batch, "decoded_MB": round(int(offsets[-1]) / 1e6, 1), "jpeg_files_MB": round(sum(map(len, datas)) / 1e6, 2),
           "packed_jpeg_MB": round((data_h.size + meta_h.numel()) / 1e6, 2), "decode_ms_events": round(ms, 3),
           "parse_ms_per_image": round(parse_ms, 2), "pillow_ms_per_image": round(pil_ms, 2),
           "sync_rounds_max": int(st[:, 0].max()), "sync_rounds_median": float(np.median(st[:, 0])),
           "boundary_redecodes_total": int(st[:, 1].sum()), "chunks_total": int(desc["nchunk"].sum())}
    print(json.dumps(res), flush=True)

    with tempfile.TemporaryDirectory() as d:
        samples = []
        for i, (h, w) in enumerate(sizes(a.images, seed=1)):
            with open(os.path.join(d, f"p{i}.jpg"), "wb") as f:
                f.write(jpeg_bytes(2000 + i, h, w))
            samples.append({"id": f"p{i}", "text": "a b c", "emotion_label": i % 3})
        with open(os.path.join(d, "all.json"), "w") as f:
            json.dump(samples, f)
        for nw in [int(x) for x in a.workers.split(",")]:
            for mode in ("host", "device"):
                ds = MSDDataset(os.path.join(d, "all.json"), d, _Tok(), max_seq=64, image_decode=mode)
                dl = DataLoader(ds, batch_size=a.batch, num_workers=nw, pin_memory=True,
                                collate_fn=I.ClipCollate(224, 224, image_decode=mode),
                                persistent_workers=True, prefetch_factor=4)
                rates, n_all, t_all, shipped = [], 0, 0.0, 0
                for epoch in range(1 + a.epochs):  # epoch 0 starts the workers and is not counted
                    t = time.perf_counter()
                    n = 0
                    for batch in dl:
                        p = batch[5]
                        shipped += (p.pixels.numel() + p.meta.numel()) if mode == "host" else \
                            (p.host_pixels.numel() + p.data.numel() + p.jmeta.numel() + p.clip_meta.numel())
                        x = p.to_pixel_values(dev)
                        n += x.shape[0]
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t
                    if epoch:
                        rates.append(n / dt)
                        n_all += n
                        t_all += dt
                print(json.dumps({"image_decode": mode, "workers": nw, "epochs": a.epochs, "samples_per_s": round(n_all / t_all, 1),
                                  "epoch_min": round(min(rates), 1), "epoch_max": round(max(rates), 1),
                                  "MB_per_batch": round(shipped / 1e6 / ((n_all + n_all // a.epochs) / a.batch), 2)}), flush=True)
                del dl


if __name__ == "__main__":
    main()
