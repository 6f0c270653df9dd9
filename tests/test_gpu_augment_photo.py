"""Photometric augmentation on the MI355X: d2r_clip_cache_augment_photo through the raw C ABI against
image.reference_photo in float64 (each option alone and all together, random boxes and flips, NaN guard bands round `out`), its
bit-exact properties (identity, erase box, grayscale, mirror, no statistics pass without contrast, determinism), refusals, the
batches of a photometric CachedLoader against the uncached training path, and training steps with and without the options."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_augment import GUARD, _guarded, _outside_is_nan, _trainer_hook, _two_steps
from test_gpu_dataset_cache import _loader, _tokenizer, make_dir

from d2r_amd import image as I

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MEAN, STD = I.CLIP_MEAN, I.CLIP_STD
ROWS = 6
# black, white, grey, near-grey (channel spread 1 / 255), saturated primaries, two equal maxima (hue sector boundaries), two equal minima
SPECIAL = np.array([(0, 0, 0), (255, 255, 255), (128, 128, 128), (100, 101, 100), (77, 77, 78), (255, 254, 255), (255, 0, 0), (0, 255, 0),
                    (0, 0, 255), (255, 255, 0), (0, 200, 200), (90, 10, 90), (1, 1, 0), (200, 13, 13), (255, 255, 254)], np.uint8)


def _cache(S, gpu, seed):
    """uint8 [ROWS, cache_row_bytes(S)] of random bytes (the padding too); the first pixels of every row are the SPECIAL colours,
    rotated by the row so that at S = 1 the rows are six different ones."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (ROWS, I.cache_row_bytes(S)), dtype=np.uint8)
    plane = S * S
    for r in range(ROWS):
        for p in range(min(plane, len(SPECIAL))):
            rows[r, [p, plane + p, 2 * plane + p]] = SPECIAL[(p + r) % len(SPECIAL)]
    return rows, torch.from_numpy(rows).to(gpu)


def _crop(rows, r, S):
    return rows[r][:3 * S * S].reshape(3, S, S)


def _boxes(S, B, seed):
    """Random resized crops and flips as the augmenter draws them (scale 0.2 .. 1)."""
    from d2r_amd.augment import Augmenter
    return [tuple(int(v) for v in row[:5]) for row in Augmenter(S, 0.2, 0.5, seed=seed).draw(B)]


def _f32(v):
    return float(np.float32(v))


def _photos(mode, S, B=4):
    """B descriptors with `mode` on ("all": every option): factors below and above 1, 0, a large one, one sample with contrast 1
    next to samples that need the statistics pass; hue at both ends, small and 0.07; erase boxes at a corner, in the middle, the whole
    image and one pixel."""
    opts = {"brightness": [0.6, 1.4, 0.0, 2.5], "contrast": [0.6, 1.4, 1.0, 0.0], "saturation": [0.6, 1.4, 0.0, 3.0],
            "hue": [-0.5, -0.1, 0.07, 0.5], "gray": [1, 0, 1, 1]}
    m = max(S // 2, 1)
    erase = [(0, 0, m, 1), (S // 3, S // 4, max(S // 3, 1), m), (0, 0, S, S), (S - 1, S - 1, 1, 1)]
    out = []
    for b in range(B):
        row = [1.0, 1.0, 1.0, 0.0, 0, 0, 0, 0, 0]
        for k, name in enumerate(("brightness", "contrast", "saturation", "hue", "gray")):
            if mode in (name, "all"):
                row[k] = _f32(opts[name][b]) if k < 4 else opts[name][b]
        if mode in ("erase", "all"):
            row[5:9] = erase[b]
        out.append(tuple(row))
    return out


def _raw_photo(cache, h_idx, boxes, photos, S, out, gpu, ws=None, ws_bytes=None, h_photo_null=False, photo_null=False, norm=None,
               reserved=False):
    """d2r_clip_cache_augment_photo through ctypes on torch's current stream, synchronised -> (status, the workspace)."""
    from d2r_amd.functional import _stream
    lib = I._lib.load()
    h = np.asarray(h_idx, np.int64)
    d = np.zeros((len(h), 8), np.int32)
    d[:, :5] = np.asarray(boxes, np.int32)
    p = I.photo_desc(photos).numpy().copy()
    if reserved:
        p[0, 11] = 7
    idx = torch.from_numpy(h).clamp(0, cache.shape[0] - 1).to(gpu)
    aug, photo = torch.from_numpy(d).to(gpu), torch.from_numpy(p).to(gpu)
    need = lib.d2r_clip_cache_augment_photo_ws_bytes(len(h), S)
    if ws is None:
        ws = torch.zeros(max(need // 4, 1), device=gpu)
    nm = (ctypes.c_float * 6)(*(norm or (MEAN + STD)))
    rc = lib.d2r_clip_cache_augment_photo(cache.data_ptr(), cache.shape[0], h.ctypes.data, idx.data_ptr(),
                                          ctypes.cast(d.ctypes.data, ctypes.POINTER(I._lib.ClipAugmentDesc)), aug.data_ptr(),
                                          None if h_photo_null else ctypes.cast(p.ctypes.data, ctypes.POINTER(I._lib.ClipPhotoDesc)),
                                          None if photo_null else photo.data_ptr(), len(h), S, nm, 1 / 255, out.data_ptr(),
                                          ws.data_ptr(), need if ws_bytes is None else ws_bytes, _stream())
    torch.cuda.synchronize()
    return rc, ws


def _hue32(x, delta):
    """Step 4 in numpy float32, operation for operation as photo_hue in csrc/image.hip (every operation rounded on its own)."""
    f = np.float32
    r, g, b = (x[c].astype(f) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    cr = mx - mn
    grey = cr == 0
    s = cr / np.where(grey, f(1), mx)
    inv = f(1) / np.where(grey, f(1), cr)
    rc, gc, bc = (mx - r) * inv, (mx - g) * inv, (mx - b) * inv
    h6 = np.where(mx == r, bc - gc, np.where(mx == g, f(2) + rc - bc, f(4) + gc - rc))
    h = h6 * (f(1) / f(6)) + f(delta)
    h = h - np.floor(h)
    hs = h * f(6)
    fl = np.floor(hs)
    fr = hs - fl
    sec = fl.astype(np.int64)
    sec = np.where(sec >= 6, sec - 6, sec)
    clamp = lambda v: np.minimum(np.maximum(v, f(0)), f(1))  # noqa: E731
    p, q, t = clamp(mx * (f(1) - s)), clamp(mx * (f(1) - s * fr)), clamp(mx * (f(1) - s * (f(1) - fr)))
    assert all(v.dtype == f for v in (p, q, t, mx))
    return np.stack([np.choose(sec, [mx, q, p, p, t, mx]), np.choose(sec, [t, mx, mx, q, p, p]), np.choose(sec, [p, p, t, mx, mx, q])])


def _parts(S):
    return -(-S * ((S + 3) // 4) // 256)


def _bound(photo, S, hue_tol):
    """Per channel, the largest |out - reference_photo| the kernel's operation order allows, by counting roundings (u = 2^-24; all
    values lie in [0, 1] after every clamp, a clamp is 1-Lipschitz, and an fma in place of a product and a sum only removes a rounding):
      raw value: fl(1/255) and the product, 2u; K21's blend of values <= 1: 8u (tests/test_gpu_augment.py) -> e = 10u;
      g(x): the weights' roundings (together u, they sum to 1), three products (together u), two sums: e_g = e + 4u;
      1. fl(beta * x), clamped: e <- beta * e + u;
      2. m: every g passes through at most 3 additions in its thread, 6 in the wavefront's halving, 3 across the four wavefronts and
         parts - 1 across the partial sums, then the division by S^2: chain = 3 + 6 + 3 + (parts - 1) + 1 roundings relative to a
         mean <= 1, so e_m = e_g + chain * u (1.001 covers the second-order terms);  fl(1 - kappa), its product with m and the
         product kappa * x are rounded relative to |1 - kappa| and kappa, the sum relative to a result that matters only inside
         [0, 1]: e <- kappa * e + |1 - kappa| * e_m + u * (kappa + 2 |1 - kappa| + 1);
      3. likewise with g(x) of the same pixel: e <- sigma * e + |1 - sigma| * (e + 4u) + u * (sigma + 2 |1 - sigma| + 1);
      4. hue: the outputs are max, min and min + (max - min) * psi((mid - min) / (max - min)) with psi piecewise linear of slope
         +-1 and values in [0, 1]: on a linear piece psi(z) = c +- z with c in [0, 2], so the third value is a combination of max, mid
         and min whose coefficients' magnitudes sum to at most 3: an input error e comes out as at most 3e.  To that the step's own
         rounding is added, hue_tol, measured on the test's inputs (see _hue_tol);
      5. e <- e + 4u;
      6. fl(mean_c) is off by u * mean_c <= u / 2, the difference is rounded once (u), fl(std_c) and the division are relative to
         the result, at most max(mean_c, 1 - mean_c) / std_c: (e + 1.5u) / std_c + 2u * max(mean_c, 1 - mean_c) / std_c;
      7. the erase box writes an exact 0."""
    beta, kappa, sigma, delta, gray = photo[:5]
    e = 10 * U
    if beta != 1.0:
        e = beta * e + U
    if kappa != 1.0:
        chain = 3 + 6 + 3 + (_parts(S) - 1) + 1
        e_m = e + 4 * U + 1.001 * chain * U
        e = kappa * e + abs(1 - kappa) * e_m + U * (kappa + 2 * abs(1 - kappa) + 1)
    if sigma != 1.0:
        e = sigma * e + abs(1 - sigma) * (e + 4 * U) + U * (sigma + 2 * abs(1 - sigma) + 1)
    if delta != 0.0:
        e = 3 * e + hue_tol
    if gray:
        e = e + 4 * U
    return np.array([(e + 1.5 * U) / s + 2 * U * max(m, 1 - m) / s for m, s in zip(MEAN, STD)])


def _hue_tol(crop, box, photo, S):
    """The hue step's own rounding error, measured: the float32 restatement of step 4 (_hue32) against float64 on what reaches the
    step in this very sample (the float64 result of steps 1 - 3, rounded to fp32).  The GPU gets 4x that, for fma contraction and
    hardware division, and never more than 64u.  -> (tolerance, the emulation's error)."""
    before = I.reference_photo(crop, box, tuple(photo[:3]) + (0.0, 0, 0, 0, 0, 0), S, (0.0,) * 3, (1.0,) * 3).astype(np.float32)
    emu = float(np.abs(_hue32(before, photo[3]).astype(np.float64) - I.reference_hue(before.astype(np.float64), photo[3])).max())
    return min(4 * emu, 64 * U), emu


CASES = [(S, mode) for S in (1, 5, 7, 16) for mode in ("brightness", "contrast", "saturation", "hue", "gray", "erase", "all")] + [(224, "all")]
H_IDX = [3, 0, 5, 3]  # a repeated row carries different boxes and settings


@pytest.mark.parametrize("S,mode", CASES)
def test_each_option_and_all_together_against_reference_photo(gpu, S, mode):
    rows, cache = _cache(S, gpu, 10 + S)
    B = len(H_IDX)
    n = B * 3 * S * S
    photos = _photos(mode, S)
    for offset, seed in ((0, 1), (1, 2)):  # 1: `out` is not 16-byte aligned, every store is a single one
        boxes = _boxes(S, B, 100 * S + seed)
        buf, out = _guarded(n, gpu, offset)
        rc, _ = _raw_photo(cache, H_IDX, boxes, photos, S, out, gpu)
        assert rc == 0, I._lib.load().d2r_last_error().decode()
        assert _outside_is_nan(buf, n, offset), "write outside out"
        got = out.view(B, 3, S, S).cpu().double().numpy()
        assert np.isfinite(got).all(), "NaN or infinity in the output"
        for b in range(B):
            crop = _crop(rows, H_IDX[b], S)
            want = I.reference_photo(crop, boxes[b], photos[b], S, MEAN, STD)
            tol, emu = _hue_tol(crop, boxes[b], photos[b], S) if photos[b][3] != 0.0 else (0.0, 0.0)
            bound = _bound(photos[b], S, tol)
            err = np.abs(got[b] - want).max(axis=(1, 2))
            print(f"S={S} {mode} offset={offset} sample {b} {photos[b][:5]}: max |err| per channel {[f'{e:.3g}' for e in err]}, bound "
                  f"{[f'{v:.3g}' for v in bound]}, hue emulation {emu / U:.2f} u, hue tolerance {tol / U:.2f} u")
            assert bool((err <= bound).all()), (S, mode, b, boxes[b], photos[b], err.tolist(), bound.tolist())


def _host_identity(rows, h_idx, S):
    """(v / 255 - mean) / std in fp32 in the documented order: fl(fl(fl(float(v) * fl(1/255)) - fl(mean_c)) / fl(std_c))."""
    f = np.float32
    out = []
    for r in h_idx:
        x = _crop(rows, r, S).astype(f) * f(1 / 255)
        out.append((x - np.asarray(MEAN, f)[:, None, None]) / np.asarray(STD, f)[:, None, None])
    out = np.stack(out)
    assert out.dtype == f
    return torch.from_numpy(out)


@pytest.mark.parametrize("S", [1, 5, 7, 16, 224])
def test_identity_descriptors_are_the_fp32_normalisation_bit_for_bit(gpu, S):
    rows, cache = _cache(S, gpu, 30 + S)
    B = len(H_IDX)
    n = B * 3 * S * S
    want = _host_identity(rows, H_IDX, S).view(torch.int32)
    for offset in (0, 1):
        buf, out = _guarded(n, gpu, offset)
        rc, _ = _raw_photo(cache, H_IDX, [(0, 0, S, S, 0)] * B, _photos("none", S), S, out, gpu)
        assert rc == 0 and _outside_is_nan(buf, n, offset)
        assert torch.equal(out.view(B, 3, S, S).cpu().view(torch.int32), want), offset


def _run(cache, boxes, photos, S, gpu, ws=None, fill=float("nan")):
    B = len(boxes)
    out = torch.full((B * 3 * S * S,), fill, device=gpu)
    rc, ws = _raw_photo(cache, H_IDX[:B], boxes, photos, S, out, gpu, ws=ws)
    assert rc == 0, I._lib.load().d2r_last_error().decode()
    return out.view(B, 3, S, S), ws


@pytest.mark.parametrize("S", [5, 16, 224])
def test_erase_box_grayscale_and_flip_bit_for_bit(gpu, S):
    _, cache = _cache(S, gpu, 50 + S)
    B = len(H_IDX)
    boxes = [b[:4] + (0,) for b in _boxes(S, B, 7 * S)]
    photos = _photos("all", S)
    full, _ = _run(cache, boxes, photos, S, gpu)
    assert bool(torch.isfinite(full).all())
    # erase: exactly +0.0f inside, the bits of the call without the box outside
    no_erase, _ = _run(cache, boxes, [p[:5] + (0, 0, 0, 0) for p in photos], S, gpu)
    for b, p in enumerate(photos):
        ex0, ey0, ew, eh = p[5:9]
        inside = torch.zeros(S, S, dtype=torch.bool, device=gpu)
        inside[ey0:ey0 + eh, ex0:ex0 + ew] = True
        assert bool(inside.any())
        assert bool((full[b].view(torch.int32)[:, inside] == 0).all()), "not +0.0f inside the erase box"
        assert torch.equal(full[b].view(torch.int32)[:, ~inside], no_erase[b].view(torch.int32)[:, ~inside])
    # grayscale: three bit-equal channels; the normalisation differs per channel, so mean 0 and std 1 here
    grey = [p[:4] + (1,) + p[5:] for p in photos]
    out = torch.full((B * 3 * S * S,), float("nan"), device=gpu)
    rc, _ = _raw_photo(cache, H_IDX, boxes, grey, S, out, gpu, norm=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
    g = out.view(B, 3, S, S).view(torch.int32)
    assert rc == 0 and torch.equal(g[:, 0], g[:, 1]) and torch.equal(g[:, 0], g[:, 2])
    assert S == 1 or len(torch.unique(g[1, 0])) > 1
    # flip: the mirror image (the erase box is given in output coordinates, so it is mirrored by hand), contrast mean included
    flipped = [b[:4] + (1,) for b in boxes]
    mirrored = [p[:5] + (S - p[5] - p[7], p[6], p[7], p[8]) for p in photos]
    fl, _ = _run(cache, flipped, mirrored, S, gpu)
    assert torch.equal(fl.view(torch.int32), full.flip(-1).view(torch.int32))
    assert not torch.equal(fl, full)


def test_without_contrast_no_statistics_pass_runs_and_the_workspace_is_never_touched(gpu):
    S = 224
    _, cache = _cache(S, gpu, 70)
    B = len(H_IDX)
    boxes = _boxes(S, B, 71)
    photos = [p[:1] + (1.0,) + p[2:] for p in _photos("all", S)]
    need = I.clip_cache_augment_photo_ws_bytes(B, S) // 4
    assert need == B * _parts(S) == 4 * 49
    ws = torch.full((need + 64,), float("nan"), device=gpu)
    out, _ = _run(cache, boxes, photos, S, gpu, ws=ws)
    assert bool(torch.isfinite(out).all()), "the NaN workspace reached the output: it was read without a contrast factor"
    assert bool(torch.isnan(ws).all()), "the workspace was written without a contrast factor"
    # with contrast on for samples 0, 1 and 3 (sample 2 has factor 1): their partial sums are written, nothing else is
    out, _ = _run(cache, boxes, _photos("all", S), S, gpu, ws=ws)
    assert bool(torch.isfinite(out).all())
    w = ws[:need].view(B, _parts(S))
    assert bool(torch.isfinite(w[[0, 1, 3]]).all()) and bool(torch.isnan(w[2]).all()) and bool(torch.isnan(ws[need:]).all())


def test_a_second_run_is_bit_identical(gpu):
    S = 224
    _, cache = _cache(S, gpu, 80)
    boxes, photos = _boxes(S, len(H_IDX), 81), _photos("all", S)
    runs = []
    for fill in (0.0, 1.0):
        ws = torch.full((I.clip_cache_augment_photo_ws_bytes(len(H_IDX), S) // 4,), fill, device=gpu)
        out, _ = _run(cache, boxes, photos, S, gpu, ws=ws, fill=fill)
        runs.append(out.view(torch.int32).cpu())
    assert torch.equal(runs[0], runs[1])


def test_refused_calls_return_an_error_and_write_nothing(gpu):
    S = 16
    _, cache = _cache(S, gpu, 90)
    ok_box, ok = (0, 0, S, S, 0), _photos("none", S)[0]
    n = 2 * 3 * S * S
    out = torch.full((n + 2 * GUARD,), 7.0, device=gpu)
    target = out[GUARD:GUARD + n]
    ws = torch.full((64,), 7.0, device=gpu)
    p = lambda **kw: tuple(kw.get(k, v) for k, v in zip(("brightness", "contrast", "saturation", "hue", "gray", "ex0", "ey0", "ew", "eh"), ok))  # noqa: E731
    cases = {"index out of range": dict(h_idx=[0, ROWS]), "box outside": dict(boxes=[ok_box, (9, 0, 8, 4, 0)]),
             "flip = 2": dict(boxes=[ok_box, (0, 0, 4, 4, 2)]), "negative brightness": dict(photos=[ok, p(brightness=-0.5)]),
             "NaN contrast": dict(photos=[ok, p(contrast=float("nan"))]), "infinite saturation": dict(photos=[p(saturation=float("inf")), ok]),
             "hue 0.6": dict(photos=[ok, p(hue=0.6)]), "gray = 2": dict(photos=[ok, p(gray=2)]),
             "erase box outside": dict(photos=[ok, p(ex0=9, ew=8, eh=2)]), "erase height 0": dict(photos=[ok, p(ew=2, eh=0)]),
             "reserved word": dict(reserved=True), "null host descriptors": dict(h_photo_null=True),
             "null device descriptors": dict(photo_null=True), "short workspace": dict(ws_bytes=4),
             "std 0": dict(norm=(0.5, 0.5, 0.5, 1.0, 0.0, 1.0))}
    for what, kw in cases.items():
        rc, _ = _raw_photo(cache, kw.pop("h_idx", [0, 1]), kw.pop("boxes", [ok_box, ok_box]), kw.pop("photos", [p(contrast=0.5), ok]), S,
                           target, gpu, ws=ws, **kw)
        assert rc == (-3 if what == "short workspace" else -1), (what, rc)
        assert "d2r_clip_cache_augment_photo" in I._lib.load().d2r_last_error().decode(), what
        assert bool((out == 7.0).all()) and bool((ws == 7.0).all()), f"{what}: the refused call wrote"
    # the checked wrapper raises for the same arguments, and accepts valid ones
    h = torch.tensor([0, 1], dtype=torch.int64)
    box = torch.zeros(2, 8, dtype=torch.int32)
    box[:, 2:4] = S
    bad, good = I.photo_desc([ok, p(hue=0.6)]), I.photo_desc([p(contrast=0.5), p(hue=0.5, ew=3, eh=2)])
    with pytest.raises(I._lib.D2RError, match="hue"):
        I.clip_cache_augment_photo(cache, h, h.to(gpu), box, box.to(gpu), bad, bad.to(gpu), S, out=target)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    I.clip_cache_augment_photo(cache, h, h.to(gpu), box, box.to(gpu), good, good.to(gpu), S, out=target)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(target).all()) and not bool((target == 7.0).any())
    assert bool((out[:GUARD] == 7.0).all()) and bool((out[-GUARD:] == 7.0).all())


ON = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, grayscale_p=0.25, erase_p=0.5)


def test_cached_loader_with_a_photometric_augmenter_yields_the_uncached_paths_batches(gpu, tmp_path):
    """Equal seeds: over two epochs the batches of the cached training loader are, bit for bit, those of the uncached training
    path (to_cache into the scratch rows, then the same kernels), with crop and flip on as well."""
    from d2r_amd.augment import Augmenter
    from d2r_amd.cache import CachedLoader, DeviceDatasetCache, prefill, release_workers
    S = 64
    data, img, vocab = make_dir(tmp_path)
    tok = _tokenizer(vocab)
    trainer = _trainer_hook(gpu)
    plain = _loader(data, img, tok, "train", True, "host", S=S)
    aug, geometric = Augmenter(S, 0.3, 0.5, seed=17, **ON), Augmenter(S, 0.3, 0.5, seed=17)
    torch.manual_seed(9)
    want, crops_only = [], []
    for epoch in range(2):
        for b in plain:
            want.append(tuple(t.cpu() for t in trainer._to_device(b, aug)))
            crops_only.append(trainer._to_device(b, geometric)[5].cpu())
    release_workers(plain)
    assert len(want) == 4 and all(bool(torch.isfinite(w[5]).all()) for w in want)
    assert all(not torch.equal(w[5], u) for w, u in zip(want, crops_only)), "the photometric options changed nothing"

    wrapped = _loader(data, img, tok, "train", True, "host", S=S)
    cache = DeviceDatasetCache.for_loader(wrapped, gpu, "train")
    torch.manual_seed(9)
    prefill(wrapped, cache, split="train")
    cached = CachedLoader(wrapped, cache, Augmenter(S, 0.3, 0.5, seed=17, **ON))
    got = [tuple(t.cpu() for t in b) for epoch in range(2) for b in cached]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    release_workers(wrapped)


@pytest.fixture(scope="module")
def plain_run(gpu, tmp_path_factory):
    """The generated image directory and the run without an augmenter: computed once, shared, left unchanged."""
    data, img, vocab = make_dir(tmp_path_factory.mktemp("augment_photo_trainer"))
    dirs = (data, img, _tokenizer(vocab))
    return dirs, _two_steps(gpu, dirs, "photo-none", None)


def test_a_run_with_the_options_differs_stays_finite_and_leaves_the_default_generator_alone(gpu, plain_run):
    from d2r_amd.augment import Augmenter
    dirs, (w0, l0, s0, _) = plain_run
    w2, l2, s2, a2 = _two_steps(gpu, dirs, "photo-on", Augmenter(64, seed=5, **ON))
    assert len(l2) == 1 and np.isfinite(l2[0]) and l2 != l0 and not torch.equal(w2, w0)
    assert bool(torch.isfinite(w2).all())
    assert torch.equal(s0, s2), "the augmenter moved torch's default generator"
    assert len(a2) == 1 and "brightness 0.4" in a2[0] and "hue 0.1" in a2[0] and "erasing with probability 0.5" in a2[0], a2


def test_a_run_with_all_six_at_their_defaults_is_bit_identical_to_the_plain_run(gpu, plain_run):
    from d2r_amd.augment import Augmenter
    dirs, (w0, l0, s0, _) = plain_run
    defaults = dict(brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, grayscale_p=0.0, erase_p=0.0)
    aug = Augmenter(64, 1.0, 0.0, seed=5, **defaults)
    w1, l1, s1, a1 = _two_steps(gpu, dirs, "photo-defaults", aug)
    assert not aug.photometric and aug.photo_generator is None
    assert l0 == l1 and torch.equal(w0, w1) and torch.equal(s0, s1)
    assert len(a1) == 1 and "brightness" not in a1[0]
