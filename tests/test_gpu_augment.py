"""Image augmentation on the MI355X: d2r_clip_cache_augment through the raw C ABI (identity box against d2r_clip_cache_gather,
arbitrary boxes against torch's float64 interpolate on the CPU, flip, determinism, refusals; NaN guard bands round `out`), the
batches of an augmenting CachedLoader against the uncached training path, and training steps with and without an augmenter."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from test_gpu_dataset_cache import _loader, _logger, _small_model, _tokenizer, make_dir

from d2r_amd import image as I

pytestmark = pytest.mark.gpu

GUARD = 4096
ROUNDINGS = 8  # see test_boxes_against_float64_interpolate


def _tables(gpu):
    """CLIP's table, and one with negative, tiny and large entries."""
    rng = np.random.default_rng(5)
    wild = (rng.standard_normal((3, 256)) * 300).astype(np.float32)
    wild[0, :4], wild[1, 7], wild[2, 250:] = (-4096.0, 4000.5, 1e-30, 0.0), -3.5e3, 1234.5678
    return [("clip", I.normalize_table()), ("wild", wild)]


def _cache(rows, S, gpu, seed):
    """uint8 [rows, cache_row_bytes(S)] of random bytes, the rows' padding included (nothing may read it as pixels)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (rows, I.cache_row_bytes(S)), dtype=torch.uint8, generator=g).to(gpu)


def _guarded(n, gpu, offset=0):
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=gpu)
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _outside_is_nan(buf, n, offset=0):
    return bool(torch.isnan(buf[:GUARD + offset]).all()) and bool(torch.isnan(buf[GUARD + offset + n:]).all())


def _desc(boxes):
    d = np.zeros((len(boxes), 8), np.int32)
    d[:, :5] = np.asarray(boxes, np.int32)
    return d


def _raw_augment(cache, h_idx, boxes, S, lut, out, gpu, h_aug_null=False, aug_null=False):
    """d2r_clip_cache_augment through ctypes on torch's current stream, synchronised -> its status."""
    from d2r_amd.functional import _stream
    lib = I._lib.load()
    h = np.asarray(h_idx, np.int64)
    d = _desc(boxes)
    idx = torch.from_numpy(h).clamp(0, cache.shape[0] - 1).to(gpu)
    aug = torch.from_numpy(d).to(gpu)
    rc = lib.d2r_clip_cache_augment(cache.data_ptr(), cache.shape[0], h.ctypes.data, idx.data_ptr(),
                                    None if h_aug_null else ctypes.cast(d.ctypes.data, ctypes.POINTER(I._lib.ClipAugmentDesc)),
                                    None if aug_null else aug.data_ptr(), len(h), S, lut.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


def _raw_gather(cache, h_idx, S, lut, out, gpu):
    from d2r_amd.functional import _stream
    h = np.asarray(h_idx, np.int64)
    idx = torch.from_numpy(h).to(gpu)
    rc = I._lib.load().d2r_clip_cache_gather(cache.data_ptr(), cache.shape[0], h.ctypes.data, idx.data_ptr(), len(h), S, lut.data_ptr(),
                                             out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("S", [1, 5, 7, 16, 224])
def test_identity_box_is_the_plain_gather_bit_for_bit(gpu, S):
    cache = _cache(4, S, gpu, S)
    h_idx = [2, 0, 2, 3, 0]
    n = len(h_idx) * 3 * S * S
    for name, table in _tables(gpu):
        lut = torch.from_numpy(table).to(gpu)
        for offset in (0, 1):  # 1: `out` is not 16-byte aligned, every store is a single one
            wbuf, want = _guarded(n, gpu, offset)
            gbuf, got = _guarded(n, gpu, offset)
            assert _raw_gather(cache, h_idx, S, lut, want, gpu) == 0
            assert _raw_augment(cache, h_idx, [(0, 0, S, S, 0)] * len(h_idx), S, lut, got, gpu) == 0
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, offset)
            assert _outside_is_nan(gbuf, n, offset), "write outside out"
            assert bool(torch.isfinite(got).all())


def _boxes_for(S):
    """B = 8 boxes: w = 1, h = 1, w = S (full width), the whole crop, an interior box, x0 + w = S, y0 + h = S, a 1 x 1 box."""
    m = max(S // 2, 1)
    q = max(S // 4, 1) if S > 2 else 0
    inner = (q, q, max(S - 2 * q - (S > 2), 1), max(S - 2 * q - (S > 3), 1)) if S > 2 else (0, 1, 1, 1)
    return [(S // 2, 0, 1, S), (0, S - 1, S, 1), (0, S // 3, S, m), (0, 0, S, S), inner, (S - m, 0, m, S - (S > 1)),
            (min(1, S - 1), S - m, max(S - 2, 1), m), (S - 1, S - 1, 1, 1)]


def _oracle(cache, table, h_idx, boxes, S):
    """torch.nn.functional.interpolate in float64 on the CPU, on the box cropped out of the normalised image; flipped after."""
    rows = cache.cpu().numpy()
    out = []
    for r, (x0, y0, w, h, flip) in zip(h_idx, boxes):
        crop = torch.from_numpy(rows[r][:3 * S * S].reshape(3, S, S).astype(np.int64))
        T = torch.stack([torch.from_numpy(table[c].astype(np.float64))[crop[c]] for c in range(3)])
        o = TF.interpolate(T[:, y0:y0 + h, x0:x0 + w].double()[None], size=(S, S), mode="bilinear", align_corners=False)[0]
        out.append(o.flip(-1) if flip else o)
    return torch.stack(out)


H_IDX = [0, 1, 1, 5, 3, 3, 2, 5]  # 6 cache rows; repeated indices carry different boxes


@pytest.mark.parametrize("S", [2, 7, 16, 224])
def test_boxes_against_float64_interpolate(gpu, S):
    """Per element |out - oracle| <= k * 2^-24 * max|lut| with k = 8, the roundings of the kernel's operation order (aug_axis /
    aug_blend in csrc/image.hip; no operation is contracted into an fma).  With M = max|lut| and u = 2^-24, every intermediate is
    a convex combination of table entries up to O(u), so each rounding adds at most u * M:
      1. fx = fl(r / 2S): the remainder and 2S are exact in fp32, one rounding.  Its error d (|d| <= u * fx) moves the row blend by
         d * (b - a), at most 2 * u * M * fx;
      2. gx = fl(1 - fx): at most u * M * gx more - together with 1. at most u * M * (2 fx + gx) <= 2 * u * M: two roundings' worth;
      3. fl(gx * a) and fl(fx * b): u * M * (gx + fx) = u * M between them: one;
      4. their sum: one.  A row blend is off by at most 4 * u * M, and so is their weighted mean in the column blend;
      5. fy, gy: two, as 1. and 2.;  6. the two products: one;  7. the final sum: one.
    4 + 2 + 1 + 1 = 8.  The oracle's own float64 error (1e-16 * M) is far below one fp32 rounding."""
    cache = _cache(6, S, gpu, 100 + S)
    boxes = _boxes_for(S)
    for x0, y0, w, h in boxes:
        assert x0 >= 0 and y0 >= 0 and w >= 1 and h >= 1 and x0 + w <= S and y0 + h <= S, (S, x0, y0, w, h)
    assert any(w == 1 for _, _, w, _ in boxes) and any(h == 1 for _, _, _, h in boxes) and any(w == S for _, _, w, _ in boxes)
    assert any(x0 + w == S and x0 > 0 for x0, _, w, _ in boxes) or S == 1
    n = len(H_IDX) * 3 * S * S
    for name, table in _tables(gpu):
        lut = torch.from_numpy(table).to(gpu)
        bound = ROUNDINGS * 2.0 ** -24 * float(np.abs(table).max())
        for flips in ([0, 1, 0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0, 1, 0]):
            full = [(*b, f) for b, f in zip(boxes, flips)]
            buf, out = _guarded(n, gpu)
            assert _raw_augment(cache, H_IDX, full, S, lut, out, gpu) == 0
            assert _outside_is_nan(buf, n), "write outside out"
            got = out.view(len(H_IDX), 3, S, S).cpu().double()
            assert bool(torch.isfinite(got).all())
            want = _oracle(cache, table, H_IDX, full, S)
            err = (got - want).abs().amax(dim=(1, 2, 3))
            print(f"S={S} table={name} flips={flips[0]}: max |err| per sample {[f'{e:.3g}' for e in err.tolist()]}, bound {bound:.3g}")
            assert float(err.max()) <= bound, (S, name, full[int(err.argmax())], float(err.max()), bound)


@pytest.mark.parametrize("S", [7, 16, 224])
def test_flip_is_the_mirror_image_bit_for_bit(gpu, S):
    cache = _cache(6, S, gpu, 200 + S)
    boxes = _boxes_for(S)
    n = len(H_IDX) * 3 * S * S
    lut = torch.from_numpy(_tables(gpu)[1][1]).to(gpu)
    outs = []
    for flip in (0, 1):
        buf, out = _guarded(n, gpu)
        assert _raw_augment(cache, H_IDX, [(*b, flip) for b in boxes], S, lut, out, gpu) == 0
        assert _outside_is_nan(buf, n)
        outs.append(out.view(len(H_IDX), 3, S, S).clone())
    assert torch.equal(outs[1].view(torch.int32), outs[0].flip(-1).view(torch.int32))
    assert not torch.equal(outs[1], outs[0])


def test_a_second_run_is_bit_identical(gpu):
    S = 224
    cache = _cache(6, S, gpu, 300)
    boxes = [(*b, k & 1) for k, b in enumerate(_boxes_for(S))]
    n = len(H_IDX) * 3 * S * S
    lut = torch.from_numpy(I.normalize_table()).to(gpu)
    runs = []
    for fill in (0.0, 1.0):
        out = torch.full((n,), fill, device=gpu)
        assert _raw_augment(cache, H_IDX, boxes, S, lut, out, gpu) == 0
        runs.append(out.view(torch.int32).cpu())
    assert torch.equal(runs[0], runs[1])


def test_refused_calls_return_an_error_and_write_nothing(gpu):
    S = 16
    cache = _cache(6, S, gpu, 400)
    lut = torch.from_numpy(I.normalize_table()).to(gpu)
    ok = (0, 0, S, S, 0)
    out = torch.full((2 * 3 * S * S + 2 * GUARD,), 7.0, device=gpu)
    target = out[GUARD:GUARD + 2 * 3 * S * S]
    cases = {"index out of range": dict(h_idx=[0, 6], boxes=[ok, ok]), "negative index": dict(h_idx=[-1, 0], boxes=[ok, ok]),
             "negative x0": dict(h_idx=[0, 1], boxes=[ok, (-1, 0, 4, 4, 0)]), "negative y0": dict(h_idx=[0, 1], boxes=[(0, -2, 4, 4, 0), ok]),
             "w = 0": dict(h_idx=[0, 1], boxes=[ok, (3, 3, 0, 4, 0)]), "h = 0": dict(h_idx=[0, 1], boxes=[ok, (3, 3, 4, 0, 0)]),
             "x0 + w > S": dict(h_idx=[0, 1], boxes=[ok, (9, 0, 8, 4, 0)]), "y0 + h > S": dict(h_idx=[0, 1], boxes=[ok, (0, 9, 4, 8, 0)]),
             "flip = 2": dict(h_idx=[0, 1], boxes=[ok, (0, 0, 4, 4, 2)]),
             "null host descriptors": dict(h_idx=[0, 1], boxes=[ok, ok], h_aug_null=True),
             "null device descriptors": dict(h_idx=[0, 1], boxes=[ok, ok], aug_null=True)}
    for what, kw in cases.items():
        rc = _raw_augment(cache, kw.pop("h_idx"), kw.pop("boxes"), S, lut, target, gpu, **kw)
        assert rc == -1, (what, rc)
        assert "d2r_clip_cache_augment" in I._lib.load().d2r_last_error().decode(), what
        assert bool((out == 7.0).all()), f"{what}: the refused call wrote"
    # the checked wrapper raises for the same arguments, and accepts valid ones
    h = torch.tensor([0, 1], dtype=torch.int64)
    bad = torch.from_numpy(_desc([ok, (9, 0, 8, 4, 0)]))
    with pytest.raises(I._lib.D2RError, match="does not lie inside"):
        I.clip_cache_augment(cache, h, h.to(gpu), bad, bad.to(gpu), S, lut, out=target)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    good = torch.from_numpy(_desc([ok, (8, 0, 8, 4, 1)]))
    I.clip_cache_augment(cache, h, h.to(gpu), good, good.to(gpu), S, lut, out=target)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(target).all()) and not bool((target == 7.0).any())
    assert bool((out[:GUARD] == 7.0).all()) and bool((out[-GUARD:] == 7.0).all())


def _trainer_hook(gpu):
    from d2r_amd.train import MSDTrainer
    trainer = MSDTrainer.__new__(MSDTrainer)  # only its _to_device hook is used
    trainer.args = type("A", (), {"device": str(gpu)})()
    return trainer


@pytest.mark.parametrize("decode", ["host", "device"])
def test_cached_loader_with_an_augmenter_yields_the_uncached_training_paths_batches(gpu, tmp_path, decode):
    """Equal seeds: over two epochs the augmented batches of the cached training loader are, bit for bit, those of the uncached
    training path (to_cache into the scratch rows, then the same kernel); the dev loader's batches stay the un-augmented ones."""
    from d2r_amd.augment import Augmenter
    from d2r_amd.cache import CachedLoader, DeviceDatasetCache, prefill, release_workers
    S = 64
    data, img, vocab = make_dir(tmp_path)
    tok = _tokenizer(vocab)
    trainer = _trainer_hook(gpu)

    plain = _loader(data, img, tok, "train", True, decode, S=S)
    aug = Augmenter(S, 0.3, 0.5, seed=17)
    torch.manual_seed(9)
    want, unaugmented = [], []
    for epoch in range(2):
        for b in plain:
            want.append(tuple(t.cpu() for t in trainer._to_device(b, aug)))
            unaugmented.append(trainer._to_device(b)[5].cpu())
    release_workers(plain)
    assert len(want) == 4 and aug._scratch.shape == (4, I.cache_row_bytes(S))
    assert all(not torch.equal(w[5], u) for w, u in zip(want, unaugmented)), "the augmenter changed nothing"
    assert all(bool(torch.isfinite(w[5]).all()) for w in want)

    wrapped = _loader(data, img, tok, "train", True, decode, S=S)
    cache = DeviceDatasetCache.for_loader(wrapped, gpu, "train")
    torch.manual_seed(9)
    prefill(wrapped, cache, split="train")
    cached = CachedLoader(wrapped, cache, Augmenter(S, 0.3, 0.5, seed=17))
    got = [tuple(t.cpu() for t in b) for epoch in range(2) for b in cached]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    # another seed gives other images; the identity settings give the plain gather's
    torch.manual_seed(9)
    other = [b[5].cpu() for b in CachedLoader(_loader(data, img, tok, "train", True, decode, S=S), cache, Augmenter(S, 0.3, 0.5, seed=18))]
    assert not torch.equal(other[0], got[0][5])
    torch.manual_seed(9)
    ident = [b[5].cpu() for b in CachedLoader(_loader(data, img, tok, "train", True, decode, S=S), cache, Augmenter(S, 1.0, 0.0, seed=17))]
    assert all(torch.equal(a, b) for a, b in zip(ident, unaugmented[:2]))

    dev_plain = _loader(data, img, tok, "dev", False, decode, S=S)
    dev_want = [tuple(t.cpu() for t in trainer._to_device(b)) for b in dev_plain]
    release_workers(dev_plain)
    dev_wrapped = _loader(data, img, tok, "dev", False, decode, S=S)
    dev_cache = DeviceDatasetCache.for_loader(dev_wrapped, gpu, "dev")
    prefill(dev_wrapped, dev_cache, split="dev")
    dev_cached = CachedLoader(dev_wrapped, dev_cache)
    assert dev_cached.augmenter is None
    for g, w in zip(list(dev_cached), dev_want):
        assert all(torch.equal(a.cpu(), b) for a, b in zip(g, w))


def _two_steps(gpu, dirs, name, augmenter):
    """Two training steps (one epoch of two batches of 4, fp32, dropout on) -> (weights, step losses, the default generator's state
    afterwards, the log lines that speak of augmentation)."""
    from d2r_amd.cache import release_workers
    from d2r_amd.train import MSDTrainer
    data, img, tok = dirs
    torch.manual_seed(31)
    torch.cuda.manual_seed_all(31)
    model, args = _small_model(torch.float32, gpu)
    args.num_epochs = 1
    logger, catch = _logger(f"augment-trainer-{name}")
    train = _loader(data, img, tok, "train", True, "host", S=64)
    tr = MSDTrainer(train_data=train, dev_data=None, test_data=None, model=model, args=args, logger=logger, writer=None,
                    augmenter=augmenter)
    tr.train(None, None)
    torch.cuda.synchronize()
    release_workers(train)
    assert tr.step == 2
    losses = [float(l.split("loss:")[1].split()[0]) for l in catch.lines if l.startswith("step ")]
    return tr.store.flat_w.clone(), losses, torch.get_rng_state(), [l for l in catch.lines if "augmentation" in l]


@pytest.fixture(scope="module")
def plain_run(gpu, tmp_path_factory):
    """The generated image directory and the run without an augmenter: computed once, shared, left unchanged."""
    data, img, vocab = make_dir(tmp_path_factory.mktemp("augment_trainer"))
    dirs = (data, img, _tokenizer(vocab))
    return dirs, _two_steps(gpu, dirs, "none", None)


def test_the_identity_augmenter_leaves_training_bit_identical(gpu, plain_run):
    from d2r_amd.augment import Augmenter
    dirs, (w0, l0, s0, a0) = plain_run
    w1, l1, s1, a1 = _two_steps(gpu, dirs, "identity", Augmenter(64, 1.0, 0.0, seed=5))
    assert len(l0) == 1 and l0 == l1 and torch.equal(w0, w1), "the identity augmenter changed the run"
    assert torch.equal(s0, s1), "the augmenter moved torch's default generator"
    assert not a0 and len(a1) == 1, (a0, a1)


def test_an_augmented_run_differs_stays_finite_and_leaves_the_default_generator_alone(gpu, plain_run):
    from d2r_amd.augment import Augmenter
    dirs, (w0, l0, s0, _) = plain_run
    w2, l2, s2, a2 = _two_steps(gpu, dirs, "augmented", Augmenter(64, 0.5, 0.5, seed=5))
    assert len(l2) == 1 and np.isfinite(l2[0]) and l2 != l0 and not torch.equal(w2, w0)
    assert bool(torch.isfinite(w2).all())
    assert torch.equal(s0, s2), "the augmenter moved torch's default generator"
    assert len(a2) == 1 and "scale [0.5, 1]" in a2[0] and "probability 0.5" in a2[0], a2
