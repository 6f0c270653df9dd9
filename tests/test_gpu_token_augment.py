"""Text augmentation on the MI355X (K23): d2r_token_augment through the raw C ABI (the identity plan against three d2r_gather_rows,
random plans against text_augment.token_augment_reference with the row lengths on the 64-position chunk boundaries, determinism,
refusals; sentinels round every output), the batches of a CachedLoader with a TokenAugmenter against the uncached training path,
training steps with and without one, and the command line.  Everything is an integer: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from test_gpu_dataset_cache import _cli, _loader, _logger, _small_model, _tokenizer, make_dir

from d2r_amd import image as I
from d2r_amd import text_augment as T

pytestmark = pytest.mark.gpu

GUARD = 512            # int64 sentinels before, between and after the three outputs
SENTINEL = -0x5A5A5A5A5A5A5A5B
VOCAB, MASK_ID = 1000, 103
K, D, M, R = T.KEEP, T.DELETE, T.MASK, T.REPLACE


def _cont_table(seed=1):
    """About 40 % of the ids are continuations; 7 is not, 8 is."""
    cont = (np.random.default_rng(seed).random(VOCAB) < 0.4).astype(np.uint8)
    cont[7], cont[8] = 0, 1
    return cont


class _Outputs:
    """out_ids, out_mask, out_seg [B, L] inside one int64 buffer of sentinels: [GUARD | ids | GUARD | mask | GUARD | seg | GUARD]."""

    def __init__(self, B, L, gpu, fill=SENTINEL):
        self.n, self.fill = B * L, fill
        self.buf = torch.full((3 * self.n + 4 * GUARD,), fill, dtype=torch.int64, device=gpu)
        self.views = [self.buf[GUARD + k * (self.n + GUARD):GUARD + k * (self.n + GUARD) + self.n].view(B, L) for k in range(3)]

    def guards_intact(self):
        return all(bool((self.buf[k * (self.n + GUARD):k * (self.n + GUARD) + GUARD] == self.fill).all()) for k in range(4))

    def untouched(self):
        return bool((self.buf == self.fill).all())

    def numpy(self):
        return [v.cpu().numpy() for v in self.views]


def _raw(src, h_idx, plan, cont, out, gpu, pad_id=0, vocab=VOCAB, mask_id=MASK_ID, L=None, rows=None, outs=None):
    """d2r_token_augment through ctypes on torch's current stream, synchronised -> its status.  src: the three [rows, L] device
    tensors; plan: numpy uint32 [B, L]; cont: a device tensor or None.  The device copy of idx is clamped into the rows."""
    from d2r_amd.functional import _stream
    lib = I._lib.load()
    h = np.ascontiguousarray(h_idx, dtype=np.int64)
    hp = np.ascontiguousarray(plan, dtype=np.uint32)
    idx = torch.from_numpy(h).clamp(0, src[0].shape[0] - 1).to(gpu)
    d_plan = torch.from_numpy(hp.view(np.int32)).to(gpu)
    o = outs or [v.data_ptr() for v in out.views]
    rc = I._lib._FN["d2r_token_augment"](src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), src[0].shape[0] if rows is None else rows,
                                         src[0].shape[1] if L is None else L, h.ctypes.data, idx.data_ptr(), hp.ctypes.data,
                                         d_plan.data_ptr(), len(h), None if cont is None else cont.data_ptr(), vocab, mask_id, pad_id,
                                         o[0], o[1], o[2], _stream())
    torch.cuda.synchronize()
    return rc, lib.d2r_last_error().decode()


def _row(rng, L, n, lo=0, hi=VOCAB):
    """A source row with n real tokens: ids [CLS]=101 ... [SEP]=102, padding 0 / 0 / 0, random seg values on the real tokens."""
    ids, mask, seg = np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L, np.int64)
    ids[:n] = rng.integers(lo, hi, n)
    if n >= 1:
        ids[0] = 101
    if n >= 2:
        ids[n - 1] = 102
    mask[:n] = 1
    seg[:n] = rng.integers(0, 5, n)
    return ids, mask, seg


@pytest.mark.parametrize("L", [16, 128])
def test_identity_plan_is_three_gather_rows_bit_for_bit(gpu, L):
    rng = np.random.default_rng(L)
    lengths = [L, 2, 3, L // 2, L - 1, 5, 1]  # a 7-row source
    rows = [_row(rng, L, n) for n in lengths]
    src = [torch.from_numpy(np.stack([r[k] for r in rows])).to(gpu) for k in range(3)]
    h_idx = np.array([3, 0, 6, 3, 3, 5, 1, 2, 4, 6, 0], np.int64)  # repeated and permuted
    h = torch.from_numpy(h_idx)
    want = [I.gather_rows(t, h, h.to(gpu)).cpu().numpy() for t in src]
    plan = np.zeros((len(h_idx), L), np.uint32)
    for cont in (None, torch.from_numpy(_cont_table()).to(gpu)):
        out = _Outputs(len(h_idx), L, gpu)
        rc, err = _raw(src, h_idx, plan, cont, out, gpu)
        assert rc == 0, err
        assert out.guards_intact(), "write outside the outputs"
        for got, w, name in zip(out.numpy(), want, ("ids", "mask", "seg")):
            assert np.array_equal(got, w), (name, cont is not None)


def _cases(L, rng):
    """Source rows and plans for row length L -> (rows, plans, names).  The row lengths sit on the chunk boundaries; with L > 66
    there are a word whose pieces straddle positions 63 | 64, a head at 64 after a piece at 63, a row where everything is deleted and
    one where all but the last content token is."""
    rows, plans, names = [], [], []

    def random_plan():
        u = rng.random(L)
        op = np.where(u < 0.3, D, np.where(u < 0.5, M, np.where(u < 0.7, R, K))).astype(np.uint32)
        return op | (rng.integers(0, VOCAB, L).astype(np.uint32) << 2)  # every word carries an id: pieces replaced through their head

    for n in sorted({n for n in (2, 3, 63, 64, 65, 66, L) if n <= L}):
        rows.append(_row(rng, L, n))
        plans.append(random_plan())
        names.append(f"n={n}")
    if L >= 3:  # ids outside [0, vocab) act as heads and are copied as they are
        n = min(L, 40)
        row = _row(rng, L, n, -50, VOCAB + 50)
        rows.append(row)
        plans.append(random_plan())
        names.append("ids outside the vocabulary")
    if L > 66:
        n = min(L, 70)
        for name, at62, at63, at64, at65 in (("a word straddles 63 | 64", 8, 7, 8, 8), ("a head at 64", 7, 8, 7, 8)):
            for op63, op64 in ((D, K), (M, D), (R, K), (K, D)):
                ids, mask, seg = _row(rng, L, n)
                ids[62:66] = (at62, at63, at64, at65)  # 7 starts a word, 8 continues one
                plan = random_plan()
                plan[63] = op63 | (plan[63] & ~np.uint32(3))
                plan[64] = op64 | (plan[64] & ~np.uint32(3))
                rows.append((ids, mask, seg))
                plans.append(plan)
                names.append(f"{name}, ops {op63} {op64}")
    for n in sorted({min(L, 100), L}):
        if n >= 3:
            rows.append(_row(rng, L, n))
            plans.append(np.full(L, D, np.uint32))
            names.append(f"everything deleted, n={n}")
        if n >= 4:
            ids, mask, seg = _row(rng, L, n)
            ids[n - 2] = 7  # a head: it survives on its own with the table too
            plan = np.full(L, D, np.uint32)
            plan[n - 2] = K
            rows.append((ids, mask, seg))
            plans.append(plan)
            names.append(f"all but the last content token deleted, n={n}")
    return rows, plans, names


@pytest.mark.parametrize("L", [3, 63, 64, 65, 130, 512, 1024])
def test_random_plans_against_the_reference_model(gpu, L):
    B = 5
    table = _cont_table()
    d_table = torch.from_numpy(table).to(gpu)
    rows, plans, names = _cases(L, np.random.default_rng(1000 + L))
    lengths = {int(r[1].sum()) for r in rows}
    assert lengths >= {n for n in (2, 3, 63, 64, 65, 66, L) if n <= L}
    assert L <= 66 or (any("straddles" in n for n in names) and any("head at 64" in n for n in names))
    assert L < 4 or (any("everything deleted" in n for n in names) and any("all but the last" in n for n in names))
    host = [np.stack([r[k] for r in rows]) for k in range(3)]
    src = [torch.from_numpy(t).to(gpu) for t in host]
    order = np.random.default_rng(L).permutation(len(rows))
    order = np.concatenate([order, order[:(-len(order)) % B]])  # whole batches of 5; the last one repeats rows
    checked = 0
    for start in range(0, len(order), B):
        h_idx = order[start:start + B]
        plan = np.stack([plans[r] for r in h_idx])
        for cont, d_cont in ((None, None), (table, d_table)):
            want = T.token_augment_reference(*host, h_idx, plan, cont, VOCAB, MASK_ID, 0)
            out = _Outputs(B, L, gpu)
            rc, err = _raw(src, h_idx, plan, d_cont, out, gpu)
            assert rc == 0, err
            assert out.guards_intact(), "write outside the outputs"
            for got, w, name in zip(out.numpy(), want, ("ids", "mask", "seg")):
                bad = np.flatnonzero((got != w).any(axis=1))
                assert bad.size == 0, (name, "cont" if cont is not None else "no cont", [names[h_idx[b]] for b in bad],
                                       got[bad[0]].tolist(), w[bad[0]].tolist())
            checked += B
    assert checked >= 2 * len(rows)
    # the special rows do what their names say (on the reference, which the kernel equals)
    for r, name in enumerate(names):
        n = int(rows[r][1].sum())
        for cont in (None, table):
            o = T.token_augment_reference(*host, [r], plans[r][None], cont, VOCAB, MASK_ID, 0)
            if name.startswith("everything deleted"):
                assert np.array_equal(o[0][0], rows[r][0]) and int(o[1].sum()) == n
            if name.startswith("all but the last"):
                assert int(o[1].sum()) == 3 and o[0][0, 1] == 7


def test_a_second_run_is_bit_identical(gpu):
    L, B = 130, 5
    table = torch.from_numpy(_cont_table()).to(gpu)
    rows, plans, _ = _cases(L, np.random.default_rng(77))
    src = [torch.from_numpy(np.stack([r[k] for r in rows])).to(gpu) for k in range(3)]
    h_idx = np.arange(B) * 2
    plan = np.stack([plans[r] for r in h_idx])
    runs = []
    for fill in (SENTINEL, 0):
        out = _Outputs(B, L, gpu, fill)
        rc, err = _raw(src, h_idx, plan, table, out, gpu)
        assert rc == 0, err
        runs.append(out.numpy())
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_refused_calls_return_an_error_and_write_nothing(gpu):
    L, B = 16, 2
    rng = np.random.default_rng(3)
    rows = [_row(rng, L, n) for n in (16, 9, 2, 12)]
    src = [torch.from_numpy(np.stack([r[k] for r in rows])).to(gpu) for k in range(3)]
    table = torch.from_numpy(_cont_table()).to(gpu)
    out = _Outputs(B, L, gpu)
    ok = np.full((B, L), D, np.uint32)
    bad_id, stray_id = ok.copy(), ok.copy()
    bad_id[1, 5] = R | (VOCAB << 2)
    stray_id[0, 3] = K | (VOCAB << 2)
    o = [v.data_ptr() for v in out.views]
    cases = {"index out of range": dict(h_idx=[0, 4]), "negative index": dict(h_idx=[-1, 0]),
             "replacement id >= vocab": dict(plan=bad_id), "an id >= vocab at a kept position": dict(plan=stray_id),
             "L = 1": dict(L=1), "L = 1025": dict(L=1025), "rows = 0": dict(rows=0), "vocab = 0": dict(vocab=0),
             "mask id = vocab": dict(mask_id=VOCAB), "pad id < 0": dict(pad_id=-1),
             "out_ids unaligned": dict(outs=[o[0] + 4, o[1], o[2]]), "out_mask is ids": dict(outs=[o[0], src[0].data_ptr(), o[2]]),
             "out_seg overlaps out_mask": dict(outs=[o[0], o[1], o[1] + 8]), "null out_seg": dict(outs=[o[0], o[1], None])}
    before = [t.clone() for t in src]
    for what, kw in cases.items():
        rc, err = _raw(src, kw.pop("h_idx", [0, 1]), kw.pop("plan", ok), table, out, gpu, **kw)
        assert rc < 0 and "d2r_token_augment" in err, (what, rc, err)
        assert out.untouched(), f"{what}: the refused call wrote"
        assert all(torch.equal(a, b) for a, b in zip(src, before)), f"{what}: the refused call wrote into its inputs"
    # the checked wrapper raises for the same arguments, and the valid call writes all of the outputs and nothing else
    h = torch.tensor([0, 1], dtype=torch.int64)
    hp = torch.from_numpy(bad_id.view(np.int32))
    with pytest.raises(I._lib.D2RError, match="replacement id"):
        T.token_augment(*src, h, h.to(gpu), hp, hp.to(gpu), table, VOCAB, MASK_ID, 0)
    torch.cuda.synchronize()
    assert out.untouched()
    rc, err = _raw(src, [0, 1], ok, table, out, gpu)
    assert rc == 0, err
    assert out.guards_intact() and not any(bool((v == SENTINEL).any()) for v in out.views)


def _trainer_hook(gpu):
    from d2r_amd.train import MSDTrainer
    trainer = MSDTrainer.__new__(MSDTrainer)  # only its _to_device hook is used
    trainer.args = type("A", (), {"device": str(gpu)})()
    return trainer


def _text_augmenter(tok, delete_p, mask_p, replace_p, seed, whole_word=True):
    from d2r_amd.run import token_settings
    return T.TokenAugmenter(delete_p, mask_p, replace_p, seed=seed, **token_settings(tok, whole_word, True))


def test_cached_loader_with_a_text_augmenter_yields_the_uncached_training_paths_batches(gpu, tmp_path):
    """Equal seeds: over two epochs the token tensors (and everything else) of the cached training loader are, bit for bit, those of
    the uncached training path, and both are the reference model's view of the un-augmented rows under the plans a twin augmenter
    draws; the dev loader's batches stay the un-augmented ones."""
    from d2r_amd.cache import CachedLoader, DeviceDatasetCache, prefill, release_workers
    S = 64
    data, img, vocab = make_dir(tmp_path)
    tok = _tokenizer(vocab)
    trainer = _trainer_hook(gpu)
    table = T.continuation_table(tok)

    plain = _loader(data, img, tok, "train", True, "host", S=S)
    aug, twin = _text_augmenter(tok, 0.3, 0.2, 0.2, 17), _text_augmenter(tok, 0.3, 0.2, 0.2, 17)
    torch.manual_seed(9)
    want, changed = [], 0
    for epoch in range(2):
        for b in plain:
            got = tuple(t.cpu() for t in trainer._to_device(b, None, aug))
            plan = twin.draw(4, 16).numpy()
            ref = T.token_augment_reference(b[0].numpy(), b[1].numpy(), b[2].numpy(), np.arange(4), plan, table, len(tok), 4, 0)
            for k in range(3):
                assert got[k].dtype == torch.int64 and np.array_equal(got[k].numpy(), ref[k]), k
            assert torch.equal(got[4], b[4])
            changed += int((got[0] != b[0]).any())
            want.append(got)
    release_workers(plain)
    assert len(want) == 4 and changed >= 3, "the augmenter changed next to nothing"

    wrapped = _loader(data, img, tok, "train", True, "host", S=S)
    cache = DeviceDatasetCache.for_loader(wrapped, gpu, "train")
    torch.manual_seed(9)
    prefill(wrapped, cache, split="train")
    cached = CachedLoader(wrapped, cache, text_augmenter=_text_augmenter(tok, 0.3, 0.2, 0.2, 17))
    got = [tuple(t.cpu() for t in b) for epoch in range(2) for b in cached]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    # an all-off augmenter gives the plain gather's batches
    torch.manual_seed(9)
    off = [b for b in CachedLoader(_loader(data, img, tok, "train", True, "host", S=S), cache, text_augmenter=_text_augmenter(tok, 0, 0, 0, 17))]
    torch.manual_seed(9)
    none = [b for b in CachedLoader(_loader(data, img, tok, "train", True, "host", S=S), cache)]
    assert all(torch.equal(x, y) for a, b in zip(off, none) for x, y in zip(a, b))

    dev_wrapped = _loader(data, img, tok, "dev", False, "host", S=S)
    dev_cache = DeviceDatasetCache.for_loader(dev_wrapped, gpu, "dev")
    prefill(dev_wrapped, dev_cache, split="dev")
    dev_cached = CachedLoader(dev_wrapped, dev_cache)
    assert dev_cached.text_augmenter is None
    dev_ds, at = dev_wrapped.dataset, 0
    for b in dev_cached:
        for k in range(b[0].shape[0]):
            for got, w in zip(b[:3], dev_ds.encode(dev_ds.texts[at])):
                assert torch.equal(got[k].cpu(), w)
            at += 1
    assert at == len(dev_ds)

    # "dogs , cats" = dog ##s , cat ##s under deletion of whole words: a word and its piece vanish or survive together
    ds = wrapped.dataset
    ids, mask, seg = ds.encode("dogs , cats")
    dog, cat, s, comma = (tok.convert_tokens_to_ids(t) for t in ("dog", "cat", "##s", ","))
    assert ids[:7].tolist() == [2, dog, s, comma, cat, s, 3]
    B = 64
    batch = [t[None].expand(B, -1).contiguous().to(gpu) for t in (ids, mask, seg)]
    out_ids, out_mask, _ = _text_augmenter(tok, 0.5, 0.0, 0.0, 3).apply_batch(*batch)

    def leftover(words):  # whole words only: nothing is left once "dog ##s", "cat ##s" and "," are taken out
        text = " ".join(map(str, words))
        for w in (f"{dog} {s}", f"{cat} {s}", str(comma)):
            text = text.replace(w, "")
        return text.strip()

    seen = set()
    for row, m in zip(out_ids.cpu().tolist(), out_mask.sum(1).cpu().tolist()):
        words = row[1:m - 1]
        assert row[0] == 2 and row[m - 1] == 3 and len(words) >= 1 and all(t == 0 for t in row[m:])
        assert not leftover(words), row
        seen.add(tuple(words))
    assert (dog, s, comma, cat, s) in seen and len(seen) >= 5, seen
    # piece by piece the words do come apart
    out_ids, out_mask, _ = _text_augmenter(tok, 0.5, 0.0, 0.0, 3, whole_word=False).apply_batch(*batch)
    assert any(leftover(row[1:m - 1]) for row, m in zip(out_ids.cpu().tolist(), out_mask.sum(1).cpu().tolist()))


def _image_augmenter():
    from d2r_amd.augment import Augmenter
    return Augmenter(64, 0.5, 0.5, seed=5, brightness=0.2)


def _two_steps(gpu, dirs, name, text_augmenter):
    """Two training steps (one epoch of two batches of 4, fp32, dropout on) with an image augmenter, a dev and a test pass -> (weights, step losses, the
    default generator's state afterwards, the image augmenter's two generator states, the log lines that speak of text augmentation)."""
    from d2r_amd.cache import release_workers
    from d2r_amd.train import MSDTrainer
    data, img, tok = dirs
    torch.manual_seed(31)
    torch.cuda.manual_seed_all(31)
    model, args = _small_model(torch.float32, gpu)
    args.num_epochs = 1
    logger, catch = _logger(f"text-augment-trainer-{name}")
    # in-process loaders: the runs compared here differ in the text augmenter alone, and worker processes cost seconds to start
    loaders = [_loader(data, img, tok, split, split == "train", "host", S=64, workers=0) for split in ("train", "dev", "test")]
    image_augmenter = _image_augmenter()
    more = {} if text_augmenter is None else {"text_augmenter": text_augmenter}
    tr = MSDTrainer(train_data=loaders[0], dev_data=loaders[1], test_data=loaders[2], model=model, args=args, logger=logger,
                    writer=None, augmenter=image_augmenter, **more)
    tr.train(None, None)
    torch.cuda.synchronize()
    for dl in loaders:
        release_workers(dl)
    assert tr.step == 2 and tr.last_dev_result is not None and tr.last_test_result is not None
    losses = [float(l.split("loss:")[1].split()[0]) for l in catch.lines if l.startswith("step ")]
    return (tr.store.flat_w.clone(), losses, torch.get_rng_state(),
            (image_augmenter.generator.get_state(), image_augmenter.photo_generator.get_state()),
            [l for l in catch.lines if "Text augmentation" in l])


@pytest.fixture(scope="module")
def plain_run(gpu, tmp_path_factory):
    """The generated directory and the run without a text augmenter: computed once, shared, left unchanged."""
    data, img, vocab = make_dir(tmp_path_factory.mktemp("text_augment_trainer"))
    dirs = (data, img, _tokenizer(vocab))
    return dirs, _two_steps(gpu, dirs, "none", None)


def test_an_all_off_text_augmenter_leaves_training_bit_identical(gpu, plain_run):
    dirs, (w0, l0, s0, i0, a0) = plain_run
    w1, l1, s1, i1, a1 = _two_steps(gpu, dirs, "off", _text_augmenter(dirs[2], 0.0, 0.0, 0.0, 5))
    assert len(l0) == 1 and l0 == l1 and torch.equal(w0, w1), "the all-off text augmenter changed the run"
    assert torch.equal(s0, s1), "the text augmenter moved torch's default generator"
    assert all(torch.equal(a, b) for a, b in zip(i0, i1)), "the text augmenter moved the image augmenter's streams"
    assert not a0 and len(a1) == 1, (a0, a1)


def test_an_augmented_run_differs_stays_finite_and_touches_nothing_else(gpu, plain_run):
    dirs, (w0, l0, s0, i0, _) = plain_run
    aug, twin = _text_augmenter(dirs[2], 0.3, 0.2, 0.2, 5), _text_augmenter(dirs[2], 0.3, 0.2, 0.2, 5)
    calls = []
    apply_batch = aug.apply_batch
    aug.apply_batch = lambda *a: (calls.append(a[0].shape), apply_batch(*a))[1]
    w2, l2, s2, i2, a2 = _two_steps(gpu, dirs, "augmented", aug)
    assert len(l2) == 1 and np.isfinite(l2[0]) and l2 != l0 and not torch.equal(w2, w0)
    assert bool(torch.isfinite(w2).all())
    assert torch.equal(s0, s2), "the text augmenter moved torch's default generator"
    assert all(torch.equal(a, b) for a, b in zip(i0, i2)), "the text augmenter moved the image augmenter's streams"
    assert len(a2) == 1 and "probability 0.3" in a2[0] and "whole words" in a2[0], a2
    # the dev and test passes never augment: two draws in all, one per training batch
    assert calls == [torch.Size([4, 16])] * 2, calls
    twin.draw(4, 16), twin.draw(4, 16)
    assert torch.equal(aug.generator.get_state(), twin.generator.get_state())


def test_cli_augments_synthetic_training_and_ignores_the_flags_with_only_test(gpu, tmp_path):
    flags = ["--aug_token_delete", "0.1", "--aug_token_mask", "0.1", "--aug_token_replace", "0.05"]
    tiny = ["--train_samples", "16", "--eval_samples", "8", "--batch_size", "8", "--encoder_layers", "1", "--image_size", "64",
            "--max_seq", "16", "--num_workers", "0", "--dtype", "bf16"]
    log = _cli(["--num_epochs", "1", *flags, *tiny], tmp_path, timeout=300)
    line = T.TokenAugmenter(0.1, 0.1, 0.05, 103, 0, 30522, replace_range=(1000, 30000)).describe()
    assert "Text augmentation of the training batches: " + line in log, log[-3000:]
    assert "Test Eval results" in log
    ck = str(tmp_path / "out" / "best_model.pth")
    assert os.path.exists(ck)
    log = _cli(["--only_test", "--load_path", ck, *flags, *tiny], tmp_path, timeout=300)
    assert "--aug_token_delete / --aug_token_mask / --aug_token_replace / --aug_whole_word are ignored with --only_test" in log
    assert "Text augmentation" not in log and "Running prediction" in log
