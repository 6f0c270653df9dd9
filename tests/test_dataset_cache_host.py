"""--cache_dataset on the host: the three entry points of the device cache in the header, the library and d2r_amd._lib; their
argument checks (no launch happens); the flag and its refusal on synthetic data; the index stream and the generator consumption of
CachedLoader against the plain DataLoader; the prefill's generator save / restore and worker release with a stub backend."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import Dataset

from conftest import ROOT
from make_clip_golden import fixture_image

NEW = ("d2r_clip_cache_row_bytes", "d2r_clip_preprocess_u8", "d2r_clip_cache_gather", "d2r_gather_rows")


def _declarations():
    hdr = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name in NEW:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/d2r_hip.h"
        out[name] = (m.group(1), [a.strip() for a in m.group(2).split(",")])
    return out


def test_entry_points_are_declared_documented_and_exported():
    from d2r_amd import _lib
    decl = _declarations()
    comments = " ".join(re.findall(r"/\*.*?\*/", open(os.path.join(ROOT, "include", "d2r_hip.h")).read(), flags=re.S))
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert name in comments, f"{name} has no comment in the header"
    assert os.path.exists(_lib.LIB_PATH), "libd2r_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"{name} declared but not exported"


def test_lib_signatures_match_the_header():
    from d2r_amd import _lib

    def kind(ctype):
        if ctype in (_lib.i32,):
            return "int"
        if ctype is _lib.i64:
            return "int64_t"
        if ctype is _lib.sz:
            return "size_t"
        assert ctype is _lib.vp or issubclass(ctype, ctypes._Pointer), ctype
        return "pointer"

    for name, (ret, args) in _declarations().items():
        res, argtypes = _lib.SIGNATURES[name]
        assert kind(res) == ret, (name, ret)
        want = ["pointer" if "*" in a else a.split()[-2] for a in args]
        assert [kind(t) for t in argtypes] == want, (name, want)
    # the host descriptor is typed, as in d2r_clip_preprocess
    assert _lib.SIGNATURES["d2r_clip_preprocess_u8"][1][2] == ctypes.POINTER(_lib.ClipImageDesc)


@pytest.mark.parametrize("S,want", [(224, 150528), (30, 2704), (1, 16), (4, 48), (31, 2896)])
def test_cache_row_bytes(S, want):
    from d2r_amd import image as I
    assert I.cache_row_bytes(S) == want == -(-3 * S * S // 16) * 16


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Slots and indices are checked on their host copies: these calls are refused and never reach a launch (the device pointers
    are dummies; nothing is dereferenced)."""
    from d2r_amd import image as I
    lib = I._lib.load()
    pixels, desc, tab = I.plan_batch([fixture_image(1, 480, 640), fixture_image(2, 80, 100)], 224, 224)
    fake = 1 << 20
    hd = ctypes.cast(desc.ctypes.data, ctypes.POINTER(I._lib.ClipImageDesc))
    need = lib.d2r_clip_preprocess_ws_bytes(hd, 2, 224)

    def u8(slots, rows=10, d=desc, ws=need):
        h = np.asarray(slots, np.int64)
        rc = lib.d2r_clip_preprocess_u8(fake, pixels.size, ctypes.cast(d.ctypes.data, ctypes.POINTER(I._lib.ClipImageDesc)), fake, 2, 224,
                                        tab.ctypes.data, fake, tab.size, fake, rows, h.ctypes.data, fake, fake, ws, None)
        return rc, lib.d2r_last_error().decode()

    for slots, msg in (([0, 10], "outside the 10 rows"), ([-1, 3], "outside the 10 rows"), ([4, 4], "named twice")):
        rc, err = u8(slots)
        assert rc == -1 and msg in err, (slots, rc, err)
    d = desc.copy(); d[1]["src_offset"] += 1
    rc, err = u8([0, 1], d=d)
    assert rc == -1 and "outside the" in err  # the descriptor checks of d2r_clip_preprocess
    rc, err = u8([0, 1], ws=need - 1)
    assert rc == -3 and "workspace" in err
    assert lib.d2r_clip_preprocess_u8(fake, pixels.size, hd, fake, 2, 224, tab.ctypes.data, fake, tab.size, None, 10,
                                      np.zeros(2, np.int64).ctypes.data, fake, fake, need, None) == -1

    def gather(idx, rows=5, cache=fake):
        h = np.asarray(idx, np.int64)
        rc = lib.d2r_clip_cache_gather(cache, rows, h.ctypes.data, fake, len(h), 224, fake, fake, None)
        return rc, lib.d2r_last_error().decode()

    for idx in ([0, 5], [-1], [2, 2, 7]):
        rc, err = gather(idx)
        assert rc == -1 and "outside the 5 rows" in err, (idx, err)
    rc, err = gather([0], cache=fake + 8)
    assert rc == -1 and "aligned" in err

    def rows(idx, n=5, row_bytes=8):
        h = np.asarray(idx, np.int64)
        rc = lib.d2r_gather_rows(fake, 2 * fake, n, row_bytes, h.ctypes.data, fake, len(h), None)
        return rc, lib.d2r_last_error().decode()

    for idx in ([5], [0, -2]):
        rc, err = rows(idx)
        assert rc == -1 and "outside the 5 rows" in err, (idx, err)
    assert rows([0], row_bytes=0)[0] == -1


def test_flag_parsing_and_refusal_on_synthetic_data():
    from d2r_amd.run import build_parser, main
    p = build_parser()
    assert p.parse_args([]).cache_dataset == "off"
    assert p.parse_args(["--cache_dataset", "device"]).cache_dataset == "device"
    assert p.parse_args(["--cache_dataset", "off"]).cache_dataset == "off"
    with pytest.raises(SystemExit):
        p.parse_args(["--cache_dataset", "host"])
    with pytest.raises(SystemExit, match="synthetic"):
        main(["--cache_dataset", "device"])


def test_allocation_that_does_not_fit_names_the_split_and_the_bytes():
    from d2r_amd import cache as K
    assert K.cache_bytes(4511, 128, 224) == 4511 * (150528 + 3 * 8 * 128 + 8)
    K.check_fit([("train", 100), ("dev", 50)], 150)
    with pytest.raises(SystemExit, match=r"the dev split needs 50 bytes.*149 bytes are free"):
        K.check_fit([("train", 100), ("dev", 50), ("test", 1)], 149)


class _Idx(Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class _StubCache:
    """Stands in for DeviceDatasetCache where no device is: gather hands the index batch back."""
    device = torch.device("cpu")

    def gather(self, h_idx, idx):
        return h_idx


def _loaders(kind, workers):
    from d2r_amd.data import make_loader
    ds = _Idx(37)
    if kind == "shuffle":
        return make_loader(ds, 5, True, workers, drop_last=True), make_loader(ds, 5, True, workers, drop_last=True)
    if kind == "sequential":
        return make_loader(ds, 5, False, workers), make_loader(ds, 5, False, workers)
    mk = lambda: torch.utils.data.distributed.DistributedSampler(ds, num_replicas=2, rank=1, shuffle=True, seed=2023)
    return make_loader(ds, 5, True, workers, drop_last=True, sampler=mk()), make_loader(ds, 5, True, workers, drop_last=True, sampler=mk())


@pytest.mark.parametrize("workers", [0, 2], ids=["in_process", "persistent_workers"])
@pytest.mark.parametrize("kind", ["shuffle", "sequential", "distributed"])
def test_cached_loader_draws_the_plain_loaders_indices_and_generator_state(kind, workers):
    """Per epoch: the same index batches as the plain DataLoader feeds its dataset, and the same state of torch's default
    generator afterwards (a DataLoader draws a base seed per iterator - once with persistent workers - and RandomSampler a seed
    per epoch), with the dropout-seed draws of a training step interleaved as the trainer interleaves them."""
    from d2r_amd.cache import CachedLoader, release_workers
    plain, wrapped = _loaders(kind, workers)
    cached = CachedLoader(wrapped, _StubCache())
    assert len(cached) == len(plain) and cached.dataset is wrapped.dataset and cached.sampler is wrapped.sampler
    assert cached.batch_sampler is wrapped.batch_sampler and cached.batch_size == 5

    def run(loader):
        torch.manual_seed(77)
        seen, states = [], []
        for epoch in range(1, 4):
            if hasattr(loader.sampler, "set_epoch"):
                loader.sampler.set_epoch(epoch)
            for batch in loader:
                seen.append(batch.tolist())
                torch.empty((), dtype=torch.int64).random_()  # a step's dropout seed
            states.append(torch.get_rng_state())
        return seen, states

    try:
        want, want_states = run(plain)
        got, got_states = run(cached)
    finally:
        release_workers(plain)
    assert got == want
    assert len(want) == 3 * len(plain) and (kind == "sequential" or want[:len(plain)] != want[len(plain):2 * len(plain)])
    for a, b in zip(got_states, want_states):
        assert torch.equal(a, b)
    assert getattr(wrapped, "_iterator", None) is None  # the wrapped loader itself was never iterated: it has no workers


class _Samples(Dataset):
    max_seq = 4

    def __init__(self, n):
        self.n, self.fallbacks = n, 0

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if i % 3 == 0:
            self.fallbacks += 1
        torch.rand(1)  # a dataset that draws from the default generator (in process: from the parent's)
        row = torch.full((4,), i)
        return row, row + 1, row + 2, torch.ones(2, dtype=torch.long), torch.tensor(i % 3), torch.full((3,), float(i))


class _Recorder:
    n, nbytes = 11, 0

    def __init__(self):
        self.batches, self.finished, self.fallbacks = [], False, 0

    def fill(self, batch):
        torch.rand(3)  # a backend that disturbs the generator too
        self.batches.append(batch)
        self.fallbacks += batch[5].fallbacks

    def finish(self):
        self.finished = True


@pytest.mark.parametrize("workers", [0, 2])
def test_prefill_is_sequential_complete_and_leaves_the_generator_alone(workers):
    import multiprocessing
    from d2r_amd.cache import IndexedImages, prefill
    from d2r_amd.data import make_loader
    dl = make_loader(_Samples(11), 4, True, workers, drop_last=True, collate_fn=torch.utils.data.default_collate)
    if workers:
        next(iter(dl))  # the loader now keeps persistent workers
        assert len(multiprocessing.active_children()) >= workers
    torch.manual_seed(5)
    before = torch.get_rng_state()
    rec = _Recorder()
    prefill(dl, rec, split="train")
    assert torch.equal(torch.get_rng_state(), before)
    assert rec.finished and [len(b[5]) for b in rec.batches] == [4, 4, 3]  # drop_last=False: the short batch is there
    assert torch.cat([b[5].indices for b in rec.batches]).tolist() == list(range(11))  # unshuffled
    for b in rec.batches:
        assert len(b) == 6 and isinstance(b[5], IndexedImages)
        assert torch.equal(b[0][:, 0], b[5].indices) and torch.equal(b[5].packed[:, 0], b[5].indices.float())
    assert rec.fallbacks == 4  # samples 0, 3, 6, 9: counted in the workers, carried back with the batches
    assert not multiprocessing.active_children(), "worker processes survived the prefill"
    assert getattr(dl, "_iterator", None) is None

    class Failing(_Recorder):
        def fill(self, batch):
            torch.rand(2)
            raise RuntimeError("boom")

    with pytest.raises(RuntimeError, match="boom"):
        prefill(dl, Failing(), split="train")
    assert torch.equal(torch.get_rng_state(), before) and not multiprocessing.active_children()


def test_decode_log_counts_cached_batches():
    import logging
    from d2r_amd.cache import CachedBatch
    from d2r_amd.jpeg import DecodeLog
    lines = []

    class Catch(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())

    logger = logging.getLogger("cache-host-test")
    logger.addHandler(Catch())
    logger.setLevel(logging.INFO)
    log = DecodeLog(logger)
    for n in (4, 4, 3):
        b = CachedBatch((torch.zeros(n),) * 6)
        b.cached_images = n
        assert len(b) == 6
        log.note(b)
    log.note((torch.zeros(2),) * 6)  # a plain batch counts nothing
    log.end_epoch(2)
    assert lines == ["epoch 2 images: 11 images from the device cache"]
    log.end_epoch(3)
    assert len(lines) == 1
