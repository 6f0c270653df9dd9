"""Text augmentation on the host (K23): token_augment_reference against hand-written rows, the plans TokenAugmenter.draw produces and
its generator, text_stream_seed against the other streams' seeds, d2r_token_augment in the header, the library and d2r_amd._lib with
every host refusal through the raw C ABI (fake device pointers, no launch happens), the command-line flags and the continuation table
of the tiny test vocabulary."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_clip_data import VOCAB

CLS, SEP, MASK_ID, V = 2, 3, 4, 20  # the tiny vocabulary's [CLS], [SEP], [MASK]; 20 ids, "##s" is id 16
CONT = np.zeros(V, np.uint8)
CONT[16] = 1
K, D, M, R = 0, 1, 2, 3


def rep(t):
    return R | (t << 2)


def _one(ids, n, plan, cont=None, pad_id=0, seg=None, vocab=V):
    """One row through the reference: ids (any length L), the first n real; plan by position -> the three output rows as lists."""
    from d2r_amd.text_augment import token_augment_reference
    L = len(ids)
    mask = [1] * n + [0] * (L - n)
    seg = seg if seg is not None else [0] * L
    out = token_augment_reference(np.array([ids]), np.array([mask]), np.array([seg]), np.array([0]), np.array([plan], np.uint32), cont,
                                  vocab, MASK_ID, pad_id)
    assert all(o.shape == (1, L) and o.dtype == np.int64 for o in out)
    return tuple(o[0].tolist() for o in out)


def test_reference_keep_delete_mask_replace_and_seg_follows_its_token():
    # [CLS] 5 6 7 8 [SEP] pad pad: keep 5, delete 6, mask 7, replace 8 by 9; the ops at [CLS], [SEP] and the padding are ignored
    ids, mask, seg = _one([CLS, 5, 6, 7, 8, SEP, 0, 0], 6, [D, K, D, M, rep(9), D, D, rep(7)], seg=[10, 11, 12, 13, 14, 15, 0, 0])
    assert ids == [CLS, 5, MASK_ID, 9, SEP, 0, 0, 0]
    assert mask == [1, 1, 1, 1, 1, 0, 0, 0]
    assert seg == [10, 11, 13, 14, 15, 0, 0, 0]
    # the identity plan
    ids, mask, seg = _one([CLS, 5, 6, 7, 8, SEP, 0, 0], 6, [K] * 8, seg=[0, 0, 0, 1, 1, 1, 0, 0])
    assert ids == [CLS, 5, 6, 7, 8, SEP, 0, 0] and mask == [1] * 6 + [0, 0] and seg == [0, 0, 0, 1, 1, 1, 0, 0]


def test_reference_short_and_full_rows_and_the_padding():
    # n = 2: no content position, the row comes out unchanged whatever the plan says
    assert _one([CLS, SEP, 0, 0], 2, [D, D, D, D])[0] == [CLS, SEP, 0, 0]
    assert _one([CLS, SEP, 0, 0], 2, [M, M, M, M])[:2] == ([CLS, SEP, 0, 0], [1, 1, 0, 0])
    # n = 3: the one content token is masked, replaced - or, deleted, kept by the keep-one rule
    assert _one([CLS, 7, SEP, 0], 3, [K, M, K, K])[0] == [CLS, MASK_ID, SEP, 0]
    assert _one([CLS, 7, SEP, 0], 3, [K, rep(19), K, K])[0] == [CLS, 19, SEP, 0]
    assert _one([CLS, 7, SEP, 0], 3, [K, D, K, K])[:2] == ([CLS, 7, SEP, 0], [1, 1, 1, 0])
    # n = 1 and n = 0 (not written by the data layer, inside the function all the same)
    assert _one([CLS, 0, 0], 1, [D, D, D])[:2] == ([CLS, 0, 0], [1, 0, 0])
    assert _one([0, 0, 0], 0, [D, D, D])[:2] == ([0, 0, 0], [0, 0, 0])
    # n = L: two deletions; the freed tail is pad_id / 0 / 0, with a pad id that is not 0
    ids, mask, seg = _one([CLS, 5, 6, 7, 8, 9, 10, SEP], 8, [K, D, K, K, K, K, D, K], pad_id=1, seg=[1, 1, 1, 1, 2, 2, 2, 2])
    assert ids == [CLS, 6, 7, 8, 9, SEP, 1, 1] and mask == [1, 1, 1, 1, 1, 1, 0, 0] and seg == [1, 1, 1, 2, 2, 2, 0, 0]
    # source padding that is not pad_id is not carried over
    assert _one([CLS, 5, SEP, 17, 17], 3, [K] * 5, pad_id=1)[0] == [CLS, 5, SEP, 1, 1]


def test_reference_whole_words():
    # dog ##s ##s cat: the word deleted through its head; the pieces' own ops (keep, mask) do not count
    assert _one([CLS, 7, 16, 16, 6, SEP, 0, 0], 6, [K, D, K, M, K, K, K, K], CONT)[0] == [CLS, 6, SEP, 0, 0, 0, 0, 0]
    # without the table every position is its own word
    assert _one([CLS, 7, 16, 16, 6, SEP, 0, 0], 6, [K, D, K, M, K, K, K, K])[0] == [CLS, 16, MASK_ID, 6, SEP, 0, 0, 0]
    # a continuation piece at position 1 is its own head; the next piece follows it, the word after does not
    assert _one([CLS, 16, 16, 7, SEP, 0], 5, [K, M, K, K, K, K], CONT)[0] == [CLS, MASK_ID, MASK_ID, 7, SEP, 0]
    # an id outside [0, vocab) is a head: 25 is deleted and takes the piece after it along; -1 likewise starts a word of its own
    assert _one([CLS, 7, 25, 16, SEP, 0], 5, [K, K, D, K, K, K], CONT)[0] == [CLS, 7, SEP, 0, 0, 0]
    assert _one([CLS, 7, -1, SEP], 4, [K, D, K, K], CONT)[0] == [CLS, -1, SEP, 0]
    # a replaced word: every piece takes its OWN replacement id, even where its own op is not replace
    assert _one([CLS, 7, 16, SEP], 4, [K, rep(9), K | (11 << 2), K], CONT)[0] == [CLS, 9, 11, SEP]
    assert _one([CLS, 7, 16, SEP], 4, [K, rep(9), K, K], CONT)[0] == [CLS, 9, 0, SEP]
    # a head's decision ends at the next head
    assert _one([CLS, 7, 16, 6, 16, SEP], 6, [K, M, D, K, rep(5), K], CONT)[0] == [CLS, MASK_ID, MASK_ID, 6, 16, SEP]


def test_reference_keep_one_rule_with_and_without_the_table():
    # dog ##s: the head deleted, the piece "kept" - with the table the whole content is deleted, so none of it is
    assert _one([CLS, 7, 16, SEP, 0], 4, [K, D, K, K, K], CONT)[:2] == ([CLS, 7, 16, SEP, 0], [1, 1, 1, 1, 0])
    # without it the piece survives on its own, and the rule does not apply
    assert _one([CLS, 7, 16, SEP, 0], 4, [K, D, K, K, K])[:2] == ([CLS, 16, SEP, 0, 0], [1, 1, 1, 0, 0])
    assert _one([CLS, 7, 16, SEP, 0], 4, [K, D, D, K, K])[0] == [CLS, 7, 16, SEP, 0]
    # all but one deleted: the rule does not apply
    assert _one([CLS, 5, 6, 7, SEP], 5, [K, D, D, K, K])[0] == [CLS, 7, SEP, 0, 0]
    assert _one([CLS, 5, 6, 7, SEP], 5, [K, D, D, M, K])[0] == [CLS, MASK_ID, SEP, 0, 0]


def test_reference_rows_by_index_with_a_plan_per_output_sample():
    from d2r_amd.text_augment import token_augment_reference
    ids = np.array([[CLS, 5, 6, SEP], [CLS, 7, SEP, 0]])
    mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0]])
    seg = np.array([[0, 1, 2, 3], [4, 5, 6, 0]])
    plan = np.array([[K, M, K, K], [K, D, K, K], [K, K, K, K]], np.uint32)
    out = token_augment_reference(ids, mask, seg, [1, 0, 1], plan, None, V, MASK_ID, 0)
    assert out[0].tolist() == [[CLS, MASK_ID, SEP, 0], [CLS, 6, SEP, 0], [CLS, 7, SEP, 0]]
    assert out[1].tolist() == [[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]]
    assert out[2].tolist() == [[4, 5, 6, 0], [0, 2, 3, 0], [4, 5, 6, 0]]


def _aug(d=0.0, m=0.0, r=0.0, **kw):
    from d2r_amd.text_augment import TokenAugmenter
    kw.setdefault("replace_range", (1000, 30000))
    return TokenAugmenter(d, m, r, 103, 0, 30522, **kw)


def test_draw_is_a_pure_function_of_the_generator_state_and_of_nothing_else():
    torch.manual_seed(123)
    before = torch.get_rng_state()
    a, b = _aug(0.1, 0.2, 0.3, seed=7), _aug(0.1, 0.2, 0.3, seed=7)
    pa, pb = [a.draw(4, 16) for _ in range(3)], [b.draw(4, 16) for _ in range(3)]
    assert all(p.dtype == torch.uint32 and tuple(p.shape) == (4, 16) and p.is_contiguous() and not p.is_cuda for p in pa)
    assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(pa, pb))
    assert not np.array_equal(pa[0].numpy(), pa[1].numpy()), "successive batches get the same plan"
    state = a.generator.get_state()
    again = a.draw(4, 16)
    a.generator.set_state(state)
    assert np.array_equal(a.draw(4, 16).numpy(), again.numpy())
    assert not np.array_equal(pa[0].numpy(), _aug(0.1, 0.2, 0.3, seed=7, rank=1).draw(4, 16).numpy())
    assert not np.array_equal(pa[0].numpy(), _aug(0.1, 0.2, 0.3, seed=8).draw(4, 16).numpy())
    assert torch.equal(torch.get_rng_state(), before), "drawing moved torch's default generator"
    # the settings do not change how much of the stream a batch consumes
    off, on, whole = _aug(seed=7), _aug(0.3, 0.3, 0.4, seed=7), _aug(0.0, 0.0, 1.0, seed=7, cont=np.zeros(30522, np.uint8))
    for x in (off, on, whole):
        x.draw(5, 33)
    assert torch.equal(off.generator.get_state(), on.generator.get_state())
    assert torch.equal(off.generator.get_state(), whole.generator.get_state())
    # everything off: an all-zero plan, with and without a table
    assert not off.draw(7, 128).numpy().any()
    assert not (_aug(0.3, 0.3, 0.0, seed=1, cont=np.zeros(30522, np.uint8)).draw(7, 128).numpy() >> 2).any()


def test_draw_follows_the_stated_rule_on_the_same_uniforms():
    a = _aug(0.2, 0.3, 0.1, seed=3, replace_range=(10, 17))
    g = torch.Generator().manual_seed(a.generator.initial_seed())
    u = torch.rand(6, 50, 2, dtype=torch.float64, generator=g).numpy()
    plan = a.draw(6, 50).numpy()
    want = np.zeros((6, 50), np.uint32)
    for b in range(6):
        for l in range(50):
            u0, u1 = u[b, l]
            op = D if u0 < 0.2 else (M if u0 < 0.2 + 0.3 else (R if u0 < 0.2 + 0.3 + 0.1 else K))
            want[b, l] = op | ((10 + min(math.floor(u1 * 7), 6)) << 2 if op == R else 0)
    assert np.array_equal(plan, want)


def test_draw_replacement_ids_and_op_frequencies():
    lo, hi = 1000, 1007
    a = _aug(0.15, 0.1, 0.25, seed=11, replace_range=(lo, hi))
    plan = a.draw(200, 1000).numpy()
    n = plan.size
    assert n == 200_000
    op, rid = plan & 3, plan >> 2
    assert ((rid[op == R] >= lo) & (rid[op == R] < hi)).all() and not rid[op != R].any()
    assert set(np.unique(rid[op == R]).tolist()) == set(range(lo, hi))  # both ends of the range are drawn
    for code, p in ((D, 0.15), (M, 0.1), (R, 0.25), (K, 0.5)):
        count, sd = int((op == code).sum()), math.sqrt(n * p * (1 - p))
        assert abs(count - n * p) <= 4 * sd, (code, count, n * p, sd)
    # whole-word mode: every position carries an id of the range, whatever its own op (a piece replaced through its head needs one)
    whole = _aug(0.15, 0.1, 0.25, seed=11, replace_range=(lo, hi), cont=np.zeros(30522, np.uint8)).draw(200, 1000).numpy()
    assert np.array_equal(whole & 3, op) and ((whole >> 2 >= lo) & (whole >> 2 < hi)).all()
    assert np.array_equal((whole >> 2)[op == R], rid[op == R])
    # the whole vocabulary as the range, and the last id of it
    wide = _aug(0.0, 0.0, 1.0, seed=2, replace_range=(0, 30522)).draw(50, 1000).numpy()
    assert ((wide & 3) == R).all() and int((wide >> 2).max()) <= 30521 and int((wide >> 2).max()) > 30000


def test_augmenter_refuses_bad_settings():
    from d2r_amd.text_augment import TokenAugmenter
    for bad in ((-0.1, 0, 0), (0, 1.5, 0), (0, 0, float("nan")), (0.5, 0.4, 0.2)):
        with pytest.raises(ValueError):
            TokenAugmenter(*bad, 103, 0, 30522)
    TokenAugmenter(0.5, 0.25, 0.25, 103, 0, 30522)
    for kw in (dict(replace_range=(5, 5)), dict(replace_range=(-1, 5)), dict(replace_range=(0, 30523)), dict(cont=np.zeros(5, np.uint8)),
               dict(cont=np.zeros(30522, np.int64))):
        with pytest.raises(ValueError):
            TokenAugmenter(0.1, 0.1, 0.1, 103, 0, 30522, **kw)
    for mask_id, pad_id, vocab in ((30522, 0, 30522), (103, -1, 30522), (0, 0, 0)):
        with pytest.raises(ValueError):
            TokenAugmenter(0.1, 0.1, 0.1, mask_id, pad_id, vocab)
    text = TokenAugmenter(0.1, 0.2, 0.05, 103, 0, 30522, replace_range=(999, 30522)).describe()
    assert "0.1" in text and "0.2" in text and "0.05" in text and "[999, 30522)" in text and "\n" not in text


def test_text_stream_seed_is_a_stream_of_its_own():
    from d2r_amd.augment import photo_stream_seed, stream_seed
    from d2r_amd.functional import drop_path_stream_seed
    from d2r_amd.text_augment import TokenAugmenter, text_stream_seed
    for seed in (0, 1, 2023, 2 ** 32 - 1):
        for rank in (0, 1, 7, 2 ** 24 - 1):
            s = text_stream_seed(seed, rank)
            assert 0 <= s < 2 ** 64
            assert len({s, stream_seed(seed, rank), photo_stream_seed(seed, rank), drop_path_stream_seed(seed, rank), seed}) == 5
    seeds = {text_stream_seed(s, r) for s in (0, 1, 2023, 2 ** 32 - 1) for r in (0, 1, 7, 2 ** 24 - 1)}
    assert len(seeds) == 16
    assert text_stream_seed(2 ** 32 + 5, 3) == text_stream_seed(5, 3) and text_stream_seed(-1, 0) == text_stream_seed(2 ** 32 - 1, 0)
    with pytest.raises(ValueError):
        text_stream_seed(1, 2 ** 24)
    with pytest.raises(ValueError):
        text_stream_seed(1, -1)
    assert TokenAugmenter(0, 0, 0, 103, 0, 30522, seed=5, rank=2).generator.initial_seed() == text_stream_seed(5, 2)


def test_entry_point_is_declared_documented_exported_and_typed():
    from d2r_amd import _lib
    text = open(os.path.join(ROOT, "include", "d2r_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+d2r_token_augment\s*\(([^)]*)\)\s*;", hdr)
    assert m, "d2r_token_augment is not declared in include/d2r_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert "d2r_token_augment" in comments and "keep-one" in comments
    res, argtypes = _lib.SIGNATURES["d2r_token_augment"]
    assert res is _lib.i32 and len(argtypes) == len(args) == 18
    for a, t in zip(args, argtypes):
        if "*" in a:
            assert t is _lib.vp, (a, t)
        else:
            assert t is {"int": _lib.i32, "int64_t": _lib.i64}[a.split()[-2]], (a, t)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "d2r_token_augment")
    assert os.path.exists(os.path.join(ROOT, "d2r_amd", "csrc", "text.hip"))


FAKE = 1 << 24  # far apart fake device tensors: ids, mask, seg, idx, plan, cont, then the three outputs
P = {name: FAKE * (k + 1) for k, name in enumerate(("ids", "mask", "seg", "idx", "plan", "cont", "out_ids", "out_mask", "out_seg"))}


def _call(h_idx=(0, 1), h_plan=None, rows=5, L=8, B=None, vocab=V, mask_id=MASK_ID, pad_id=0, h_idx_ptr=True, h_plan_ptr=True, **ptr):
    """d2r_token_augment with fake device pointers -> (status, message).  Every such call must be refused before its launch."""
    from d2r_amd import _lib
    lib = _lib.load()
    h = np.asarray(h_idx, np.int64)
    B = len(h) if B is None else B
    hp = np.zeros((max(B, 1), max(L, 1)), np.uint32) if h_plan is None else np.ascontiguousarray(h_plan, dtype=np.uint32)
    p = dict(P, **ptr)
    rc = _lib._FN["d2r_token_augment"](p["ids"], p["mask"], p["seg"], rows, L, h.ctypes.data if h_idx_ptr else None, p["idx"],
                                       hp.ctypes.data if h_plan_ptr else None, p["plan"], B, p["cont"], vocab, mask_id, pad_id,
                                       p["out_ids"], p["out_mask"], p["out_seg"], None)
    return rc, lib.d2r_last_error().decode()


def _refused(what, **kw):
    rc, err = _call(**kw)
    assert rc < 0 and "d2r_token_augment" in err, (what, rc, err)
    return err


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every host refusal of d2r_token_augment: the checks run on the host copies, these calls never reach a launch (the device
    pointers are dummies; nothing is dereferenced)."""
    for name in ("ids", "mask", "seg", "idx", "plan", "out_ids", "out_mask", "out_seg"):
        assert "null" in _refused(f"null {name}", **{name: None})
    assert "null" in _refused("null h_idx", h_idx_ptr=False) and "null" in _refused("null h_plan", h_plan_ptr=False)
    for B in (0, -1, 65536):
        _refused(f"B = {B}", B=B)
    for L in (1, 0, -5, 1025):
        _refused(f"L = {L}", L=L)
    for rows in (0, -3):
        _refused(f"rows = {rows}", rows=rows)
    for h_idx in ([0, 5], [-1, 0], [2 ** 40, 0]):
        assert "outside the 5 rows" in _refused(f"h_idx = {h_idx}", h_idx=h_idx)
    for vocab in (0, -1):
        _refused(f"vocab = {vocab}", vocab=vocab, mask_id=0)
    for kw in (dict(mask_id=V), dict(mask_id=-1), dict(pad_id=V), dict(pad_id=-1)):
        assert "outside" in _refused(str(kw), **kw)
    plan = np.zeros((2, 8), np.uint32)
    plan[1, 3] = rep(V)
    assert "sample 1, position 3" in _refused("replacement id = vocab", h_plan=plan)
    plan[1, 3] = rep(2 ** 30 - 1)
    _refused("replacement id = 2^30 - 1", h_plan=plan)
    plan[1, 3] = K | (V << 2)  # a piece replaced through its head would take this id
    _refused("replacement id = vocab at an op that is not replace", h_plan=plan)
    for name in ("ids", "mask", "seg", "idx", "out_ids", "out_mask", "out_seg"):
        assert "aligned" in _refused(f"{name} + 4", **{name: P[name] + 4})
    assert "aligned" in _refused("plan + 2", plan=P["plan"] + 2)
    src, out = 5 * 8 * 8, 2 * 8 * 8  # bytes of a source tensor and of an output
    for o in ("out_ids", "out_mask", "out_seg"):
        for i, n in (("ids", src), ("mask", src), ("seg", src), ("idx", 2 * 8), ("plan", 2 * 8 * 4), ("cont", V)):
            assert "overlap" in _refused(f"{o} = {i}", **{o: P[i]})
            assert "overlap" in _refused(f"{o} ends inside {i}", **{o: P[i] - out + 8})
            assert "overlap" in _refused(f"{o} begins inside {i}", **{o: P[i] + (n - 1) // 8 * 8})
    assert "overlap" in _refused("out_mask = out_ids", out_mask=P["out_ids"])
    assert "overlap" in _refused("out_seg inside out_mask", out_seg=P["out_mask"] + out - 8)


def test_flag_ranges_sum_and_refusals():
    from d2r_amd.run import build_parser, main
    p = build_parser()
    d = p.parse_args([])
    assert d.aug_token_delete == d.aug_token_mask == d.aug_token_replace == 0.0 and d.aug_whole_word is False
    a = p.parse_args(["--aug_token_delete", "0.1", "--aug_token_mask", "1", "--aug_token_replace", "0.05", "--aug_whole_word"])
    assert (a.aug_token_delete, a.aug_token_mask, a.aug_token_replace, a.aug_whole_word) == (0.1, 1.0, 0.05, True)
    for flag in ("--aug_token_delete", "--aug_token_mask", "--aug_token_replace"):
        for bad in ("-0.01", "1.5", "nan", "half"):
            with pytest.raises(SystemExit):
                p.parse_args([flag, bad])
    with pytest.raises(SystemExit, match=r"--aug_token_delete / --aug_token_mask / --aug_token_replace"):
        main(["--aug_token_delete", "0.5", "--aug_token_mask", "0.4", "--aug_token_replace", "0.2"])
    with pytest.raises(SystemExit, match="synthetic"):
        main(["--aug_whole_word", "--aug_token_delete", "0.1"])
    with pytest.raises(SystemExit, match="synthetic"):
        main(["--aug_whole_word"])


def _tiny_tokenizer(tmp_path):
    transformers = pytest.importorskip("transformers")
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    return transformers.BertTokenizer.from_pretrained(str(tmp_path), do_lower_case=True)


def test_continuation_table_and_token_settings_of_the_tiny_vocabulary(tmp_path):
    from d2r_amd.run import token_settings
    from d2r_amd.text_augment import TokenAugmenter, continuation_table
    tok = _tiny_tokenizer(tmp_path)
    table = continuation_table(tok)
    assert table.dtype == np.uint8 and table.shape == (len(VOCAB),)
    assert np.flatnonzero(table).tolist() == [VOCAB.index("##s")] == [16]
    s = token_settings(tok, whole_word=True, need_mask=True)
    assert (s["mask_id"], s["pad_id"], s["vocab"], s["replace_range"]) == (MASK_ID, 0, 20, (5, 20)) and np.array_equal(s["cont"], table)
    assert token_settings(tok, whole_word=False, need_mask=True)["cont"] is None
    TokenAugmenter(0.1, 0.1, 0.1, **s)
    # [unusedN] tokens count as reserved; a tokenizer without a mask token is refused only when masking is asked for
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB[:4] + ["[unused0]", "the", "[unused7]", "cat", "##s"]) + "\n")
    import transformers
    bare = transformers.BertTokenizer.from_pretrained(str(tmp_path), do_lower_case=True, mask_token=None)
    assert bare.mask_token_id is None
    with pytest.raises(SystemExit, match="mask token"):
        token_settings(bare, whole_word=False, need_mask=True)
    s = token_settings(bare, whole_word=True, need_mask=False)
    assert s["replace_range"] == (7, 9) and np.flatnonzero(s["cont"]).tolist() == [8]


class _StubCache:
    device = torch.device("cpu")

    def gather(self, h_idx, idx, augmenter=None, text_augmenter=None):
        return h_idx, augmenter, text_augmenter


def test_cached_loader_passes_its_text_augmenter_to_every_gather():
    from d2r_amd.cache import CachedLoader
    from d2r_amd.data import make_loader
    text = _aug(0.1, 0.1, 0.1)
    dl = make_loader(list(range(10)), 5, False, 0)
    both, only_text, without = (CachedLoader(dl, _StubCache(), "image", text_augmenter=text), CachedLoader(dl, _StubCache(), text_augmenter=text),
                                CachedLoader(dl, _StubCache()))
    assert only_text.text_augmenter is text and only_text.augmenter is None and without.text_augmenter is None
    assert [(a, t) for _, a, t in both] == [("image", text)] * 2
    assert [(a, t) for _, a, t in only_text] == [(None, text)] * 2
    assert [(a, t) for _, a, t in without] == [(None, None)] * 2


class _StubTrainer:
    made = []

    def __init__(self, **kwargs):
        self.kwargs, self.samples_per_sec = kwargs, None
        _StubTrainer.made.append(self)

    def train(self, clip_sd, bert_sd):
        pass

    def _load_checkpoint(self, path):
        pass

    def predict(self, loader, path):
        pass


def test_run_gives_the_text_augmenter_to_the_cached_training_loader_or_to_the_trainer(monkeypatch, tmp_path, caplog):
    """run.main's wiring with the dataset, the model, the trainer and cache_loaders stubbed.  With the cache: text_augmenters is
    {"train": augmenter} and the trainer gets none.  Without it: the trainer gets the augmenter.  Flags at their defaults: neither
    keyword is passed at all.  --only_test: none is built, and a line says the flags are ignored."""
    import logging
    from d2r_amd import cache as C, data as D, modules as M, run, train as T
    from d2r_amd.text_augment import TokenAugmenter, text_stream_seed
    tok = _tiny_tokenizer(tmp_path)
    for name in ("train.json", "dev.json", "test.json"):
        (tmp_path / name).write_text("[]")

    class Split(torch.utils.data.Dataset):
        max_seq, tokenizer = 16, tok

        def __init__(self, *args, **kwargs):
            pass

        def __len__(self):
            return 10

        def __getitem__(self, i):
            return i

    calls = []

    def cache_loaders(loaders, device, logger=None, augmenters=None, **more):
        calls.append((augmenters, more))
        return loaders

    monkeypatch.setattr(C, "cache_loaders", cache_loaders)
    monkeypatch.setattr(D, "MSDDataset", Split)
    monkeypatch.setattr(M, "UnimoModelF", lambda **kwargs: object())
    monkeypatch.setattr(T, "MSDTrainer", _StubTrainer)
    monkeypatch.setattr(run, "set_seed", lambda seed: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--data_path", str(tmp_path), "--img_path", str(tmp_path), "--bert_name", str(tmp_path), "--device", "cpu", "--seed", "5",
            "--num_workers", "0"]
    on = ["--aug_token_delete", "0.25", "--aug_token_replace", "0.5", "--aug_whole_word"]

    def main(extra):
        del calls[:], _StubTrainer.made[:]
        run.main(base + extra)
        assert len(_StubTrainer.made) == 1
        return _StubTrainer.made[0].kwargs

    def check(aug):
        assert isinstance(aug, TokenAugmenter) and (aug.delete_p, aug.mask_p, aug.replace_p) == (0.25, 0.0, 0.5)
        assert (aug.mask_id, aug.pad_id, aug.vocab, aug.replace_range) == (MASK_ID, 0, 20, (5, 20))
        assert aug.cont is not None and aug.cont.nonzero().flatten().tolist() == [16]
        assert aug.generator.initial_seed() == text_stream_seed(5, 0)

    kwargs = main(on + ["--cache_dataset", "device"])
    assert len(calls) == 1 and calls[0][0] is None and list(calls[0][1]) == ["text_augmenters"] and list(calls[0][1]["text_augmenters"]) == ["train"]
    check(calls[0][1]["text_augmenters"]["train"])
    assert "text_augmenter" not in kwargs

    kwargs = main(on)
    assert calls == []
    check(kwargs["text_augmenter"])
    assert main(on[:-1])["text_augmenter"].cont is None

    kwargs = main(["--cache_dataset", "device"])
    assert calls == [(None, {})] and "text_augmenter" not in kwargs
    assert "text_augmenter" not in main([])

    with caplog.at_level(logging.INFO, logger="d2r_amd.run"):
        kwargs = main(on + ["--only_test", "--load_path", str(tmp_path / "model.pth")])
    assert calls == [] and "text_augmenter" not in kwargs
    assert sum("--aug_whole_word are ignored with --only_test" in r.getMessage() for r in caplog.records) == 1
