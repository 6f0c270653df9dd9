"""--aug_token_delete / --aug_token_mask / --aug_token_replace / --aug_whole_word: token-level augmentation of the training texts,
on the device.

Every training batch's input_ids, input_mask and segment_ids are built on the device anyway: by three d2r_gather_rows launches from
the device cache (d2r_amd.cache), or by the batch's own copy without it.  One kernel (d2r_token_augment, csrc/text.hip) takes the
place of the three gathers and deletes, masks ([MASK]) or replaces (a random id) tokens per sample on the way; [CLS] and [SEP] are
never touched, the survivors are packed to the front, and a post whose every content token would be deleted keeps them all.  What
happens to which position is drawn on the host, one vectorised draw per batch, from a generator of the augmenter's own: torch's
default generator (the samplers, the dropout seeds) and the image augmentation's streams are never touched.  With a continuation
table (--aug_whole_word) the pieces of a word share the decision drawn at its first piece.  The reference has no augmentation; this
is an extension, off by default, and only the training split is ever augmented.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

_TAG = 0x74657874617567  # "textaug": apart from the crop ("augment"), photometric and DropPath streams and a default generator's
KEEP, DELETE, MASK, REPLACE = 0, 1, 2, 3  # bits 0-1 of a plan word; bits 2-31 hold the replacement id
MAX_VOCAB = 1 << 30        # a replacement id has 30 bits
MAX_L, MAX_B = 1024, 65535  # d2r_token_augment's limits


def text_stream_seed(seed: int, rank: int = 0) -> int:
    """The seed of rank `rank`'s text-augmentation generator: augment.stream_seed's construction with a tag of its own,
    ``(((seed mod 2^32) << 24) | rank) ^ 0x74657874617567`` with 0 <= rank < 2^24."""
    if not 0 <= int(rank) < (1 << 24):
        raise ValueError(f"rank must be in [0, 2^24), got {rank}")
    return (((int(seed) & 0xFFFFFFFF) << 24) | int(rank)) ^ _TAG


def continuation_table(tokenizer) -> np.ndarray:
    """uint8 [len(tokenizer)]: 1 where the token's text starts with "##" (a WordPiece continuation), 0 elsewhere."""
    table = np.zeros(len(tokenizer), dtype=np.uint8)
    for token, i in tokenizer.get_vocab().items():
        if token.startswith("##"):
            table[i] = 1
    return table


def token_augment_reference(ids, mask, seg, idx, plan, cont, vocab, mask_id, pad_id):
    """d2r_token_augment in plain numpy, position by position (the function is stated at the declaration in include/d2r_hip.h):
    ids, mask, seg int64 [rows, L]; idx [B]; plan uint32 [B, L]; cont uint8 [vocab] or None -> (out_ids, out_mask, out_seg), int64
    [B, L]."""
    ids, mask, seg = (np.asarray(t, dtype=np.int64) for t in (ids, mask, seg))
    idx, plan = np.asarray(idx, dtype=np.int64), np.asarray(plan).astype(np.int64)
    B, L = len(idx), ids.shape[1]
    out_ids = np.full((B, L), pad_id, dtype=np.int64)
    out_mask, out_seg = np.zeros((B, L), dtype=np.int64), np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        r = int(idx[b])
        n = int(np.count_nonzero(mask[r]))
        content = list(range(1, n - 1))
        op, head_op = {}, KEEP
        for l in content:
            t = int(ids[r, l])
            if l == 1 or cont is None or not 0 <= t < vocab or cont[t] == 0:
                head_op = int(plan[b, l]) & 3
            op[l] = head_op
        if content and all(op[l] == DELETE for l in content):  # the keep-one rule
            op = {l: KEEP for l in content}
        j = 0
        for l in range(n):
            o = op.get(l, KEEP)  # [CLS] and [SEP] are kept
            if o == DELETE:
                continue
            out_ids[b, j] = mask_id if o == MASK else (int(plan[b, l]) >> 2 if o == REPLACE else ids[r, l])
            out_mask[b, j], out_seg[b, j] = 1, seg[r, l]
            j += 1
    return out_ids, out_mask, out_seg


def token_augment(ids, mask, seg, h_idx, idx, h_plan, plan, cont, vocab, mask_id, pad_id, out=None):
    """d2r_token_augment on the current stream: ids / mask / seg contiguous int64 [rows, L] on the device, idx int64 [B] there and
    h_idx its host copy, plan uint32 [B, L] there and h_plan its host copy, cont uint8 [vocab] on the device or None.
    -> (out_ids, out_mask, out_seg), the three [B, L] slices of `out` (int64 [3, B, L], allocated when None)."""
    from .functional import _stream
    B, L = int(h_idx.numel()), int(ids.shape[1])
    for name, t in (("ids", ids), ("mask", mask), ("seg", seg)):
        if t.dtype != torch.int64 or t.dim() != 2 or not t.is_contiguous() or t.shape != ids.shape or t.device != ids.device:
            raise ValueError(f"{name} must be a contiguous int64 [rows, L] tensor on the device of ids, got {t.dtype} {tuple(t.shape)}")
    if h_idx.dtype != torch.int64 or h_idx.is_cuda or not h_idx.is_contiguous() or idx.dtype != torch.int64 or idx.shape != h_idx.shape:
        raise ValueError("h_idx must be a contiguous host int64 [B] tensor and idx its device copy")
    for name, t in (("h_plan", h_plan), ("plan", plan)):
        if t.dtype not in (torch.uint32, torch.int32) or tuple(t.shape) != (B, L) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint32 (or int32: the same bits) [{B}, {L}] tensor, got {t.dtype} {tuple(t.shape)}")
    if h_plan.is_cuda or plan.device != ids.device or idx.device != ids.device:
        raise ValueError("h_plan must be on the host, plan and idx on the device of ids")
    if cont is not None and (cont.dtype != torch.uint8 or cont.numel() != vocab or cont.device != ids.device or not cont.is_contiguous()):
        raise ValueError(f"cont must be a contiguous uint8 [{vocab}] tensor on the device of ids")
    if out is None:
        out = torch.empty(3, B, L, dtype=torch.int64, device=ids.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (3, B, L) or not out.is_contiguous() or out.device != ids.device:
        raise ValueError(f"out must be a contiguous int64 [3, {B}, {L}] tensor on the device of ids")
    _lib.call("d2r_token_augment", ids.data_ptr(), mask.data_ptr(), seg.data_ptr(), ids.shape[0], L, h_idx.data_ptr(), idx.data_ptr(),
              h_plan.data_ptr(), plan.data_ptr(), B, None if cont is None else cont.data_ptr(), vocab, mask_id, pad_id,
              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream())
    return out[0], out[1], out[2]


class TokenAugmenter:
    """Per content token of a training text: delete it with probability delete_p, else put mask_id in its place with probability
    mask_p, else an id drawn uniformly from replace_range = [lo, hi) with probability replace_p, else keep it.  With `cont` (uint8
    [vocab], continuation_table) a word's pieces share what was drawn at its first piece; a replaced piece still gets an id of its
    own.  Everything at 0 is "off": ``apply`` is then bit for bit the plain gather.  The draws happen all the same, so the stream does
    not depend on the settings."""

    def __init__(self, delete_p: float, mask_p: float, replace_p: float, mask_id: int, pad_id: int, vocab: int, replace_range=None,
                 cont=None, seed: int = 0, rank: int = 0):
        for name, p in (("delete_p", delete_p), ("mask_p", mask_p), ("replace_p", replace_p)):
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"{name} must be in [0, 1], got {p}")
        if not delete_p + mask_p + replace_p <= 1.0:
            raise ValueError(f"delete_p + mask_p + replace_p must be <= 1, got {delete_p} + {mask_p} + {replace_p}")
        if not 1 <= int(vocab) <= MAX_VOCAB:
            raise ValueError(f"vocab must be in [1, 2^30], got {vocab}")
        for name, t in (("mask_id", mask_id), ("pad_id", pad_id)):
            if not 0 <= int(t) < int(vocab):
                raise ValueError(f"{name} must be in [0, {vocab}), got {t}")
        lo, hi = (0, int(vocab)) if replace_range is None else (int(replace_range[0]), int(replace_range[1]))
        if not 0 <= lo < hi <= int(vocab):
            raise ValueError(f"replace_range must satisfy 0 <= lo < hi <= vocab = {vocab}, got ({lo}, {hi})")
        self.delete_p, self.mask_p, self.replace_p = float(delete_p), float(mask_p), float(replace_p)
        self.mask_id, self.pad_id, self.vocab, self.replace_range = int(mask_id), int(pad_id), int(vocab), (lo, hi)
        self.cont = None
        if cont is not None:
            cont = np.ascontiguousarray(cont)
            if cont.dtype != np.uint8 or cont.shape != (self.vocab,):
                raise ValueError(f"cont must be a uint8 [{self.vocab}] array, got {cont.dtype} {cont.shape}")
            self.cont = torch.from_numpy(cont.copy())
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(text_stream_seed(seed, rank))
        self._slots = {}     # B -> (host arange, device arange) of the uncached path
        self._cont_dev = {}  # device -> cont there

    def describe(self) -> str:
        lo, hi = self.replace_range
        return (f"per token: delete with probability {self.delete_p:g}, [MASK] (id {self.mask_id}) with probability {self.mask_p:g}, "
                f"a random id in [{lo}, {hi}) with probability {self.replace_p:g}; "
                f"{'whole words (a word and its ## pieces share one decision)' if self.cont is not None else 'every piece on its own'}; "
                "[CLS] and [SEP] are kept, and so is a text whose every token would be deleted")

    def draw(self, B: int, L: int) -> torch.Tensor:
        """The plan of one batch, host uint32 [B, L] (bits 0-1: 0 keep, 1 delete, 2 mask, 3 replace; bits 2-31: the replacement
        id), from ONE torch.rand(B, L, 2, float64) of the augmenter's generator, whatever the settings.  Per position, with u0, u1
        its pair: delete if u0 < delete_p, else mask if u0 < delete_p + mask_p, else replace if u0 < delete_p + mask_p + replace_p,
        else keep; the replacement id is lo + min(floor(u1 * (hi - lo)), hi - lo - 1).  The id is stored where the op is replace - and,
        with a continuation table and replace_p > 0, at every position: a piece that is replaced through its word's first piece
        takes its OWN id, which must then be one of [lo, hi) and not 0.  Everything off draws an all-zero plan."""
        u = torch.rand(B, L, 2, dtype=torch.float64, generator=self.generator)
        d, m = self.delete_p, self.delete_p + self.mask_p
        r = m + self.replace_p
        u0 = u[..., 0]
        op = torch.where(u0 < d, DELETE, torch.where(u0 < m, MASK, torch.where(u0 < r, REPLACE, KEEP)))
        lo, hi = self.replace_range
        rid = lo + torch.floor(u[..., 1] * float(hi - lo)).to(torch.int64).clamp_(max=hi - lo - 1)
        stored = op == REPLACE
        if self.cont is not None and self.replace_p > 0.0:
            stored = torch.ones_like(stored)
        word = op + torch.where(stored, rid << 2, torch.zeros_like(rid))
        return torch.from_numpy(word.numpy().astype(np.uint32))

    def apply(self, ids: torch.Tensor, mask: torch.Tensor, seg: torch.Tensor, h_idx: torch.Tensor, idx: torch.Tensor):
        """Draws one batch's plan, uploads it (one non-blocking copy from pinned memory) and launches d2r_token_augment on the
        current stream: the augmented (input_ids, input_mask, segment_ids), int64 [B, L], of the rows idx of ids / mask / seg
        (int64 [rows, L] on the device; h_idx is the host copy of idx)."""
        h_plan = self.draw(int(h_idx.numel()), int(ids.shape[1])).view(torch.int32)  # the same bits, a dtype every copy path takes
        if ids.is_cuda:
            h_plan = h_plan.pin_memory()
        cont = None
        if self.cont is not None:
            cont = self._cont_dev.get(ids.device)
            if cont is None:
                cont = self._cont_dev[ids.device] = self.cont.to(ids.device)
        return token_augment(ids, mask, seg, h_idx, idx, h_plan, h_plan.to(ids.device, non_blocking=True), cont, self.vocab,
                             self.mask_id, self.pad_id)

    def apply_batch(self, ids: torch.Tensor, mask: torch.Tensor, seg: torch.Tensor):
        """The uncached path: the batch's own token tensors, already on the device, are the source rows 0..B-1."""
        B = int(ids.shape[0])
        key = (B, ids.device)
        if key not in self._slots:
            h = torch.arange(B, dtype=torch.int64)
            h = h.pin_memory() if ids.is_cuda else h
            self._slots[key] = (h, h.to(ids.device))
        h_slots, slots = self._slots[key]
        return self.apply(ids.contiguous(), mask.contiguous(), seg.contiguous(), h_slots, slots)
