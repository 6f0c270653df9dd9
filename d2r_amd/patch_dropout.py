"""--patch_dropout: PatchDropout of the vision tower (Liu et al. 2022, "PatchDropout: Economizing Vision Transformers Using Patch
Dropout"; open_clip's --force-patch-dropout), DESIGN.md K25.

In a training forward every image keeps its class token and K of its np patch tokens, drawn without replacement and independently per
sample; the rest never enter the tower.  The kept patches carry the position embedding of their original position, so the result is
what open_clip computes by dropping after the position embedding is added.  Everything behind the embedding - the CLIP layers, the
vision self layer and both routing modules - then runs on [B, 1 + K, 768], which is the point: it regularises AND removes work.  The
embedding itself only unfolds, multiplies and finishes the kept patches (d2r_patchify_keep, d2r_clip_embed_finish_keep,
d2r_clip_embed_bwd_keep, csrc/misc.hip).

Which patches stay is drawn on the host, one torch.rand per training forward, from a generator of the sampler's own: torch's default
generator (the samplers, the dropout seeds) and every other stream of a run (augmenters, mixer, DropPath) are never touched.  The
reference has no PatchDropout; this is an extension, off by default, and dev / test / prediction passes always see all patches.
"""
from __future__ import annotations

import math

import torch

_PATCH_DROPOUT_TAG = 0x7061746368647270  # "patchdrp": apart from the augmenters', the mixer's, DropPath's streams and a default generator's


def check_rate(p) -> float:
    """P as a float in [0, 1), or ValueError (non-finite values included)."""
    p = float(p)
    if not (math.isfinite(p) and 0.0 <= p < 1.0):
        raise ValueError(f"patch_dropout must be in [0, 1) (0 = off), got {p}")
    return p


def kept_patches(num_patches: int, p: float) -> int:
    """K = max(1, int(np * (1.0 - P))) in Python floats: open_clip's PatchDropout rule.  The same on every rank."""
    if int(num_patches) < 1:
        raise ValueError(f"an image has at least one patch, got {num_patches}")
    return max(1, int(int(num_patches) * (1.0 - check_rate(p))))


def patch_dropout_stream_seed(seed: int, rank: int = 0) -> int:
    """The seed of rank `rank`'s PatchDropout generator in a run seeded `seed`: augment.stream_seed's construction with a tag of its
    own, ``((((seed mod 2^32) << 24) | rank) ^ 0x7061746368647270) mod 2^64``: distinct (seed mod 2^32, rank) pairs give distinct seeds."""
    if not 0 <= int(rank) < (1 << 24):
        raise ValueError(f"rank must be in [0, 2^24), got {rank}")
    return ((((int(seed) & 0xFFFFFFFF) << 24) | int(rank)) ^ _PATCH_DROPOUT_TAG) & 0xFFFFFFFFFFFFFFFF


class PatchDropout:
    """The sampler of one vision tower: `num_patches` patches per image, K = kept_patches(num_patches, p) of them kept per sample."""

    def __init__(self, p: float, num_patches: int, seed: int = 0, rank: int = 0):
        self.p = check_rate(p)
        if self.p == 0.0:
            raise ValueError("patch_dropout 0 is off: no sampler is built (UnimoModel.set_patch_dropout clears it)")
        self.num_patches = int(num_patches)
        self.K = kept_patches(self.num_patches, self.p)
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(patch_dropout_stream_seed(seed, rank))

    def describe(self) -> str:
        return (f"P = {self.p:g}: K = {self.K} of np = {self.num_patches} patches kept per training image, drawn per sample without "
                f"replacement; {1 + self.K} image tokens (class token + K) instead of {1 + self.num_patches} in the vision tower, the "
                "vision self layer and both routing modules; dev, test and prediction passes use all patches")

    def draw(self, B: int) -> torch.Tensor:
        """The kept positions of one batch, host int32 [B, K], every row strictly increasing: ONE u = torch.rand(B, np) from the
        sampler's generator; sample b keeps the K positions with the smallest u[b] - torch.argsort(u[b], stable=True)[:K], sorted
        ascending.  (A stable sort: equal values, should they occur, go to the lower position on every platform.)"""
        u = torch.rand(B, self.num_patches, generator=self.generator)
        keep = torch.argsort(u, dim=1, stable=True)[:, :self.K].sort(dim=1).values
        return keep.to(torch.int32).contiguous()

    def sample(self, B: int, device):
        """(h_keep, keep): the draw of one batch on the host - in pinned memory when `device` is a GPU, so that the copy does not
        block - and its device copy, enqueued on the current stream."""
        h_keep = self.draw(B)
        device = torch.device(device)
        if device.type != "cuda":
            return h_keep, h_keep
        h_keep = h_keep.pin_memory()
        return h_keep, h_keep.to(device, non_blocking=True)
