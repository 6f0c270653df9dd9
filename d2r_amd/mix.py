"""--aug_mixup / --aug_cutmix / --aug_mix_prob: MixUp and CutMix of the training images, on the device, with a mixed-label loss.

Every sample of a training batch is paired with another sample of the same batch.  MixUp blends the two images, a * own + (1 - a) *
partner; CutMix pastes a box of the partner's image over the sample's own.  The label follows the image's share: the cross entropy
of sample b is taken against lam_b onehot(y_b) + (1 - lam_b) onehot(y_partner) (d2r_ce_mix_fwd / d2r_ce_mix_bwd, or the one-call head
with its two extra fields).  ONLY THE IMAGE IS MIXED: the text of sample b stays its own - the usual convention when one modality is
mixed.  lam is drawn per sample (timm's mode="elem"), not per batch.

One kernel (d2r_image_mix, csrc/image.hip, K24) runs on the finished fp32 pixel batch, after every path that builds one (plain gather,
crop / flip, photometric augmentation, the uncached preprocessing, synthetic tensors), so cached and uncached loaders mix alike and
no other kernel changes.  The descriptors are drawn on the host from a generator of the mixer's own: torch's default generator (the
samplers, the dropout seeds) and the augmenters' generators are never touched.  The reference has no augmentation; this is an
extension, off by default, and only the training split is ever mixed.
"""
from __future__ import annotations

import math

import torch

from . import functional as F

MIX_FIELDS = 8             # int32 words per descriptor: partner, fp32 bits of a, x0, y0, w, h, 0, 0
SWITCH_PROB = 0.5          # with both on: CutMix with this probability, MixUp otherwise (timm's switch_prob)
_MIX_TAG = 0x6D697875706D6978  # "mixupmix": the mixer's stream, apart from the augmenters', DropPath's and a default generator's


def mix_stream_seed(seed: int, rank: int = 0) -> int:
    """The seed of rank `rank`'s mixing generator: augment.stream_seed's construction with a tag of its own,
    ``((((seed mod 2^32) << 24) | rank) ^ 0x6D697875706D6978) mod 2^64`` (as augment.photo_stream_seed)."""
    if not 0 <= int(rank) < (1 << 24):
        raise ValueError(f"rank must be in [0, 2^24), got {rank}")
    return ((((int(seed) & 0xFFFFFFFF) << 24) | int(rank)) ^ _MIX_TAG) & 0xFFFFFFFFFFFFFFFF


def _gamma_seed(base: int, batch: int) -> int:
    """The seed of the gamma draw of batch number `batch` (0, 1, ...) of the mixer seeded `base`: splitmix64 of base + batch + 1
    (the CPU generator keeps the low 32 bits of a seed; the finaliser spreads every input bit over them)."""
    z = (base + 0x9E3779B97F4A7C15 * (batch + 1)) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


class Mixer:
    """MixUp (mixup_alpha > 0) and / or CutMix (cutmix_alpha > 0) of [B, 3, S, S] pixel batches: each sample is mixed with probability
    `prob`, its lam ~ Beta(alpha, alpha) drawn per sample.  With both alphas 0, or prob = 0, every descriptor is the identity (the
    draws happen all the same, so the stream does not depend on the settings)."""

    def __init__(self, S: int, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0, seed: int = 0, rank: int = 0):
        if not (isinstance(S, int) and 1 <= S <= 4096):
            raise ValueError(f"S must be an integer in [1, 4096], got {S}")
        for name, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"prob must be in [0, 1], got {prob}")
        self.S, self.mixup_alpha, self.cutmix_alpha, self.prob = S, float(mixup_alpha), float(cutmix_alpha), float(prob)
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(mix_stream_seed(seed, rank))
        # torch's gamma sampler rejects: how much of a stream it consumes depends on the shape parameters.  It therefore draws from a
        # second generator that is seeded anew for every batch from (seed, rank, batch number), so that neither generator's position
        # at the start of a batch depends on the settings.
        self.gamma_generator = torch.Generator(device="cpu")
        self.batches = 0
        am, ac = self.mixup_alpha or 1.0, self.cutmix_alpha or 1.0
        self._shape = torch.tensor([am, am, ac, ac], dtype=torch.float64)
        self.last_lam0 = None  # float64 [B, 2]: the Beta values of the last draw (MixUp's, CutMix's), for inspection

    def describe(self) -> str:
        parts = []
        if self.mixup_alpha > 0.0:
            parts.append(f"MixUp with lam ~ Beta({self.mixup_alpha:g}, {self.mixup_alpha:g})")
        if self.cutmix_alpha > 0.0:
            parts.append(f"CutMix with lam ~ Beta({self.cutmix_alpha:g}, {self.cutmix_alpha:g}), the label share corrected to the clipped box")
        if len(parts) == 2:
            parts.append(f"CutMix chosen with probability {SWITCH_PROB:g} per sample")
        if not parts:
            parts.append("off")
        return ("; ".join(parts) + f"; applied to a sample with probability {self.prob:g}; partner: a random permutation of the batch; "
                "only the image is mixed (the text stays the sample's own), the label by the image's share")

    def draw(self, B: int):
        """(descriptors, lam) of one batch: host int32 [B, 8] ({partner, fp32 bits of a, x0, y0, w, h, 0, 0}: d2r_image_mix) and host
        fp32 [B] (the share of the sample's own label), from ONE torch.rand(B, 6, float64) and ONE torch._standard_gamma(float64
        [B, 4]) with shape parameters (am, am, ac, ac) - mixup_alpha, cutmix_alpha, 1.0 in place of a 0 - whatever the settings.  The
        uniforms come from the mixer's generator; the gammas from its second one, seeded for this batch (see __init__), because the
        gamma sampler's consumption depends on its shape parameters.  Per sample b, with u0..u5 and g0..g3 its rows:
            partner = argsort(u0)[b]  (a permutation of the batch; fixed points are allowed),
            apply   = u1 < prob and some alpha > 0;  otherwise the identity: partner = b, a = 1, empty box, lam = 1,
            CutMix  if only cutmix_alpha > 0, or both are and u2 < 0.5;  MixUp otherwise,
            lam0    = g0 / (g0 + g1) for MixUp, g2 / (g2 + g3) for CutMix: Beta(alpha, alpha)  (0.5 should both gammas underflow to 0),
            MixUp:  a = lam = fp32(lam0), empty box,
            CutMix: r = sqrt(1 - lam0),  cut = int(S * r),  cx = floor(u3 * S),  cy = floor(u4 * S),
                    x0 = clamp(cx - cut // 2, 0, S),  x1 = clamp(cx + cut // 2, 0, S),  y0, y1 likewise from cy,
                    a = 1,  box (x0, y0, x1 - x0, y1 - y0),  lam = fp32(1 - (x1 - x0) (y1 - y0) / S^2);  u5 is spare.
        This is timm's Mixup(mode="elem", switch_prob=0.5, correct_lam=True) - rand_bbox with the share corrected to the clipped
        box - with a permutation as the pairing where timm flips the batch."""
        S = self.S
        u = torch.rand(B, 6, dtype=torch.float64, generator=self.generator)
        self.gamma_generator.manual_seed(_gamma_seed(self.generator.initial_seed(), self.batches))
        self.batches += 1
        g = torch._standard_gamma(self._shape.expand(B, 4).contiguous(), generator=self.gamma_generator)
        den = torch.stack((g[:, 0] + g[:, 1], g[:, 2] + g[:, 3]), 1)
        lam0 = torch.where(den > 0, torch.stack((g[:, 0], g[:, 2]), 1) / den.clamp_min(torch.finfo(torch.float64).tiny), torch.full_like(den, 0.5))
        self.last_lam0 = lam0
        own = torch.arange(B, dtype=torch.int64)
        partner = torch.argsort(u[:, 0])
        on = (u[:, 1] < self.prob) if (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0) else torch.zeros(B, dtype=torch.bool)
        if self.cutmix_alpha > 0.0 and self.mixup_alpha > 0.0:
            cut_on = on & (u[:, 2] < SWITCH_PROB)
        else:
            cut_on = on & (self.cutmix_alpha > 0.0)
        mix_on = on & ~cut_on
        # CutMix boxes (for every sample; kept where cut_on)
        cut = (S * torch.sqrt(1.0 - lam0[:, 1])).to(torch.int64)
        cx, cy = torch.floor(u[:, 3] * S).to(torch.int64), torch.floor(u[:, 4] * S).to(torch.int64)
        x0, x1 = (cx - cut // 2).clamp(0, S), (cx + cut // 2).clamp(0, S)
        y0, y1 = (cy - cut // 2).clamp(0, S), (cy + cut // 2).clamp(0, S)
        lam_cut = 1.0 - ((x1 - x0) * (y1 - y0)).to(torch.float64) / float(S * S)
        one = torch.ones(B, dtype=torch.float64)
        lam = torch.where(mix_on, lam0[:, 0], torch.where(cut_on, lam_cut, one)).to(torch.float32)
        a = torch.where(mix_on, lam0[:, 0], one).to(torch.float32)
        zero = torch.zeros(B, dtype=torch.int64)
        out = torch.zeros(B, MIX_FIELDS, dtype=torch.int32)
        out[:, 0] = torch.where(on, partner, own)
        out[:, 1] = a.view(torch.int32)
        out[:, 2], out[:, 3] = torch.where(cut_on, x0, zero), torch.where(cut_on, y0, zero)
        out[:, 4], out[:, 5] = torch.where(cut_on, x1 - x0, zero), torch.where(cut_on, y1 - y0, zero)
        return out, lam

    def apply(self, pixels: torch.Tensor, labels: torch.Tensor):
        """Draws one batch, uploads descriptors and shares together (one non-blocking copy from pinned memory), launches
        d2r_image_mix on the current stream and picks the partners' labels on the device (one index_select):
        -> (mixed pixels, labels, labels[partner], lam fp32 [B] on the device)."""
        B = pixels.shape[0]
        if pixels.shape[-1] != self.S:
            raise ValueError(f"the batch holds {pixels.shape[-1]} x {pixels.shape[-1]} images, the mixer was built for {self.S}")
        h_desc, h_lam = self.draw(B)
        n = B * MIX_FIELDS
        host = torch.empty(n + 2 * B, dtype=torch.int32)  # [descriptors | fp32 bits of lam | partners]: one upload, three views
        host[:n], host[n:n + B], host[n + B:] = h_desc.view(-1), h_lam.view(torch.int32), h_desc[:, 0]
        if pixels.is_cuda:
            host = host.pin_memory()
        dev = host.to(pixels.device, non_blocking=True)
        mixed = F.image_mix(pixels, h_desc, dev[:n].view(B, MIX_FIELDS))
        return mixed, labels, labels.index_select(0, dev[n + B:]), dev[n:n + B].view(torch.float32)
