"""Cost and gain of PatchDropout (--patch_dropout, K25).  Two measurements in one process:

  1. the three *_keep kernels next to the three they replace, at B = 32 and 224 px images in 32 px and in 16 px patches (np = 49, 196),
     D = 768, in D2R_PROBE_DTYPE (default bf16): each launch between two HIP events of its own on the launching stream, the variants
     alternating launch by launch so that drift hits all alike:
         full      d2r_patchify / d2r_clip_embed_finish / d2r_clip_embed_bwd on all np patches
         keep_all  the *_keep entry point with K = np and the identity (the same bytes as full)
         keep_half the *_keep entry point with P = 0.5 (K = max(1, int(np * 0.5))), a new draw per launch
     The median, the minimum and the 90th percentile of N launches per variant (an interval between two events holds the launch's
     own overhead too, so these are upper bounds of the kernel's time).
  2. the training step (forward + backward + AdamW of ONE model, eager) for P in D2R_PROBE_RATES (default 0, 0.25, 0.5, 0.75) and
     P = 0 a second time ("off2": the run-to-run spread of P = 0), at
         C2   batch 32, 128 text tokens, 224 px images in 32 px patches: 50 image tokens, 3 classes
         C4   the BASELINE configs[3] shard: batch 8, 256 text tokens, 384 px images in 16 px patches: 577 image tokens, 7 classes
     Blocks of STEPS steps between two device events, the variants in one order in even blocks and reversed in odd ones.  Prints the
     median and the range of the per-block mean step time of each and its ratio to P = 0.

A checkout without set_patch_dropout (the parent commit, through D2R_PROBE_ROOT) runs part 2 with P = 0 only: the same box, the same
process layout, for the comparison of the P = 0 column; D2R_PROBE_KERNELS=0 D2R_PROBE_RATES=0 runs the same on this checkout.  The
last line is JSON.

    python tests/probes/patch_dropout_cost.py > profiles/patch_dropout_cost.log
    D2R_PROBE_ROOT=<checkout of the parent> python tests/probes/patch_dropout_cost.py >> profiles/patch_dropout_cost.log
    D2R_PROBE_KERNELS=0 D2R_PROBE_RATES=0 python tests/probes/patch_dropout_cost.py >> profiles/patch_dropout_cost.log
"""
import json
import os
import statistics
import sys

ROOT = os.environ.get("D2R_PROBE_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

import d2r_amd
from d2r_amd import functional as F
from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.params import FusedAdamW, ParamStore

LAUNCHES = int(os.environ.get("D2R_PROBE_LAUNCHES", "200"))
STEPS = int(os.environ.get("D2R_PROBE_STEPS", "10"))   # steps per block
BLOCKS = int(os.environ.get("D2R_PROBE_BLOCKS", "6"))  # blocks per variant
RATES = [float(r) for r in os.environ.get("D2R_PROBE_RATES", "0,0.25,0.5,0.75").split(",")]
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}[os.environ.get("D2R_PROBE_DTYPE", "bf16")]
SHAPES = {"C2": dict(B=32, L=128, S=224, patch=32, classes=3), "C4": dict(B=8, L=256, S=384, patch=16, classes=7)}
WARMUP = 20
HAS_FEATURE = hasattr(M.UnimoModel, "set_patch_dropout")
d2r_amd.configure_runtime()
dev = torch.device("cuda:0")
CODE = {torch.bfloat16: F._lib.BF16, torch.float16: F._lib.F16}[DTYPE]
res = {"root": "this checkout" if not os.environ.get("D2R_PROBE_ROOT") else "D2R_PROBE_ROOT", "dtype": str(DTYPE)[6:], "feature": HAS_FEATURE,
       "launches": LAUNCHES, "steps": STEPS, "blocks": BLOCKS, "kernels": {}, "steps_ms": {}}
print(f"PatchDropout cost probe: {res['root']}, {res['dtype']}, feature {'present' if HAS_FEATURE else 'absent (P = 0 only)'}", flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def summarise(tag, events):
    out = {}
    for name, evs in events.items():
        us = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
        out[name] = {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2)}
        print(f"  {tag:44s} {name:9s}: median {out[name]['median_us']:7.2f} us, min {out[name]['min_us']:7.2f} us, "
              f"p90 {out[name]['p90_us']:7.2f} us over {len(us)} launches", flush=True)
    return out


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------
def kernels(B, S, p, D=768):
    from d2r_amd.patch_dropout import PatchDropout
    n, Kd = (S // p) ** 2, 3 * p * p
    g = torch.Generator().manual_seed(0)
    px = torch.randn(B, 3, S, S, generator=g).to(dev)
    cls, pos = torch.randn(D, generator=g).to(dev), torch.randn(1 + n, D, generator=g).to(dev)
    sampler = PatchDropout(0.5, n, seed=0)
    K = sampler.K
    ident = torch.arange(n, dtype=torch.int32).repeat(B, 1)
    ident_d = ident.to(dev)
    draws = []
    for _ in range(WARMUP + LAUNCHES):
        h = sampler.draw(B)
        draws.append((h, h.to(dev)))
    patches = torch.empty(B * n, Kd, dtype=DTYPE, device=dev)
    x = torch.randn(B, 1 + n, D, generator=g).to(DTYPE).to(dev)  # finish works in place: the values drift, the bytes do not
    dcls, dpos = torch.empty(D, device=dev), torch.empty(1 + n, D, device=dev)
    st = F._stream()
    call = F._lib.call
    trios = {
        f"patchify B={B} {S}/{p} np={n} K={K}": lambda h, d: [
            ("full", lambda: call("d2r_patchify", CODE, px.data_ptr(), B, S, S, p, patches.data_ptr(), st)),
            ("keep_all", lambda: call("d2r_patchify_keep", CODE, px.data_ptr(), B, S, S, p, ident.data_ptr(), ident_d.data_ptr(), n, patches.data_ptr(), st)),
            ("keep_half", lambda: call("d2r_patchify_keep", CODE, px.data_ptr(), B, S, S, p, h.data_ptr(), d.data_ptr(), K, patches.data_ptr(), st))],
        f"clip_embed_finish B={B} np={n} K={K} D={D}": lambda h, d: [
            ("full", lambda: call("d2r_clip_embed_finish", CODE, x.data_ptr(), cls.data_ptr(), pos.data_ptr(), B, 1 + n, D, st)),
            ("keep_all", lambda: call("d2r_clip_embed_finish_keep", CODE, x.data_ptr(), cls.data_ptr(), pos.data_ptr(), ident.data_ptr(), ident_d.data_ptr(), B, n, n, D, st)),
            ("keep_half", lambda: call("d2r_clip_embed_finish_keep", CODE, x.data_ptr(), cls.data_ptr(), pos.data_ptr(), h.data_ptr(), d.data_ptr(), B, K, n, D, st))],
        f"clip_embed_bwd B={B} np={n} K={K} D={D}": lambda h, d: [
            ("full", lambda: call("d2r_clip_embed_bwd", CODE, x.data_ptr(), B, 1 + n, D, dcls.data_ptr(), dpos.data_ptr(), st)),
            ("keep_all", lambda: call("d2r_clip_embed_bwd_keep", CODE, x.data_ptr(), ident.data_ptr(), ident_d.data_ptr(), B, n, n, D, dcls.data_ptr(), dpos.data_ptr(), st)),
            ("keep_half", lambda: call("d2r_clip_embed_bwd_keep", CODE, x.data_ptr(), h.data_ptr(), d.data_ptr(), B, K, n, D, dcls.data_ptr(), dpos.data_ptr(), st))],
    }
    for tag, make in trios.items():
        x.normal_()
        events = {"full": [], "keep_all": [], "keep_half": []}
        for k, (h, d) in enumerate(draws):
            trio = make(h, d)
            for name, fn in trio[k % 3:] + trio[:k % 3]:
                ev = timed(fn)
                torch.cuda.synchronize()  # one variant in flight at a time
                if k >= WARMUP:
                    events[name].append(ev)
        res["kernels"][tag] = summarise(tag, events)


if HAS_FEATURE and os.environ.get("D2R_PROBE_KERNELS", "1") != "0":
    print("1. kernels (interval between two HIP events around one launch):", flush=True)
    kernels(32, 224, 32)
    kernels(32, 224, 16)


# ---- 2. the training step ----------------------------------------------------------------------------------------------------
def steps(tag, B, L, S, patch, classes):
    torch.manual_seed(2023)
    model = M.UnimoModelF(default_args(DR_step=3), VisionConfig(num_hidden_layers=12, image_size=S, patch_size=patch),
                          TextConfig(num_hidden_layers=12, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), num_classes=classes)
    model.to(dev).set_compute_dtype(DTYPE).train()
    store = ParamStore(model, DTYPE)
    opt = FusedAdamW(store, lr=3e-5)
    if DTYPE == torch.float16:
        opt.enable_loss_scaling()
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1000, 30000, (B, L), generator=g)
    ids[:, 0] = 101
    batch = tuple(t.to(dev) for t in (ids, torch.ones(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long),
                                      torch.randint(0, classes, (B,), generator=g), torch.randn(B, 3, S, S, generator=g)))

    def step():
        loss, _ = model(*batch)
        opt.backward(loss)
        opt.step()
        opt.zero_grad()
        return loss

    def set_rate(p):
        if HAS_FEATURE:
            model.model.set_patch_dropout(p, 2023, 0)

    rates = {f"P={p:g}": p for p in (RATES if HAS_FEATURE else [0.0])}
    rates["off2"] = 0.0
    order = list(rates)
    times = {k: [] for k in order}
    for k in order:
        set_rate(rates[k])
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for blk in range(BLOCKS):
        for k in (order if blk % 2 == 0 else order[::-1]):
            set_rate(rates[k])
            step()  # the first step after a switch is not timed
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(STEPS):
                loss = step()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / STEPS)
    assert bool(torch.isfinite(loss))
    n = (S // patch) ** 2
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"  {tag} step, {str(DTYPE)[6:]}, eager: batch {B}, {L} text tokens, {1 + n} image tokens; {STEPS} steps x {BLOCKS} blocks per variant, "
          "order reversed every other block", flush=True)
    for k in order:
        ntok = 1 + n if rates[k] == 0.0 else 1 + max(1, int(n * (1.0 - rates[k])))
        print(f"    {k:7s} ({ntok:3d} image tokens): {med[k]:8.3f} ms [{min(times[k]):8.3f}, {max(times[k]):8.3f}]  x{med[k] / med['P=0']:.3f} of P=0", flush=True)
    res["steps_ms"][tag] = {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}
    del model, store, opt


print("2. training steps:", flush=True)
for tag, shape in SHAPES.items():
    steps(tag, **shape)
    torch.cuda.empty_cache()
print(json.dumps(res))
