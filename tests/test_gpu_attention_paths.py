"""Every dispatch path of the attention cores (d2r_amd/csrc/attention.hip, attention_impl.inc, xattn2.hip, xattn3.hip) against fp64,
through the raw C ABI: d2r_mha_fwd / bwd, d2r_xattn_fwd / bwd, d2r_xattn_fwd_multi / bwd_multi.

Each case names the kernel variants it must reach, in launch order (d2r_attn_trace, include/d2r_hip_probes.h), so a change of a
dispatch rule cannot quietly move a case to another kernel; `test_every_variant_has_a_case` compares the table with the list of codes
the library defines.  Operands are made of values that are exact in bf16 AND fp16 (8 significant bits, magnitude in fp16's normal
range), so one fp64 reference per shape serves both types:

    S = scale Q K^T + mask     P = softmax(S)     O = (Z o P) V + residual     lse = logsumexp(S)      (Z = keep / (1 - p), or 1)
    dV = (Z o P)^T dO     dP = Z o (dO V^T)     D = rowsum(P o dP)     dS = P o (dP - D)     dQ = scale dS K     dK = scale dS^T Q

Per element, with u half an ulp of the 16-bit type (2^-8 bf16, 2^-11 fp16):

    |got - ref| <= u |ref| + C u M + tiny
    M(o)  = (Z o P) |V|                        M(dv) = (Z o P)^T |dO|
    M(dq) = scale (P o (|dP| + Dbar)) |K|      M(dk) = scale (P o (|dP| + Dbar))^T |Q|
    Dbar  = rowsum(|dO| o (|O| + |residual|))
    lse:  |got - ref| <= C 2^-24 (|lse| + max_k |S| + sum_k P_k scale (|Q| |K|^T)_k)
          (the last term is the condition of the fp32 score product itself: at Lk = 1 lse IS the score, and a score that cancels to
           near zero carries the rounding of its 64 .. 768 products; without it the rounding model below misses the bound 600-fold)
    tiny  = 2^-25 (1 + n max|operand| max(1, scale)) for fp16 (below 2^-14 fp16 is subnormal, absolute spacing 2^-24: the stored output
            itself, and the n rounded probabilities or dS - some kernels round scale * dS - that enter a product), 2^-100 otherwise

and where M is exactly zero (keys under the -10000 mask: exp(-10000 + O(100)) is 0 in fp32 and in fp64) the result must BE zero.
C is not fitted to the kernels: `_reference(..., dt)` is an fp64 model that rounds where the kernels are documented to round (scores from an fp32
product, P to 16 bits before the value product, dS to 16 bits, D from the rounded O, every output to 16 bits);
`test_bound_constant_from_the_emulation` (no GPU) evaluates it over the case table and C = 3 x its worst ratio - the factor for what the
model leaves out (fp32 summation order over up to 1024 keys, the hardware exponential).

    worst emulated ratio over the table (CPU):  o 0.96, o with residual 1.64, lse 1.55, dq 1.33, dk 1.42, dv 0.99 (C is kept per
                                                output: EMULATED_WORST below; > 4 for o with a residual, lse, dq, dk: the model's own
                                                double rounding of P V + residual, D from the rounded O, the 768-deep fp32 score sum)
    worst measured ratio on an MI355X:          2.08 (lse, xattn2<1,640>), 1.38 (o, xattn2<1,640>), <= 1.26 for every other variant
                                                and output; per variant and type in profiles/attention_paths_ratios.md

Every case also runs with INDICATOR operands (`probe`): V[b, k, c] = [c mod W == k mod W] and dO[b, q, c] = [c mod W == q mod W] (W = 768,
or head_dim), which makes o the summed probability of the keys congruent to its column and dv[k, c] the probability P[q = c, k]: a
missing, repeated or permuted key or query moves its element by 100 %, which the random-input bound cannot see at one key in 577.

Every output lives inside a larger buffer of the all-ones byte pattern (NaN in bf16, fp16 and fp32): two rows before and after, row
padding, batch gaps, the other slots of a packed [B, L, 3E] / [B, L, 2E] gradient.  Outside the output rectangles it must come back
bit-identical; inside it starts as NaN, so a skipped element shows.  P / dS / dsum scratch starts as NaN.  Every case runs twice and
must be bit-identical to itself."""
import ctypes as C
import functools
import math

import pytest
import torch

from test_gpu_gemm_paths import BF, H as FP16, U, _bits, _code, _nan_like

LOWP = [BF, FP16]
LOWP_IDS = ["bf16", "fp16"]
E768 = 768
# worst ratio |emulated - ref| / (u |ref| + u M + tiny) of the rounding model over CASES x {bf16, fp16} x {random, probe}, printed and
# re-checked by test_bound_constant_from_the_emulation; C = 3 x this figure
EMULATED_WORST = dict(o=1.0, o_res=1.7, lse=1.6, dq=1.4, dk=1.45, dv=1.0)
CBOUND = {k: 3.0 * v for k, v in EMULATED_WORST.items()}

# variant codes (d2r_amd/csrc/attn_trace.h)
X3F, X3B, DKV, DKV2 = 60001, 60002, 60003, 60004
X2_2_256, X2_1_256, X2_1_640 = 60011, 60012, 60013
XB2, XB5, KGRP, KDV, KDK = 60021, 60022, 60031, 60032, 60033


def MF(dh, nk):  # MHA short forward / backward, long forward / dQ / dK-dV
    return 10000 + dh * 100 + nk


def MB(dh, nk):
    return 20000 + dh * 100 + nk


def ML(dh):
    return [30000 + dh * 100], [40000 + dh * 100, 50000 + dh * 100]


# ---------------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------------
SPEC = dict(fam="x", B=2, Lq=16, Lk=16, H=1, dh=768, ncore=1, scale=1.0, gen="rand", res=False, mask=None, layout="plain",
            lkp_extra=0, p=0.0, seed=1234, h_o=True, fwd=None, bwd=None, api="multi", huge=False, probe=True)
CASES = []


def case(name, **kw):
    s = dict(SPEC, **kw)
    s["id"] = name
    assert s["fwd"] is not None
    CASES.append(s)


def mha(Lq, Lk, dh, H, **kw):
    kw.setdefault("B", 2)
    kw.setdefault("scale", 1.0 / math.sqrt(dh))
    if Lq <= 256 and Lk <= 256:
        fwd, bwd = [MF(dh, -(-Lk // 32))], [MB(dh, -(-max(Lq, Lk) // 32))]
    else:
        fwd, bwd = ML(dh)
    # (the expected codes are spelled out from the documented rule: NK32 = ceil(Lk / 32) forward, ceil(max(Lq, Lk) / 32) backward)
    tag = "".join("-%s%s" % (k, v) for k, v in sorted(kw.items()) if k in ("mask", "layout", "p", "gen", "res") and v)
    case("mha-%dx%d-d%d-h%d%s" % (Lq, Lk, dh, H, tag), fam="mha", Lq=Lq, Lk=Lk, dh=dh, H=H, fwd=fwd, bwd=bwd, **kw)


def xat(name, Lq, Lk, fwd, bwd, **kw):
    kw.setdefault("scale", 0.25)
    case("x-%s-%dx%d" % (name, Lq, Lk), Lq=Lq, Lk=Lk, fwd=fwd, bwd=bwd, **kw)


# --- MHA, whole head in LDS: every NK32 for both head dims (forward: ceil(Lk/32); backward: ceil(max/32)), Lq != Lk both ways,
#     lengths 1, 15, 16, 17, 31, 32, 33, 255, 256 on each side, H in {1, 3, 12, 16}
mha(1, 1, 64, 1)
mha(15, 17, 48, 3, layout="pad", mask="tail")
mha(17, 15, 64, 12, res=True)
mha(16, 33, 64, 3, layout="pad", mask="mid")
mha(33, 16, 48, 16, layout="pad")
mha(31, 32, 64, 16, mask="one")
mha(32, 31, 48, 1, res=True, layout="kv")
mha(33, 64, 48, 3)
mha(64, 64, 64, 1, layout="qkv", mask="tail")
mha(65, 96, 64, 3, layout="kv")
mha(96, 65, 48, 3, mask="mid", res=True)
mha(128, 100, 48, 12, layout="pad")
mha(100, 128, 64, 3, mask="tail")
mha(160, 129, 64, 3)
mha(129, 160, 48, 3, layout="kv", mask="mid")
mha(161, 192, 48, 3)
mha(192, 161, 64, 3, layout="pad", res=True)
mha(224, 193, 64, 3, mask="one")
mha(193, 224, 48, 3)
mha(197, 197, 64, 12, layout="qkv", mask="tail")
mha(255, 256, 48, 3, layout="pad")
mha(256, 255, 64, 12, B=1, mask="mid")
mha(256, 1, 64, 3)
mha(1, 256, 48, 3, mask="tail")
mha(256, 256, 48, 16, B=1, layout="qkv", res=True)
# --- MHA, block loop (either side > 256; 128-row blocks, 16-query wave rounds), dsum given
mha(257, 257, 64, 3, B=1, layout="qkv", mask="mid")
mha(383, 385, 48, 3, B=1, layout="pad", mask="tail")
mha(385, 383, 64, 3, B=1, res=True)
mha(384, 1023, 64, 2, B=1, layout="kv")
mha(1023, 384, 48, 2, B=1, mask="mid")
mha(1024, 1, 64, 3, B=2)
mha(1, 1024, 48, 3, B=2, mask="tail")
mha(1024, 1024, 64, 1, B=1, layout="qkv", mask="one")
mha(577, 577, 48, 16, B=1, layout="pad")
# --- dropout on the probabilities against fp64 (keep mask recovered through d2r_dropout), short and long
mha(64, 60, 64, 3, p=0.1, seed=77, mask="tail")
mha(128, 128, 48, 3, p=0.5, seed=5, layout="qkv")
mha(300, 264, 64, 2, p=0.1, seed=99, B=1, res=True)
mha(257, 130, 48, 2, p=0.5, seed=3, B=2, mask="mid", layout="pad")
# --- raw scores beyond fp16's range (|Q K^T| > 65504, scale * Q K^T = O(10))
mha(64, 64, 64, 3, gen="big", scale=2.0 ** -15)
mha(260, 64, 48, 2, gen="big", scale=2.0 ** -15, B=1)

# --- xattn3 forward / query-side backward (64 queries per workgroup, 16-key tiles) + the full product kernel
V3 = dict(fwd=[X3F], bwd=[X3B, DKV])
V3_TO_2 = dict(fwd=[X3F], bwd=[XB2, KGRP])  # Lq > 256 (or lkp > 256, or no h_o): the query side falls back to the second generation
xat("v3", 1, 1, **V3)
xat("v3", 15, 7, layout="pad", mask="tail", **V3)
xat("v3", 16, 8, res=True, scale=1.0, **V3)
xat("v3", 17, 9, layout="kv", **V3)
xat("v3", 63, 15, mask="mid", **V3)
xat("v3", 64, 16, layout="align4", **V3)
xat("v3", 65, 17, layout="pad", res=True, mask="one", **V3)
xat("v3", 255, 31, lkp_extra=24, **V3)
xat("v3", 256, 33, layout="kv", mask="mid", **V3)
xat("v3", 128, 256, B=1, mask="tail", **V3)
xat("v3", 33, 249, layout="align4", mask="mid", **V3)
xat("v3", 64, 255, res=True, scale=1.0, layout="pad", **V3)
xat("v3-qkv", 128, 128, layout="qkv", mask="tail", **V3)
xat("v3-unit", 128, 197, gen="unit", scale=100.0 / math.sqrt(768.0), mask="tail", **V3)
xat("v3-res", 197, 128, scale=1.0, gen="half", res=True, **V3)
xat("v3-big", 64, 48, gen="big", scale=2.0 ** -15, **V3)
xat("v3-single", 40, 24, api="single", fwd=[X3F], bwd=[XB2])
xat("v3to2", 257, 249, B=1, **V3_TO_2)
xat("v3to2", 577, 255, B=1, layout="kv", mask="mid", **V3_TO_2)
xat("v3to2-lkp", 33, 249, lkp_extra=24, **V3_TO_2)  # lkp = 280 > 256: the documented fall-back
xat("v3to2-no-o", 64, 64, h_o=False, layout="pad", **V3_TO_2)
xat("v3to2-split", 48, 100, h_o=False, layout="split", mask="tail", fwd=[X3F], bwd=[XB2, KDV, KDK])
# --- product kernels: roundup8(B) * ngroup > 256 from both sides, the compact kernel's own shape rule from both sides
xat("dkv-216", 128, 197, ncore=3, B=24, probe=False, **V3)
xat("dkv2-288", 128, 197, ncore=3, B=32, res=[True, False, True], fwd=[X3F], bwd=[X3B, DKV2])
xat("dkv2-288", 197, 128, ncore=3, B=32, probe=False, layout="align4", fwd=[X3F], bwd=[X3B, DKV2])
xat("dkv-288-shape", 129, 256, ncore=3, B=32, probe=False, **V3)
xat("dkv-288-shape", 256, 256, ncore=3, B=32, probe=False, **V3)
xat("dkv2-b88", 16, 8, ncore=1, B=88, layout="kv", fwd=[X3F], bwd=[X3B, DKV2])
xat("dkv-b80", 16, 8, ncore=1, B=80, **V3)
# --- B on the XCD-mapped kernels (b = (rr / n) * 8 + xcd), ncore 1..4 with distinct tensors
xat("b1", 17, 9, B=1, **V3)
xat("b7", 17, 9, B=7, mask="tail", ncore=2, **V3)
xat("b8", 16, 16, B=8, **V3)
xat("b9", 17, 9, B=9, ncore=4, res=[True, True, False, True], mask="mid", **V3)
xat("b17", 15, 7, B=17, layout="pad", **V3)
xat("b33", 16, 8, B=33, ncore=3, mask="tail", fwd=[X3F], bwd=[X3B, DKV2])  # roundup8(33) * 9 groups = 360 > 256: compact
# --- second generation: Lk > 256 (xattn2<1,640> forward, xattn_bwd_kernel<5>), key side grouped / split
V2 = dict(fwd=[X2_1_640], bwd=[XB5, KGRP])
xat("v2", 33, 257, **V2)
xat("v2", 64, 264, layout="kv", mask="mid", **V2)
xat("v2", 128, 577, B=1, lkp_extra=24, mask="tail", **V2)
xat("v2", 100, 639, B=1, layout="pad", res=True, scale=1.0, gen="half", **V2)
xat("v2", 577, 640, B=1, mask="one", **V2)
xat("v2-qkv", 264, 264, B=1, layout="qkv", fwd=[X2_1_640], bwd=[XB5, KDV, KDK])
xat("v2-split", 31, 300, layout="split", ncore=2, fwd=[X2_1_640], bwd=[XB5, KDV, KDK])
xat("v2-unit", 197, 577, B=1, gen="unit", scale=100.0 / math.sqrt(768.0), **V2)
xat("v2-big", 32, 272, gen="big", scale=2.0 ** -15, **V2)
xat("v2-b9", 17, 257, B=9, mask="tail", **V2)
xat("v2-b33", 16, 264, B=33, ncore=2, probe=False, **V2)
xat("v2-single", 40, 300, api="single", fwd=[X2_1_640], bwd=[XB5])
# --- xattn2<2,256> / <1,256>: reachable only when a per-sample offset of K or V does not fit 32 bits (ld * Lk >= 2^31).  Lk = 2 with
#     a row stride of 2^30 elements: two 2-GiB operands, every byte the kernel reads inside them; Lq on either side of
#     ceil(Lq / 32) * B * ncore = 192.  (xattn2.hip forms every row offset in 64 bits: `src + (int64_t)key * ld`, `(int64_t)qrow * a.ldq`.)
xat("x2-huge-16q", 6112, 2, B=1, huge=True, fwd=[X2_1_256], bwd=None)
xat("x2-huge-32q", 6113, 2, B=1, huge=True, mask="none0", fwd=[X2_2_256], bwd=None)

CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# ---------------------------------------------------------------------------------------------------------------------------
# operands and the fp64 reference (CPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _exact16(t):
    """Values exact in bf16 and in fp16: 8 significant bits, |x| in [2^-14, 65504] or zero."""
    t = t.to(torch.bfloat16).double()
    t[t.abs() < 2.0 ** -14] = 0.0
    assert float(t.abs().max()) < 65000.0
    return t


def _mask_for(kind, B, Lk, g):
    if kind is None or Lk < 2:
        return None
    m = torch.zeros(B, Lk, dtype=torch.float64)
    for b in range(B):
        if kind == "tail":      # a different number of trailing masked keys per sample
            n = min(Lk - 1, 1 + (5 * b + 3) % max(1, Lk // 2))
            m[b, Lk - n:] = -10000.0
        elif kind == "mid":     # masked keys in the middle, straddling a 16-key tile and a 128-row block
            for lo, hi in ((Lk // 3 - 2 + b, Lk // 3 + 3 + b), (122 + b, 133), (12, 19 - b % 2)):
                if 0 < lo < hi < Lk:
                    m[b, lo:hi] = -10000.0
        elif kind == "one":     # one sample with a single unmasked key, the others a tail
            if b == 0:
                m[b] = -10000.0
                m[b, (2 * Lk) // 3] = 0.0
            else:
                m[b, Lk - 1:] = -10000.0
        elif kind == "none0":   # zeros: the mask pointer is given, nothing is masked
            pass
    return m


def _operands(c, probe):
    """fp64 CPU operands (exact in both 16-bit types) per core: q, k, v, g (= dO), res; and the additive mask."""
    g = torch.Generator().manual_seed(zlib_seed(c["id"]))
    B, Lq, Lk, H, dh, W = c["B"], c["Lq"], c["Lk"], c["H"], c["dh"], c["H"] * c["dh"]
    cores = []
    for core in range(c["ncore"]):
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        q, k, v, go = r(B, Lq, W), r(B, Lk, W), r(B, Lk, W), r(B, Lq, W)
        if c["gen"] == "unit":
            q, k = q / q.norm(dim=-1, keepdim=True), k / k.norm(dim=-1, keepdim=True)
        elif c["gen"] == "half":
            q, k = 0.5 * q, 0.5 * k
        elif c["gen"] == "big":   # |q . k| ~ sqrt(dh) * 2048 * 16 (MHA) or sqrt(768) * 1024 * 8: far beyond 65504
            q, k = (2048.0 if c["fam"] == "mha" else 1024.0) * q, (16.0 if c["fam"] == "mha" else 8.0) * k
        if probe:
            col = torch.arange(W) % dh
            v = (col[None, :] == (torch.arange(Lk) % dh)[:, None]).double().expand(B, Lk, W).clone()
            go = (col[None, :] == (torch.arange(Lq) % dh)[:, None]).double().expand(B, Lq, W).clone()
        want_res = c["res"][core] if isinstance(c["res"], list) else c["res"]
        res = _exact16(r(B, Lq, W)) if (want_res and not probe) else None
        cores.append(dict(q=_exact16(q), k=_exact16(k), v=_exact16(v), g=_exact16(go), res=res))
    return cores, _mask_for(c["mask"], B, Lk, g)


def zlib_seed(s):
    import zlib
    return zlib.crc32(s.encode()) & 0x7FFFFFFF


def _heads(t, H, dh):
    return t.view(t.shape[0], t.shape[1], H, dh).transpose(1, 2)  # [B, H, L, dh]


def _merge(t):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)


def _reference(c, ops, mask, Z, dt=None):
    """fp64 truth (dt None) or the rounding model of the kernels (dt given).  Returns per-core dicts of o, lse, dq, dk, dv and the
    condition terms M of the bound.  Z: [B, H, Lq, Lk] keep / (1 - p), or None."""
    H, dh, scale = c["H"], c["dh"], c["scale"]
    rnd = (lambda t: t) if dt is None else (lambda t: t.to(dt).double())
    out = []
    for op in ops:
        q, k, v, g = (_heads(op[n], H, dh) for n in ("q", "k", "v", "g"))
        res = op["res"]
        if dt is None:
            S = scale * (q @ k.transpose(-1, -2))
        else:  # scores from an fp32 product
            S = (q.float() @ k.float().transpose(-1, -2) * scale).double()
        if mask is not None:
            S = S + mask[:, None, None, :]
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        if dt is not None:
            lse = lse.float().double()
        ZP = P if Z is None else Z * P
        ZPr = rnd(ZP)
        pv = rnd(ZPr @ v)
        o = _merge(pv) if res is None else rnd(_merge(pv) + res)
        dV = rnd(ZPr.transpose(-1, -2) @ g)
        dP = g @ v.transpose(-1, -2)
        if Z is not None:
            dP = Z * dP
        if dt is None:
            D = (P * dP).sum(-1, keepdim=True)
        else:  # D from the rounded output
            D = (g * _heads(o if res is None else o - res, H, dh)).sum(-1, keepdim=True)
        dS = rnd(P * (dP - D))
        dQ, dK = rnd(scale * (dS @ k)), rnd(scale * (dS.transpose(-1, -2) @ q))
        r = dict(o=o, lse=lse, dq=_merge(dQ), dk=_merge(dK), dv=_merge(dV))
        if dt is None:
            oabs = _heads(o.abs() + (0 if res is None else res.abs()), H, dh)
            env = P * (dP.abs() + (g.abs() * oabs).sum(-1, keepdim=True))
            r["M"] = dict(o=_merge(ZP @ v.abs()), dv=_merge(ZP.transpose(-1, -2) @ g.abs()), dq=_merge(scale * (env @ k.abs())),
                          dk=_merge(scale * (env.transpose(-1, -2) @ q.abs())),
                          lse=lse.abs() + S.abs().amax(-1) + (P * (scale * (q.abs() @ k.abs().transpose(-1, -2)))).sum(-1))
            r["has_res"] = res is not None
            big = max(1.0, scale)
            h = 2.0 ** -25  # half the spacing of fp16's subnormals: the output itself, and each of the n rounded factors P or dS
            r["tiny16"] = dict(o=h * (1 + c["Lk"] * float(v.abs().max())), dv=h * (1 + c["Lq"] * float(g.abs().max())),
                               dq=h * (1 + c["Lk"] * float(k.abs().max()) * big), dk=h * (1 + c["Lq"] * float(q.abs().max()) * big))
        out.append(r)
    return out


def _ratio(name, got, ref, dt):
    """max over elements of |got - ref| / (u |ref| + u M + tiny) for the 16-bit outputs, / (2^-24 (|lse| + max |S|)) for lse: the unit in
    which the emulation and the measurements are reported."""
    M = ref["M"][name]
    if name == "lse":
        return float(((got - ref[name]).abs() / (2.0 ** -24 * M + 2.0 ** -100)).max())
    tiny = ref["tiny16"][name] if dt == FP16 else 2.0 ** -100
    return float(((got - ref[name]).abs() / (U[dt] * ref[name].abs() + U[dt] * M + tiny)).max())


def _check(name, got, ref, dt, what):
    """|got - ref| <= u |ref| + C u M + tiny per element; exactly zero where M is.  Returns the worst |err| / (u |ref| + u M + tiny)."""
    M, want = ref["M"][name], ref[name]
    cb = CBOUND["o_res" if (name == "o" and ref["has_res"]) else name]
    assert torch.isfinite(got).all(), "%s: %s has non-finite elements (%d)" % (what, name, int((~torch.isfinite(got)).sum()))
    err = (got - want).abs()
    if name == "lse":
        bound = cb * 2.0 ** -24 * M
    else:
        tiny = ref["tiny16"][name] if dt == FP16 else 2.0 ** -100
        bound = U[dt] * want.abs() + cb * U[dt] * M + tiny
        dead = M == 0  # (then ref is 0, or the residual alone: exact in 16 bits)
        assert (got[dead] == want[dead]).all(), "%s: %s is not exactly zero where every contributing probability is masked" % (what, name)
    ratio = _ratio(name, got, ref, dt)
    bad = err > bound
    if bad.any():
        i = int((err - bound).argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError("%s: %s misses the bound at %d of %d elements; worst at %s: got %.9g ref %.9g bound %.3g (ratio %.2f, C = %.2f)"
                             % (what, name, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx]), float(bound[idx]),
                                ratio, cb))
    return ratio


@functools.lru_cache(maxsize=2)
def _truth_cached(case_index, probe, zkey):
    c = CASES[case_index]
    ops, mask = _operands(c, probe)
    Z = _ZSTORE.get(zkey)
    return ops, mask, _reference(c, ops, mask, Z)


_ZSTORE = {}


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests: the bound's constant, the coverage of the table
# ---------------------------------------------------------------------------------------------------------------------------
def _cpu_cost(c):
    return c["ncore"] * c["B"] * c["H"] * c["Lq"] * c["Lk"]


def test_bound_constant_from_the_emulation():
    """Evaluates the rounding model over the case table (both types, random and indicator operands) and prints the worst ratio per
    output; C = 3 x the figure recorded in EMULATED_WORST, which must cover what is measured here."""
    worst = {}
    for ci, c in enumerate(CASES):
        for probe in ((False, True) if c["probe"] else (False,)):
            ops, mask = _operands(c, probe)
            Z = None
            if c["p"] > 0:  # any keep mask of that rate serves the model
                g = torch.Generator().manual_seed(c["seed"])
                Z = (torch.rand(c["B"], c["H"], c["Lq"], c["Lk"], generator=g) >= c["p"]).double() / (1.0 - c["p"])
            ref = _reference(c, ops, mask, Z)
            for dt in LOWP:
                em = _reference(c, ops, mask, Z, dt)
                for r, e in zip(ref, em):
                    for name in ("o", "lse", "dq", "dk", "dv"):
                        key = ("o_res" if (name == "o" and r["has_res"]) else name, "fp16" if dt == FP16 else "bf16")
                        x = _ratio(name, e[name], r, dt)
                        if x > worst.get(key, (0.0, ""))[0]:
                            worst[key] = (x, c["id"] + ("/probe" if probe else ""))
    for key in sorted(worst):
        print("emulated worst ratio %-5s %s: %.3f  (%s)" % (key[0], key[1], worst[key][0], worst[key][1]))
    for name, recorded in EMULATED_WORST.items():
        top = max(v[0] for k, v in worst.items() if k[0] == name)
        print("%-5s emulated worst %.3f, recorded %.2f -> C = %.2f" % (name, top, recorded, CBOUND[name]))
        # (the fp32 score product of the emulation is the CPU BLAS's: its summation order, and with it the last digits of these
        #  figures, depends on the machine - hence rounded-up records and a 10 % band on either side)
        assert top <= 1.1 * recorded, "%s: the emulation exceeds the recorded figure; EMULATED_WORST must say %.3f" % (name, top)
        assert recorded <= 1.1 * top + 0.01, "%s: the recorded figure %.2f is looser than the emulation (%.3f)" % (name, recorded, top)


def test_every_variant_has_a_case():
    from d2r_amd import _lib
    lib = _lib.load()
    n = lib.d2r_attn_trace_codes(None, 0)
    buf = (C.c_int * n)()
    assert lib.d2r_attn_trace_codes(buf, n) == n
    defined = set(buf)
    covered = set()
    for c in CASES:
        covered |= set(c["fwd"]) | set(c["bwd"] or [])
    assert covered <= defined, "the table expects codes the library does not define: %s" % sorted(covered - defined)
    assert defined <= covered, "variants without a case: %s" % sorted(defined - covered)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: NaN-guarded buffers, the calls
# ---------------------------------------------------------------------------------------------------------------------------
class Arena:
    """A flat all-ones-bytes buffer with rectangles [B, L, W] inside it (row stride ld, batch stride sb, offset off)."""

    def __init__(self, dt, n, dev):
        self.dt, self.flat, self.rects = dt, _nan_like(n, dt, dev), []
        assert self.flat.data_ptr() % 256 == 0

    def rect(self, off, B, L, W, ld, sb):
        self.rects.append((off, B, L, W, ld, sb))
        return torch.as_strided(self.flat, (B, L, W), (sb, ld, 1), off)

    def ptr(self, off):
        return self.flat.data_ptr() + off * self.flat.element_size()

    def outside_intact(self):
        out = torch.ones(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        for off, B, L, W, ld, sb in self.rects:
            torch.as_strided(out, (B, L, W), (sb, ld, 1), off).fill_(False)
        return bool((_bits(self.flat)[out] == -1).all())


class T:
    """One [B, L, W] tensor of a call: its arena, view, pointer and strides."""

    def __init__(self, arena, off, B, L, W, ld, sb):
        self.arena, self.off, self.ld, self.sb = arena, off, ld, sb
        self.view = arena.rect(off, B, L, W, ld, sb)
        self.ptr = arena.ptr(off)

    def set(self, t64):
        self.view.copy_(t64.to(self.view.dtype))
        return self

    def get(self):
        return self.view.double().cpu()


def _slots(dt, dev, B, L, W, nslot=1, pad=0, gap=0, guard=2, shift=0):
    """nslot tensors [B, L, W] side by side in one arena: ld = nslot * W + pad, sb = L * ld + gap, `guard` rows before and after."""
    ld = nslot * W + pad
    sb = L * ld + gap
    off = guard * ld + shift
    arena = Arena(dt, off + (B - 1) * sb + L * ld + guard * ld + 8, dev)
    return [T(arena, off + s * W, B, L, W, ld, sb) for s in range(nslot)]


def _vec32(dev, n):
    """fp32 [n] inside a NaN arena with 8 guard elements on each side."""
    a = Arena(torch.float32, n + 16, dev)
    t = T(a, 8, 1, 1, n, n, n)
    return t


def _stream():
    from d2r_amd.functional import _stream as s
    return s()


def _parr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _trace_begin():
    from d2r_amd import _lib
    _lib.load().d2r_attn_trace(1)


def _trace_end():
    from d2r_amd import _lib
    lib = _lib.load()
    n = lib.d2r_attn_trace_read(None, 0)
    buf = (C.c_int * max(n, 1))()
    lib.d2r_attn_trace_read(buf, n)
    lib.d2r_attn_trace(0)
    return [buf[i] for i in range(n)]


def _keep_scale(c, dev):
    """Z = keep / (1 - p) [B, H, Lq, Lk] from d2r_dropout on ones: element index ((b * H + h) * Lq + q) * lkp + key, lkp = roundup8(Lk)."""
    from d2r_amd import _lib
    lkp = (c["Lk"] + 7) // 8 * 8
    n = c["B"] * c["H"] * c["Lq"] * lkp
    ones, y = torch.ones(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    assert _lib.load().d2r_dropout(_lib.F32, ones.data_ptr(), None, y.data_ptr(), n, C.c_float(c["p"]), c["seed"], _stream()) == 0
    keep = (y != 0).view(c["B"], c["H"], c["Lq"], lkp)[..., :c["Lk"]].double().cpu()
    frac = float(keep.mean())
    assert abs(frac - (1.0 - c["p"])) < 0.05, "keep rate %.3f for p = %.2f" % (frac, c["p"])
    return keep / (1.0 - c["p"])


LAYOUTS = {  # name -> (input pad, input gap) ; o / res / dO / gradients follow below
    "plain": (0, 0), "pad": (8, 24), "qkv": (8, 24), "kv": (8, 24), "split": (8, 24), "align4": (0, 0)}


def _build(c, dt, dev, ops, mask):
    """All device tensors of one run (per core): inputs filled, outputs / scratch NaN."""
    B, Lq, Lk, W = c["B"], c["Lq"], c["Lk"], c["H"] * c["dh"]
    lay = c["layout"]
    pad, gap = LAYOUTS[lay]
    lkp = (Lk + 7) // 8 * 8 + c["lkp_extra"]
    cores = []
    for op in ops:
        t = {}
        if c["huge"]:      # K / V rows 2^30 elements apart, no guard rows (they would be rows of 2 GiB)
            t["q"], = _slots(dt, dev, B, Lq, W)
            for n in ("k", "v"):
                arena = Arena(dt, (Lk - 1) * 2 ** 30 + W + 8, dev)
                t[n] = T(arena, 0, B, Lk, W, 2 ** 30, Lk * 2 ** 30)
        elif lay == "qkv":
            assert Lq == Lk
            t["q"], t["k"], t["v"] = _slots(dt, dev, B, Lq, W, 3, 0, gap)
        elif lay == "kv":
            t["q"], = _slots(dt, dev, B, Lq, W, 1, pad, gap)
            t["k"], t["v"] = _slots(dt, dev, B, Lk, W, 2, 0, gap)
        else:
            t["q"], = _slots(dt, dev, B, Lq, W, 1, pad, gap)
            t["k"], = _slots(dt, dev, B, Lk, W, 1, pad, gap)
            t["v"], = _slots(dt, dev, B, Lk, W, 1, pad, gap)
        for n in ("q", "k", "v"):
            t[n].set(op[n])
        t["g"] = _slots(dt, dev, B, Lq, W, 1, pad, gap)[0].set(op["g"])
        t["o"], = _slots(dt, dev, B, Lq, W, 1, pad, gap)
        t["res"] = _slots(dt, dev, B, Lq, W, 1, pad, gap)[0].set(op["res"]) if op["res"] is not None else None
        # gradients: packed beside each other (and NaN) where the inputs are packed
        if lay == "qkv":
            t["dq"], t["dk"], t["dv"] = _slots(dt, dev, B, Lq, W, 3, 0, gap)
        elif lay == "kv":
            t["dq"], = _slots(dt, dev, B, Lq, W, 1, pad, gap)
            t["dk"], t["dv"] = _slots(dt, dev, B, Lk, W, 2, 0, gap)
        elif lay == "align4":  # what the product kernel accepts and the others do not: 8-byte aligned, ld % 4 == 0
            t["dq"], = _slots(dt, dev, B, Lq, W, 1, pad, gap)
            t["dk"], = _slots(dt, dev, B, Lk, W, 1, 4, 4, shift=4)
            t["dv"], = _slots(dt, dev, B, Lk, W, 1, 4, 4, shift=4)
            assert t["dk"].ptr % 16 == 8 and t["dk"].ld % 8 == 4
        else:
            t["dq"], = _slots(dt, dev, B, Lq, W, 1, pad, gap)
            t["dk"], = _slots(dt, dev, B, Lk, W, 1, pad, gap)
            t["dv"], = _slots(dt, dev, B, Lk, W, 1, pad + (16 if lay == "split" else 0), gap)
        t["lse"] = _vec32(dev, B * c["H"] * Lq)
        t["dsum"] = _vec32(dev, B * c["H"] * Lq)
        t["P"] = _nan_like(B * Lq * lkp + 8, dt, dev)
        t["dS"] = _nan_like(B * Lq * lkp + 8, dt, dev)
        cores.append(t)
    dmask = None if mask is None else mask.float().to(dev).contiguous()
    return cores, dmask, lkp


def _run(c, dt, dev, ops, mask):
    """Forward, then backward (from the forward's own o and lse), through the C ABI.  Returns the tensors and the two launch lists."""
    from d2r_amd import _lib
    lib = _lib.load()
    cores, dmask, lkp = _build(c, dt, dev, ops, mask)
    B, Lq, Lk, H, dh = c["B"], c["Lq"], c["Lk"], c["H"], c["dh"]
    mp = None if dmask is None else dmask.data_ptr()
    code, st, scale = _code(dt), _stream(), C.c_float(c["scale"])
    t0 = cores[0]
    rp = lambda t: (None if t["res"] is None else t["res"].ptr)
    rld, rsb = next(((t["res"].ld, t["res"].sb) for t in cores if t["res"] is not None), (0, 0))

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        assert rc == 0, "%s returned %d: %s" % (name, rc, lib.d2r_last_error().decode(errors="replace"))

    _trace_begin()
    if c["fam"] == "mha":
        call("d2r_mha_fwd", code, t0["q"].ptr, t0["q"].ld, t0["q"].sb, t0["k"].ptr, t0["k"].ld, t0["k"].sb, t0["v"].ptr, t0["v"].ld, t0["v"].sb,
             t0["o"].ptr, t0["o"].ld, t0["o"].sb, rp(t0), rld, rsb, mp, t0["lse"].ptr, B, H, Lq, Lk, dh, scale, C.c_float(c["p"]), c["seed"], st)
    elif c["api"] == "single":
        call("d2r_xattn_fwd", code, t0["q"].ptr, t0["q"].ld, t0["q"].sb, t0["k"].ptr, t0["k"].ld, t0["k"].sb, t0["v"].ptr, t0["v"].ld, t0["v"].sb,
             t0["o"].ptr, t0["o"].ld, t0["o"].sb, rp(t0), rld, rsb, mp, t0["lse"].ptr, B, Lq, Lk, E768, scale, st)
    else:
        arr = lambda n: _parr([t[n].ptr for t in cores])
        hres = None if all(t["res"] is None for t in cores) else _parr([rp(t) for t in cores])
        call("d2r_xattn_fwd_multi", code, c["ncore"], arr("q"), t0["q"].ld, t0["q"].sb, arr("k"), t0["k"].ld, t0["k"].sb, arr("v"), t0["v"].ld,
             t0["v"].sb, arr("o"), t0["o"].ld, t0["o"].sb, hres, rld, rsb, mp, arr("lse"), B, Lq, Lk, E768, scale, st)
    torch.cuda.synchronize()
    fwd = _trace_end()
    bwd = None
    if c["bwd"] is not None:
        _trace_begin()
        if c["fam"] == "mha":
            call("d2r_mha_bwd", code, t0["q"].ptr, t0["q"].ld, t0["q"].sb, t0["k"].ptr, t0["k"].ld, t0["k"].sb, t0["v"].ptr, t0["v"].ld, t0["v"].sb,
                 t0["g"].ptr, t0["g"].ld, t0["g"].sb, mp, t0["lse"].ptr, t0["dsum"].ptr, t0["dq"].ptr, t0["dq"].ld, t0["dq"].sb,
                 t0["dk"].ptr, t0["dk"].ld, t0["dk"].sb, t0["dv"].ptr, t0["dv"].ld, t0["dv"].sb, B, H, Lq, Lk, dh, scale, C.c_float(c["p"]),
                 c["seed"], st)
        elif c["api"] == "single":
            call("d2r_xattn_bwd", code, t0["q"].ptr, t0["q"].ld, t0["q"].sb, t0["k"].ptr, t0["k"].ld, t0["k"].sb, t0["v"].ptr, t0["v"].ld,
                 t0["v"].sb, t0["g"].ptr, t0["g"].ld, t0["g"].sb, mp, t0["lse"].ptr, t0["dq"].ptr, t0["dq"].ld, t0["dq"].sb,
                 t0["P"].data_ptr(), t0["dS"].data_ptr(), lkp, B, Lq, Lk, E768, scale, st)
        else:
            arr = lambda n: _parr([t[n].ptr for t in cores])
            hres = None if all(t["res"] is None for t in cores) else _parr([rp(t) for t in cores])
            call("d2r_xattn_bwd_multi", code, c["ncore"], arr("q"), t0["q"].ld, t0["q"].sb, arr("k"), t0["k"].ld, t0["k"].sb, arr("v"),
                 t0["v"].ld, t0["v"].sb, arr("g"), t0["g"].ld, t0["g"].sb, arr("o") if c["h_o"] else None, t0["o"].ld, t0["o"].sb, hres, rld, rsb,
                 mp, arr("lse"), arr("dq"), t0["dq"].ld, t0["dq"].sb, arr("dk"), t0["dk"].ld, t0["dk"].sb, arr("dv"), t0["dv"].ld, t0["dv"].sb,
                 _parr([t["P"].data_ptr() for t in cores]), _parr([t["dS"].data_ptr() for t in cores]), lkp, B, Lq, Lk, E768, scale, st)
        torch.cuda.synchronize()
        bwd = _trace_end()
    return cores, fwd, bwd


def _outputs(c):
    if c["bwd"] is None:
        return ("o", "lse")
    if c["fam"] == "x" and c["api"] == "single":
        return ("o", "lse", "dq")
    return ("o", "lse", "dq", "dk", "dv")


RATIOS = {}  # (variant code, dtype id, output) -> worst measured ratio, printed at the end of the module's run


# (case, operands, type) with the two types of one reference next to each other; a few large-batch cases run with random operands
# only: their variants have indicator runs elsewhere
RUNS = [(ci, probe, dt) for ci, c in enumerate(CASES) for probe in ((False, True) if c["probe"] else (False,)) for dt in LOWP]
RUN_IDS = ["%s-%s-%s" % (CASES[ci]["id"], "probe" if probe else "rand", "fp16" if dt == FP16 else "bf16") for ci, probe, dt in RUNS]


@pytest.mark.gpu
@pytest.mark.parametrize("ci,probe,dt", RUNS, ids=RUN_IDS)
def test_attention_path(gpu, ci, probe, dt):
    c = CASES[ci]
    zkey = None
    if c["p"] > 0:
        zkey = c["id"]
        if zkey not in _ZSTORE:
            _ZSTORE[zkey] = _keep_scale(c, gpu)
    ops, mask, ref = _truth_cached(ci, probe, zkey)
    what = "%s[%s%s]" % (c["id"], "fp16" if dt == FP16 else "bf16", ",probe" if probe else "")
    cores, fwd, bwd = _run(c, dt, gpu, ops, mask)
    assert fwd == c["fwd"], "%s: forward launched %s, the case names %s" % (what, fwd, c["fwd"])
    assert bwd == c["bwd"], "%s: backward launched %s, the case names %s" % (what, bwd, c["bwd"])
    names = _outputs(c)
    lse_shape = (c["B"], c["H"], c["Lq"])
    for k, (t, r) in enumerate(zip(cores, ref)):
        for name in names:
            got = t[name].get()
            got = got.view(lse_shape) if name == "lse" else got
            ratio = _check(name, got, r, dt, "%s core %d" % (what, k))
            for code in (c["fwd"] if name in ("o", "lse") else c["bwd"]):
                key = (code, "fp16" if dt == FP16 else "bf16", name)
                RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        arenas = {id(t[n].arena): t[n].arena for n in names}
        for a in arenas.values():
            assert a.outside_intact(), "%s core %d: bytes outside an output rectangle were written" % (what, k)
    # deterministic: a second run from fresh NaN buffers is bit-identical
    cores2, fwd2, bwd2 = _run(c, dt, gpu, ops, mask)
    assert (fwd2, bwd2) == (fwd, bwd)
    for t, t2 in zip(cores, cores2):
        for name in names:
            assert torch.equal(_bits(t[name].arena.flat), _bits(t2[name].arena.flat)), "%s: %s differs between two runs" % (what, name)


@pytest.mark.gpu
def test_print_measured_ratios(gpu):
    """(runs after the cases of this module) the worst measured |err| / (u |ref| + u M + tiny) per variant, type and output."""
    for key in sorted(RATIOS):
        print("measured worst ratio variant %d %s %-3s: %.3f" % (key[0], key[1], key[2], RATIOS[key]))
    assert all(v <= 1.0 + max(CBOUND.values()) for v in RATIOS.values())


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: non-zero status, d2r_last_error set, nothing launched, outputs untouched
# ---------------------------------------------------------------------------------------------------------------------------
def _refusal_calls(dev, dt):
    """(name, thunk, output arenas) for every refused call.  Thunks return the status."""
    from d2r_amd import _lib
    lib = _lib.load()
    st = _stream()
    code = _code(dt)
    out = []
    # ---- MHA
    B, H, dh, L = 2, 2, 64, 32
    W = H * dh
    q, k, v, g, o, dq, dk, dv = (_slots(dt, dev, B, L, W)[0] for _ in range(8))
    for t in (q, k, v, g):
        t.view.fill_(0.25)
    lse, dsum = _vec32(dev, B * H * 1025), _vec32(dev, B * H * 1025)
    arenas = [t.arena for t in (o, dq, dk, dv, lse, dsum)]

    def mfwd(code=code, dh=dh, Lq=L, Lk=L, qoff=0, ldq=q.ld, p=0.0):
        return lambda: lib.d2r_mha_fwd(code, q.ptr + qoff, ldq, q.sb, k.ptr, k.ld, k.sb, v.ptr, v.ld, v.sb, o.ptr, o.ld, o.sb, None, 0, 0, None,
                                       lse.ptr, B, H, Lq, Lk, dh, C.c_float(0.125), C.c_float(p), 1, st)

    def mbwd(code=code, dh=dh, Lq=L, Lk=L, dqoff=0, lddk=dk.ld, p=0.0, ds=dsum.ptr):
        return lambda: lib.d2r_mha_bwd(code, q.ptr, q.ld, q.sb, k.ptr, k.ld, k.sb, v.ptr, v.ld, v.sb, g.ptr, g.ld, g.sb, None, lse.ptr, ds,
                                       dq.ptr + dqoff, dq.ld, dq.sb, dk.ptr, lddk, dk.sb, dv.ptr, dv.ld, dv.sb, B, H, Lq, Lk, dh,
                                       C.c_float(0.125), C.c_float(p), 1, st)

    for tag, f, b in (("fp32", mfwd(code=_lib.F32), mbwd(code=_lib.F32)), ("head_dim=32", mfwd(dh=32), mbwd(dh=32)),
                      ("Lq=1025", mfwd(Lq=1025), mbwd(Lq=1025)), ("Lk=1025", mfwd(Lk=1025), mbwd(Lk=1025)),
                      ("pointer+2", mfwd(qoff=2), mbwd(dqoff=2)), ("ld%8", mfwd(ldq=q.ld + 4), mbwd(lddk=dk.ld + 4)),
                      ("p_drop=1", mfwd(p=1.0), mbwd(p=1.0))):
        out.append(("mha_fwd " + tag, f, arenas))
        out.append(("mha_bwd " + tag, b, arenas))
    out.append(("mha_bwd long without dsum", mbwd(Lq=257, ds=None), arenas))
    # ---- single-head cores (the same small buffers serve: nothing may be launched)
    Lx = 16
    xq, xk, xv, xg, xo, xdq, xdk, xdv = (_slots(dt, dev, B, Lx, E768)[0] for _ in range(8))
    for t in (xq, xk, xv, xg, xo):
        t.view.fill_(0.25)
    xlse = _vec32(dev, B * Lx)
    P, dS = _nan_like(B * Lx * 64, dt, dev), _nan_like(B * Lx * 64, dt, dev)
    xar = [t.arena for t in (xdq, xdk, xdv)]
    far = [_slots(dt, dev, B, Lx, E768)[0]]  # the forward's output of the refused forward calls
    xar_f = [far[0].arena, xlse.arena]

    def xfwd(code=code, ncore=1, Lk=Lx, D=E768, qoff=0, ldk=xk.ld, single=False):
        if single:
            return lambda: lib.d2r_xattn_fwd(code, xq.ptr + qoff, xq.ld, xq.sb, xk.ptr, ldk, xk.sb, xv.ptr, xv.ld, xv.sb, far[0].ptr, far[0].ld,
                                             far[0].sb, None, 0, 0, None, xlse.ptr, B, Lx, Lk, D, C.c_float(1.0), st)
        n = max(ncore, 1)
        return lambda: lib.d2r_xattn_fwd_multi(code, ncore, _parr([xq.ptr + qoff] * n), xq.ld, xq.sb, _parr([xk.ptr] * n), ldk, xk.sb,
                                               _parr([xv.ptr] * n), xv.ld, xv.sb, _parr([far[0].ptr] * n), far[0].ld, far[0].sb, None, 0, 0, None,
                                               _parr([xlse.ptr] * n), B, Lx, Lk, D, C.c_float(1.0), st)

    def xbwd(code=code, ncore=1, Lk=Lx, D=E768, qoff=0, ldk=xk.ld, lkp=Lx, h_o=True, single=False):
        if single:
            return lambda: lib.d2r_xattn_bwd(code, xq.ptr + qoff, xq.ld, xq.sb, xk.ptr, ldk, xk.sb, xv.ptr, xv.ld, xv.sb, xg.ptr, xg.ld, xg.sb, None,
                                             xlse.ptr, xdq.ptr, xdq.ld, xdq.sb, P.data_ptr(), dS.data_ptr(), lkp, B, Lx, Lk, D,
                                             C.c_float(1.0), st)
        n = max(ncore, 1)
        a = lambda p: _parr([p] * n)
        return lambda: lib.d2r_xattn_bwd_multi(code, ncore, a(xq.ptr + qoff), xq.ld, xq.sb, a(xk.ptr), ldk, xk.sb, a(xv.ptr), xv.ld, xv.sb,
                                               a(xg.ptr), xg.ld, xg.sb, a(xo.ptr) if h_o else None, xo.ld, xo.sb, None, 0, 0, None, a(xlse.ptr),
                                               a(xdq.ptr), xdq.ld, xdq.sb, a(xdk.ptr), xdk.ld, xdk.sb, a(xdv.ptr), xdv.ld, xdv.sb,
                                               a(P.data_ptr()), a(dS.data_ptr()), lkp, B, Lx, Lk, D, C.c_float(1.0), st)

    for single in (False, True):
        s = " (single)" if single else " (multi)"
        for tag, kw in (("fp32", dict(code=_lib.F32)), ("Lk=641", dict(Lk=641)), ("D=760", dict(D=760)), ("pointer+2", dict(qoff=2)),
                        ("ld%8", dict(ldk=xk.ld + 4))):
            out.append(("xattn_fwd " + tag + s, xfwd(single=single, **kw), xar_f))
            out.append(("xattn_bwd " + tag + s, xbwd(single=single, **dict(kw, lkp=648 if tag == "Lk=641" else Lx)), xar))
        out.append(("xattn_bwd lkp<Lk" + s, xbwd(single=single, lkp=8), xar))
        out.append(("xattn_bwd lkp%8" + s, xbwd(single=single, lkp=Lx + 4), xar))
    out.append(("xattn_bwd lkp<Lk without h_o", xbwd(lkp=8, h_o=False), xar))
    for n in (0, 5):
        out.append(("xattn_fwd_multi ncore=%d" % n, xfwd(ncore=n), xar_f))
        out.append(("xattn_bwd_multi ncore=%d" % n, xbwd(ncore=n), xar))
    keep = (q, k, v, g, xq, xk, xv, xg, xo, P, dS)
    return out, keep, (P, dS)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
def test_refusals_launch_nothing(gpu, dt):
    from d2r_amd import _lib
    lib = _lib.load()
    calls, _keep, scratch = _refusal_calls(gpu, dt)
    assert len(calls) >= 40
    for name, thunk, arenas in calls:
        _trace_begin()
        rc = thunk()
        torch.cuda.synchronize()
        launched = _trace_end()
        assert rc != 0, "%s was accepted" % name
        assert lib.d2r_last_error(), "%s: no error text" % name
        assert launched == [], "%s launched %s" % (name, launched)
        for a in arenas:
            assert bool((_bits(a.flat) == -1).all()), "%s wrote to an output" % name
        for s in scratch:
            assert bool((_bits(s) == -1).all()), "%s wrote to the P / dS scratch" % name
