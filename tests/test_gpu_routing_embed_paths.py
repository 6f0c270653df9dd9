"""Every host-selected path of the routing, pooling, embedding and column-sum kernels (routing.hip, the embedding kernels and SAF
products of misc.hip, d2r_colsum / d2r_colsum_add of rowops.hip, d2r_lincomb) against fp64, through the raw C ABI.

Branch (host condition that selects it)                                 Test id that reaches it
----------------------------------------------------------------------  ----------------------------------------------------------
route_aggregate, P = ncell and P = 1
  nchunk = cdiv(L, 8) = 1, 1, 1, 2, 3, 5, 9, 17                          test_route_aggregate[*-L1|L7|L8|L9|L19|L33|L65|L129-*]
    finish kernels: no trip of the 4- / 8-at-a-time loops (nchunk < 4)   ...-L1 .. L19
    full trip + remainder (nchunk = 5, 9, 17)                            ...-L33 (4+1, 8-loop short), -L65 (8+1), -L129 (16+1)
  D = VEC (RG = 128 row groups, one pack per row)                        ...-D4 (fp32), -D8 (16-bit)
  D = 64                                                                 ...-D64
  D = 400 (npk6 = 100: two row groups, 56 idle threads)                  ...-D400
  D = 768, D = 1000, D = 1024 (npk6 = 256: the P = ncell limit)          ...-D768, -D1000, -D1024
  P = 1, D / VEC = 256 (D = 2048 16-bit; fp32: 1024)                     test_route_aggregate[*-P1-D2048-*], [fp32-P1-D1024-*]
  ncell = 2 .. 6 (stand-in pointers, demb5 NULL, e5 zeroed for nc < 6)   ...-nc2 .. -nc6
  B = 1, 3; B = 65535 (grid.y limit) with L = 1, D = VEC                 ...-B1, -B3, test_route_aggregate[*-B65535-*]
  one block / several blocks per sample in the forward                   L * D / VEC <= 1024 (-L1-D*) / > 1024 (-L129-D768 ...)
    (agg_chunks = cdiv(L * D / VEC, 1024); probs written by block 0)
  ld_probs, ld_dprobs > P * ncell                                        ...-ld+3 (every other case)
  d_probs given / NULL                                                   ...-dp / -nodp
  gates open / mixed / all closed                                        ...-open, -mixed, -closed
  S == float32(1e-4) (kept), the float below (skipped), 0                ...-thresh (P = ncell: one nonzero gate per output)
  g == float32(1e-4 / nc) (open), the float below (closed), 0            ...-thresh (P = 1; nc = 2, 3, 4, 6 via the nc cycle + extras)
  x0 == +0, -0, smallest positive subnormal (relu and its gradient)      every case (first elements of x0)
  workspace pre-filled with NaN                                          every case
  d_gates of the all-closed final layer, relative to its own size        ...-P1-*-closed
  refusals (D % VEC, D = 1028 / 1032 for P = ncell, D / VEC = 257 for    test_route_aggregate_refusals[*]
    P = 1, ncell = 1 / 7, P not in {1, ncell}, short workspace, no refs,
    misaligned pointer, B = 65536)
bert_embed_fwd: D = 4, 260, 768, 1024, 1028; ntok 1 .. 8193              test_bert_embed_fwd[*]
bert_embed_bwd
  ntok <= 8192 -> ids in LDS; ntok = 8193 -> ids in global memory        test_bert_embed_bwd[*-n8192-*] / [*-n8193-*]
  leader at a multiple of 64 (index 64), at index 8192                   ...-leader64-*, ...-n8193-distinct (token 8192 is its own leader)
  duplicates inside one 64-token chunk / across chunks                   ...-dupin-*, ...-dupacross-*
  one id for all tokens; all pad                                         ...-equal-*, ...-allpad-*
  type kernel: 8-deep loop (ntok >= 113), tail only (ntok < 113)         ...-n129|n8192|n8193-* / -n1|n63|n64|n65-*
  ntype = 1, 2, 3, one type absent                                       ...-ty1, -ty2, -ty3, -ty3absent
  rows of pad / unused ids / the absent type keep their bits             every case
  D = 1028 refused                                                       test_embed_refusals
meanpool_fwd: D < 16 * VEC (one partial column block), L < 16            test_meanpool_fwd[*-D4|D8|D60|D120-*], [*-L1|L15-*]
  nsrc = 1, 2, 6, 8; refusals nsrc = 0, 9, D % VEC                       test_meanpool_fwd[*-s1|s2|s6|s8], test_meanpool_refusals
meanpool_bwd: cdiv(B L D / VEC, 256) <= / > 2048 blocks                  test_meanpool_bwd[*-below|above-*]
meanpool_bwd_multi: <= / > 1024 blocks, n = 1, 3, 8, acc_mask 0 / all /  test_meanpool_bwd_multi[*]
  alternating; alias refusal                                             test_meanpool_refusals
patchify: p = 1, 16, 32; H != W; cdiv(total, 256) > 4096                 test_patchify[*]
clip_embed_finish / bwd: ntok = 1, 50; B = 1; > 4096 blocks; D % 256     test_clip_embed[*]
colsum: M = 0, 1, 32 (one slice, direct), 33 (two slices, rows_per 17),  test_colsum[*]
  8192 (256 slices), 8193 / 20000 (slice cap, empty trailing slices)
  vector path; scalar path by N % VEC, by pitch, by misaligned X         test_colsum[*-vec|-scalarN|-scalarld|-scalarX]
colsum_add: M = 0, 1, 32 bit-identical to sink + colsum; M >= 33 refused test_colsum[*-M0|M1|M32-*] / [*-M33 ...-*] (same test)
saf_dweights / saf_dscores: B * n around the 4 rows of a block,          test_saf_products[*]
  E = 8, 504, 512, 520, 768 (64 lanes x 8 = 512), B = 1, > 4096 blocks
lincomb: n = 1, 8; refusal at 0, 9                                       test_lincomb[*], test_lincomb_refusals

Every output is a `Guarded` tensor (test_gpu_kernel_edges): sentinel bits before, after and in any pitch gap, asserted unchanged; every
workspace starts as NaN; accumulating outputs start from known nonzero values; every call runs twice into fresh buffers and must give
identical bits (fixed-order reductions, no float atomics).

Checks without a tolerance (a cast, one fp32 operation, or adds in a stated order): d2r_patchify, d2r_bert_embed_fwd
((word + type) + pos), d2r_clip_embed_finish, d2r_meanpool_bwd / _bwd_multi with accumulate = 0 (g * (1.f / L)), d2r_colsum_add against
sink + d2r_colsum, the final layer's probs (a copy of the gates), and every untouched table row are compared bit for bit with the same
expression in torch fp32 rounded to the output type.  These also run with INDICATOR operands: one nonzero per tensor, a distinct power
of two at a position of its own, so an indexing error moves a whole element.

Checks with a bound, per element:

    |got - ref| <= C (u_out |ref| + n 2^-24 sum|terms|) + sub

u_out = 2^-9 (bf16), 2^-12 (fp16), 2^-24 (fp32): the unit roundoff of the output type; sum|terms| the fp64 sum of the absolute values of
what the kernel adds to form the element; n the longest sequential chain of fp32 operations in the kernel's documented order (given
next to each reference below); sub = 2^-25 for fp16 outputs (half the subnormal spacing), 2^-100 otherwise.  ref is fp64 on the exact
operand values; the skip / close decisions of route_aggregate are taken from the same fp32 comparisons as the kernel (the threshold
cases are built so that those fp32 sums are exact in any order).

C is kept per output and per output type (key "agg.out.bf16", ...).  C is not fitted to the kernels.  Each reference below is written once and evaluated in fp64 (the truth) and in fp32 in the kernel's
order with the final rounding to the output type (the rounding model); test_bound_constants_from_the_rounding_model (no GPU) evaluates
model error / bound over the whole case table, and C = 3 x the worst ratio per output (MODEL_WORST below, the table in
profiles/routing_embed_paths_ratios.md).  The factor 3 covers multiply-add contraction and the reduction-order freedom inside a chunk
or a wave that the model does not fix."""
import ctypes as C
import math
import os
import zlib

import numpy as np
import pytest
import torch

from test_gpu_kernel_edges import CODE, DT, DT_IDS, PAD, VEC, Guarded, _lib, _st, call

gpu_test = pytest.mark.gpu
F32, BF, FP16 = torch.float32, torch.bfloat16, torch.float16
LOWP = [BF, FP16]
UOUT = {F32: 2.0 ** -24, BF: 2.0 ** -9, FP16: 2.0 ** -12}
SUB = {F32: 2.0 ** -100, BF: 2.0 ** -100, FP16: 2.0 ** -25}
TH = np.float32(1e-4)
TH_BELOW = np.nextafter(TH, np.float32(0))
EPS = float(np.float32(1e-8))
AGG_LC = 8

# worst |model - ref| / (u_out |ref| + n 2^-24 sum|terms|) of the fp32 rounding model over the case tables (CPU); re-derived and compared
# by test_bound_constants_from_the_rounding_model; C = 3 x this figure
MODEL_WORST = {
    "agg.dbc.bf16": 1.991, "agg.dbc.fp16": 1.987, "agg.dbc.fp32": 0.119, "agg.demb.bf16": 1.992,
    "agg.demb.fp16": 1.993, "agg.demb.fp32": 0.261, "agg.dgates.fp32": 0.090, "agg.out.bf16": 1.992,
    "agg.out.fp16": 1.992, "agg.out.fp32": 0.290, "agg.probs.fp32": 0.321, "agg1.dbc.bf16": 1.991,
    "agg1.dbc.fp16": 1.985, "agg1.dbc.fp32": 0.162, "agg1.demb.bf16": 1.992, "agg1.demb.fp16": 1.991,
    "agg1.demb.fp32": 0.319, "agg1.dgates.fp32": 0.048, "agg1.out.bf16": 1.991, "agg1.out.fp16": 1.989,
    "agg1.out.fp32": 0.202, "bert.dpos.fp32": 0.561, "bert.dtype.fp32": 0.116, "bert.dword.fp32": 0.514,
    "clip.dpos.fp32": 0.410, "colsum.fp32": 0.074, "lincomb.fp32": 0.197, "pool.acc.bf16": 1.993,
    "pool.acc.fp16": 1.998, "pool.acc.fp32": 0.432, "pool.fwd.fp32": 0.170, "saf.ds.bf16": 1.993,
    "saf.ds.fp16": 1.997, "saf.dw.fp32": 0.082,
}
CBOUND = {k: 3.0 * v for k, v in MODEL_WORST.items()}
RATIO_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "routing_embed_paths_ratios.md")


def _seed(s):
    return zlib.crc32(s.encode()) & 0x7FFFFFFF


def _parr(ts):
    arr = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return arr


def seq(xs):
    """Sum in list order (the working precision is that of the tensors)."""
    t = xs[0]
    for x in xs[1:]:
        t = t + x
    return t


def chunk4(parts):
    """The finish kernels' sum over chunk partials: four interleaved accumulators, remainder into the first, (t0 + t1) + (t2 + t3)."""
    t = [torch.zeros_like(parts[0]) for _ in range(4)]
    k = 0
    while k + 3 < len(parts):
        for u in range(4):
            t[u] = t[u] + parts[k + u]
        k += 4
    while k < len(parts):
        t[0] = t[0] + parts[k]
        k += 1
    return (t[0] + t[1]) + (t[2] + t[3])


def ratio(got, ref, terms, n, out_dt):
    """max over elements of (|got - ref| - sub) / (u_out |ref| + n 2^-24 terms); 0 / 0 counts as 0, x / 0 as inf."""
    err = ((got.double() - ref).abs() - SUB[out_dt]).clamp_min(0.0)
    den = UOUT[out_dt] * ref.abs() + n * 2.0 ** -24 * terms
    r = torch.where(err > 0, err / den, torch.zeros_like(err))
    assert not torch.isnan(got.double()).any(), "NaN in an output (an element the kernel did not write, or scratch it read unwritten)"
    return float(r.max()) if r.numel() else 0.0


def check_bounded(tag, got, spec):
    """spec = (ref fp64, terms fp64, n, out dtype, key of the constant), or (ref, None, None, dtype, 'exact') for bit identity."""
    ref, terms, n, out_dt, key = spec
    got = got.detach().cpu()
    assert got.dtype == out_dt and tuple(got.shape) == tuple(ref.shape), f"{tag}: shape / dtype {got.shape} {got.dtype} vs {ref.shape}"
    if key == "exact":
        assert_bits(tag, got, ref.to(out_dt))
        return
    key = f"{key}.{DT_IDS[out_dt]}"
    r = ratio(got, ref, terms, n, out_dt)
    print(f"ratio {key:16s} {r:8.3f}  {tag}")  # (run with -s to collect the measured figures)
    assert r <= CBOUND[key], f"{tag}: error / bound = {r:.3f} > C = {CBOUND[key]:.3f} ({key})"


def _ibits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def assert_bits(tag, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{tag}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    bad = _ibits(got) != _ibits(want)
    # +0 / -0 of a sum are the same value; everything else must match bit for bit
    bad &= ~((got.double() == 0) & (want.double() == 0))
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{tag}: {n} element(s) differ in bits; first at flat index {i}: got {got.reshape(-1)[i].item()!r}, "
                             f"expected {want.reshape(-1)[i].item()!r}")


def run_twice(tag, fn):
    """fn() -> dict name -> Guarded.  Two runs into fresh buffers: identical bits, guards intact."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for k, G in a.items():
        G.intact(f"{tag}.{k}")
        b[k].intact(f"{tag}.{k} (second run)")
        assert torch.equal(G.buf.view(G.it), b[k].buf.view(G.it)), f"{tag}.{k}: two runs of the same call differ in bits"
    return a


def nan_ws(gpu, nbytes):
    """A guarded fp32 workspace of nbytes, every element NaN."""
    n = max(1, (nbytes + 3) // 4)
    return Guarded(gpu, F32, n, fill=torch.full((n,), float("nan")))


def untouched(tag, *gs):
    for G in gs:
        assert bool((G.buf.view(G.it) == G.sent).all()), f"{tag}: a refused call wrote to an output"


def refused(tag, name, *args):
    from d2r_amd._lib import D2RError
    try:
        call(name, *args)
    except D2RError:
        torch.cuda.synchronize()
        return
    pytest.fail(f"{tag}: {name} accepted arguments it must refuse")


def model_ratios(ref_fn, ops):
    """{key: worst ratio} of the fp32 rounding model of one case against the fp64 evaluation of the same reference."""
    truth, model = ref_fn(ops, torch.float64), ref_fn(ops, torch.float32)
    out = {}
    for name, (ref, terms, n, out_dt, key) in truth.items():
        if key == "exact":
            continue
        m = model[name][0].to(out_dt)
        key = f"{key}.{DT_IDS[out_dt]}"
        out[key] = max(out.get(key, 0.0), ratio(m, ref, terms, n, out_dt))
    return out


# ================================================================================================================================
# 1. d2r_route_aggregate_fwd / bwd
# ================================================================================================================================
def agg_case_id(c):
    return "%s-P%s-D%d-L%d-nc%d-B%d-%s-%s-ld+%d" % (DT_IDS[c["dt"]], "nc" if c["P"] != 1 else "1", c["D"], c["L"], c["nc"], c["B"],
                                                 c["regime"], "dp" if c["dp"] else "nodp", c["ldx"])


def _agg_cases():
    cases = []
    Ls = [1, 7, 8, 9, 19, 33, 65, 129]
    regimes = ["open", "mixed", "closed", "thresh"]
    for dt in DT:
        v = VEC[dt]
        for final in (False, True):
            Ds = [v, 64, 400, 768, 1000, 1024] + ([256 * v] if final and 256 * v > 1024 else [])
            n = 0
            for D in Ds:
                for L in Ls:
                    nc = 2 + (n % 5)
                    cases.append(dict(dt=dt, P=1 if final else nc, D=D, L=L, nc=nc, B=1 if (n // 5) % 2 else 3, regime=regimes[(n // 2) % 4],
                                      dp=n % 3 != 1, ldx=3 if n % 2 else 0))
                    n += 1
            # the threshold set for nc = 2, 3, 4, 6 and every regime for the smallest and the reference's own cell count
            for nc in (2, 3, 4, 6):
                cases.append(dict(dt=dt, P=1 if final else nc, D=64, L=9, nc=nc, B=7, regime="thresh", dp=True, ldx=1))
            for nc in (2, 6):
                for regime in regimes:
                    cases.append(dict(dt=dt, P=1 if final else nc, D=768, L=33, nc=nc, B=3, regime=regime, dp=regime != "mixed", ldx=2))
            cases.append(dict(dt=dt, P=1 if final else 2, D=v, L=1, nc=2, B=65535, regime="mixed", dp=True, ldx=0))
    seen, out = set(), []
    for c in cases:
        c["id"] = agg_case_id(c)
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


AGG_CASES = _agg_cases()


def agg_gates(c, g):
    B, nc, P = c["B"], c["nc"], c["P"]
    gates = 0.05 + 0.95 * torch.rand(B, nc, P, generator=g)
    if c["regime"] == "mixed":
        gates = gates * (torch.rand(B, nc, P, generator=g) > 0.5)
        if B > 1:
            gates[0] = 0.0  # one sample with every path closed
        if P != 1:
            gates[B - 1, :, 0] = 0.0  # one output of an otherwise mixed sample takes the skip
        else:
            gates[B - 1, 0, 0], gates[B - 1, 1, 0] = 0.0, 0.7  # one closed and one open path in the same sample
    elif c["regime"] == "closed":
        gates.zero_()
    elif c["regime"] == "thresh":
        gates.zero_()
        if P != 1:  # one nonzero gate per output: its fp32 sum is that gate whatever the order
            vals = [float(TH), float(TH_BELOW), 0.0, 0.5]
            for b in range(B):
                for i in range(P):
                    gates[b, (b + 2 * i) % nc, i] = vals[(b + i) % 4]
        else:
            thf = np.float32(1e-4 / nc)
            vals = [float(thf), float(np.nextafter(thf, np.float32(0))), 0.0, 0.5]
            for b in range(B):
                for j in range(nc):
                    gates[b, j, 0] = vals[(b + j) % 4]
    return gates.float().contiguous()


def agg_ops(c):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    dt, B, L, D, nc, P = c["dt"], c["B"], c["L"], c["D"], c["nc"], c["P"]
    r = lambda *s: torch.randn(*s, generator=g).to(dt)
    o = dict(c)
    o["embs"] = [r(B, D) if k in (1, 5) else r(B, L, D) for k in range(nc)]
    x0 = o["embs"][0].view(-1)
    tiny = {F32: 2.0 ** -149, BF: 2.0 ** -133, FP16: 2.0 ** -24}[dt]
    x0[0], x0[1], x0[2] = 0.0, -0.0, tiny
    assert float(x0[2]) == tiny and math.copysign(1.0, float(x0[1])) < 0
    o["gates"] = agg_gates(c, g)
    o["douts"] = [r(B, L, D) for _ in range(P)]
    o["ldp"] = P * nc + c["ldx"]                             # pitch of probs
    o["ldd"] = ldd = P * nc + (c["ldx"] + 2 if c["ldx"] else 0)  # pitch of d_probs: a different one, its gap holds NaN
    o["dprobs"] = torch.randn(B, ldd, generator=g) if c["dp"] else None
    if c["dp"]:
        o["dprobs"][:, P * nc:] = float("nan")
    if P == 1:
        o["refs"] = [r(B, L, D) for _ in range(nc)]
        o["out"] = agg_fwd(o, torch.float64)["out0"][0].view(B, L, D).to(dt)  # what the backward reads as the forward output
    return o


def _agg_coef(o, wd):
    """Per-sample coefficients, in the kernels' order.  P = ncell: c[b, i, j] = g_ji / (S_i + eps) + [j == 0][S_i < 1e-4], S_i summed
    over j = 0 .. 5 in order (fp32 decision).  P = 1: cg = g / (ss + sg), cs = [g < float(1e-4 / nc)] / (ss + sg)."""
    nc, G32 = o["nc"], o["gates"]
    G = G32.to(wd)
    if o["P"] != 1:
        S32 = seq([G32[:, j, :] for j in range(nc)])
        skip = (S32 < float(TH)).to(wd)
        S = seq([G[:, j, :] for j in range(nc)])
        inv_den = S + EPS
        ph = G.transpose(1, 2) / inv_den[:, :, None]  # [B, i, j]
        c = ph.clone()
        c[:, :, 0] += skip
        return dict(ph=ph, c=c, den=inv_den, G=G)
    thf = float(np.float32(1e-4 / nc))
    s = (G32[:, :, 0] < thf).to(wd)
    g1 = G[:, :, 0]
    sg, ss = seq([g1[:, j] for j in range(nc)]), seq([s[:, j] for j in range(nc)])
    inv = 1.0 / (ss + sg)
    return dict(cg=g1 * inv[:, None], cs=s * inv[:, None], inv=inv, g=g1)


def _agg_embs(o, wd):
    e = [x.to(wd) for x in o["embs"]]
    x0 = e[0]
    pos = o["embs"][0].double() > 0
    e[0] = torch.where(pos, x0, torch.zeros_like(x0))
    return [ek[:, None, :] if k in (1, 5) else ek for k, ek in enumerate(e)], x0, pos


def agg_fwd(o, wd):
    """out_i = sum_k c_ik emb_k, k in order (n = 14: 5 adds of S, + eps, divide, + skip, a product, 5 adds); probs = g / (S + eps) (n = 7).
    Final layer: out = cg_0 relu(x0) + cs_0 x0 + sum_k (cg_k emb_k + cs_k ref_k) (n = 21: 5 adds, ss + sg, reciprocal, g * inv, a
    product, 11 adds, the rounding of the skip coefficient); probs = the gates."""
    dt, B, L, D, nc, P = o["dt"], o["B"], o["L"], o["D"], o["nc"], o["P"]
    ex, x0, _ = _agg_embs(o, wd)
    k_ = _agg_coef(o, wd)
    want = wd == torch.float64
    res = {}
    if P != 1:
        c = k_["c"]
        for i in range(P):
            ci = lambda k: c[:, i, k, None, None]
            val = seq([ci(k) * ex[k] for k in range(nc)]).expand(B, L, D)
            terms = seq([ci(k).abs() * ex[k].abs() for k in range(nc)]).expand(B, L, D) if want else None
            res[f"out{i}"] = (val.reshape(B * L, D), None if terms is None else terms.reshape(B * L, D), 14, dt, "agg.out")
        ph = k_["ph"].reshape(B, nc * nc)
        res["probs"] = (ph, ph.abs(), 7, F32, "agg.probs")
        return res
    cg, cs = k_["cg"], k_["cs"]
    b3 = lambda t, k: t[:, k, None, None]
    refs = [x.to(wd) for x in o["refs"]]
    parts = [b3(cg, 0) * ex[0], b3(cs, 0) * x0]
    for k in range(1, nc):
        parts += [b3(cg, k) * ex[k], b3(cs, k) * refs[k]]
    val = seq(parts).expand(B, L, D)
    terms = seq([p.abs() for p in parts]).expand(B, L, D).reshape(B * L, D) if want else None
    res["out0"] = (val.reshape(B * L, D), terms, 21, dt, "agg1.out")
    res["probs"] = (o["gates"][:, :, 0].double(), None, None, F32, "exact")
    return res


def _chunk_rows(t, L):
    """[B, L, ...] -> list over chunks of [B, rows, ...]."""
    return [t[:, l0:min(L, l0 + AGG_LC)] for l0 in range(0, L, AGG_LC)]


def agg_bwd(o, wd):
    """Chains.  A dot product: <= 32 (P = 1: 64) products added per thread, 6 wave-shuffle levels, 4 waves, nchunk partials, the product
    itself.  d_gates adds the coefficient chain (8), the inner product with the probabilities (6 + 1), a subtraction, a product:
    n = nchunk + 59 (P = 1: nchunk + 86, with the d_probs add).  demb of a full cell: n = 14 (P = 1: 10).  demb of a broadcast cell:
    + 8 rows of a chunk + cdiv(nchunk, 4) + 3 over the chunks."""
    dt, B, L, D, nc, P = o["dt"], o["B"], o["L"], o["D"], o["nc"], o["P"]
    nchunk = -(-L // AGG_LC)
    ex, x0, pos = _agg_embs(o, wd)
    k_ = _agg_coef(o, wd)
    want = wd == torch.float64
    dv = [x.to(wd) for x in o["douts"]]
    res = {}
    z = lambda t: torch.zeros_like(t)

    def dot_chunks(a, b):  # [B, nchunk]: the per-block partials of <a, b>
        p = (a * b).expand(B, L, D).sum(-1)
        return torch.stack([ch.sum(-1) for ch in _chunk_rows(p, L)], 1)

    def over_rows(t):  # sum over the token rows: rows of a chunk in order, chunks by chunk4
        return chunk4([seq([ch[:, r] for r in range(ch.shape[1])]) for ch in _chunk_rows(t.expand(B, L, D), L)])

    if P != 1:
        c, G, den = k_["c"], k_["G"], k_["den"]
        dpr = None if o["dprobs"] is None else o["dprobs"][:, :nc * nc].reshape(B, nc, nc).to(wd)
        dph = torch.zeros(B, nc, nc, dtype=wd)
        aabs = torch.zeros(B, nc, nc, dtype=wd)
        for i in range(nc):
            for j in range(nc):
                parts = dot_chunks(dv[i], ex[j])
                dph[:, i, j] = seq(([dpr[:, i, j]] if dpr is not None else [z(parts[:, 0])]) + [parts[:, ch] for ch in range(nchunk)])
                if want:
                    aabs[:, i, j] = (dv[i].abs() * ex[j].abs()).expand(B, L, D).sum((1, 2)) + (dpr[:, i, j].abs() if dpr is not None else 0.0)
        inv = 1.0 / den
        q = G.transpose(1, 2) * inv[:, :, None]
        dotp = seq([dph[:, :, j] * q[:, :, j] for j in range(nc)])
        dg = ((dph - dotp[:, :, None]) * inv[:, :, None]).transpose(1, 2).reshape(B * nc * nc)
        tg = ((aabs + (aabs * q.abs()).sum(-1, keepdim=True)) * inv[:, :, None]).transpose(1, 2).reshape(B * nc * nc) if want else None
        res["d_gates"] = (dg, tg, nchunk + 59, F32, "agg.dgates")
        for k in range(nc):
            ck = lambda i: c[:, i, k, None, None]
            t = seq([ck(i) * dv[i] for i in range(nc)])
            ta = seq([ck(i).abs() * dv[i].abs() for i in range(nc)]) if want else None
            if k in (1, 5):
                res[f"demb{k}"] = (over_rows(t), ta.sum(1) if want else None, 14 + 8 + -(-nchunk // 4) + 3, dt, "agg.dbc")
            else:
                if k == 0:
                    t = torch.where(pos, t, z(t))
                    ta = torch.where(pos, ta, z(ta)) if want else None
                res[f"demb{k}"] = (t.reshape(B * L, D), ta.reshape(B * L, D) if want else None, 14, dt, "agg.demb")
        return res
    cg, cs, inv = k_["cg"], k_["cs"], k_["inv"]
    d0 = dv[0]
    outv = o["out"].to(wd)
    dots = [seq([p[:, ch] for ch in range(nchunk)]) for p in [dot_chunks(d0, ex[j]) for j in range(nc)] + [dot_chunks(d0, outv)]]
    dpr = None if o["dprobs"] is None else o["dprobs"][:, :nc].to(wd)
    dg = torch.stack([(dots[j] - dots[nc]) * inv for j in range(nc)], 1)
    if dpr is not None:
        dg = dg + dpr
    tg = None
    if want:
        ab = [(d0.abs() * e.abs()).expand(B, L, D).sum((1, 2)) for e in list(ex) + [outv]]
        tg = torch.stack([(ab[j] + ab[nc]) * inv for j in range(nc)], 1) + (dpr.abs() if dpr is not None else 0.0)
        tg = tg.reshape(B * nc)
    res["d_gates"] = (dg.reshape(B * nc), tg, nchunk + 86, F32, "agg1.dgates")
    b3 = lambda t, k: t[:, k, None, None]
    rowsum, rowabs = over_rows(d0), (d0.abs().sum(1) if want else None)
    for k in range(nc):
        if k in (1, 5):
            res[f"demb{k}"] = (cg[:, k, None] * rowsum, cg[:, k, None].abs() * rowabs if want else None, 10 + 8 + -(-nchunk // 4) + 3, dt,
                               "agg1.dbc")
        else:
            t = b3(cg, k) * d0
            if k == 0:
                t = torch.where(pos, t, z(t))
            res[f"demb{k}"] = (t.reshape(B * L, D), t.abs().reshape(B * L, D) if want else None, 10, dt, "agg1.demb")
        t = b3(cs, k) * d0
        res[f"dref{k}"] = (t.reshape(B * L, D), t.abs().reshape(B * L, D) if want else None, 10, dt, "agg1.demb")
    return res


def agg_ref(o, wd):
    res = agg_fwd(o, wd)
    res.update(agg_bwd(o, wd))
    return res


def agg_gpu(gpu, o):
    dt, B, L, D, nc, P, ldp, ldd = o["dt"], o["B"], o["L"], o["D"], o["nc"], o["P"], o["ldp"], o["ldd"]
    code = CODE[dt]
    embs = [x.to(gpu) for x in o["embs"]]
    refs = [x.to(gpu) for x in o["refs"]] if P == 1 else None
    gates, douts = o["gates"].to(gpu), [x.to(gpu) for x in o["douts"]]
    dpr = None if o["dprobs"] is None else o["dprobs"].to(gpu)
    outv = o["out"].to(gpu) if P == 1 else None
    need = _lib().load().d2r_route_aggregate_bwd_workspace(B, L, D, P)

    def once():
        G = {f"out{i}": Guarded(gpu, dt, B * L, D) for i in range(P)}
        G["probs"] = Guarded(gpu, F32, B, P * nc, ld=ldp)
        call("d2r_route_aggregate_fwd", code, _parr(embs), None if refs is None else _parr(refs), gates.data_ptr(), B, L, D, nc, P,
             _parr([G[f"out{i}"].t for i in range(P)]), G["probs"].ptr, ldp, _st())
        for k in range(nc):
            G[f"demb{k}"] = Guarded(gpu, dt, B, D) if k in (1, 5) else Guarded(gpu, dt, B * L, D)
            if P == 1:
                G[f"dref{k}"] = Guarded(gpu, dt, B * L, D)
        G["d_gates"] = Guarded(gpu, F32, B * nc * P)
        G["ws"] = nan_ws(gpu, need)
        call("d2r_route_aggregate_bwd", code, _parr(embs), None if refs is None else _parr(refs), gates.data_ptr(), _parr(douts),
             None if P != 1 else _parr([outv]), None if dpr is None else dpr.data_ptr(), ldd, B, L, D, nc, P,
             _parr([G[f"demb{k}"].t for k in range(nc)]), None if P != 1 else _parr([G[f"dref{k}"].t for k in range(nc)]),
             G["d_gates"].ptr, G["ws"].ptr, need, _st())
        return G
    return once


@gpu_test
@pytest.mark.parametrize("case", AGG_CASES, ids=[c["id"] for c in AGG_CASES])
def test_route_aggregate(gpu, case):
    o = agg_ops(case)
    G = run_twice(case["id"], agg_gpu(gpu, o))
    for name, spec in agg_ref(o, torch.float64).items():
        check_bounded(f"route_aggregate[{case['id']}].{name}", G[name].t, spec)


AGG_REFUSALS = ["D%VEC", "D-over-P=nc", "D/VEC=257-P=1", "ncell=1", "ncell=7", "P=2-of-4", "short-workspace", "no-refs", "misaligned",
                "B=65536"]


@gpu_test
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
@pytest.mark.parametrize("what", AGG_REFUSALS)
def test_route_aggregate_refusals(gpu, dtype, what):
    """Every refusal returns an error before any launch: all guarded outputs keep their sentinel bits."""
    v = VEC[dtype]
    nc, P, B, L, D, fwd = 4, 4, 2, 3, 64, True
    if what == "D%VEC":
        D = 64 + v // 2
    elif what == "D-over-P=nc":  # npk6 = D / 4 > 256 (16-bit: 1032 is a multiple of 8; fp32: 1028 also trips D / VEC <= 256)
        D, fwd = (1028 if dtype == F32 else 1032), False
    elif what == "D/VEC=257-P=1":
        D, P, fwd = 257 * v, 1, False
    elif what == "ncell=1":
        nc = P = 1
    elif what == "ncell=7":
        nc = P = 7
    elif what == "P=2-of-4":
        P = 2
    elif what == "no-refs":
        P = 1
    elif what == "B=65536":
        B, L, D = 65536, 1, v
    ne = max(nc, 6)
    big = torch.zeros(B * L * D + 64, dtype=dtype, device=gpu)
    src = big[:B * L * D]
    embs = [src] * ne
    refs = None if what == "no-refs" else [src] * ne
    gates = torch.full((B * ne * ne,), 0.5, device=gpu)
    outs = [Guarded(gpu, dtype, B * L, D) for _ in range(max(P, 1))]
    probs = Guarded(gpu, F32, B, ne * ne)
    dembs = [Guarded(gpu, dtype, B * L, D) for _ in range(ne)]
    drefs = [Guarded(gpu, dtype, B * L, D) for _ in range(ne)]
    dg = Guarded(gpu, F32, B * ne * ne)
    need = _lib().load().d2r_route_aggregate_bwd_workspace(B, L, D, P)
    ws = nan_ws(gpu, need)
    ws_bytes = need - 4 if what == "short-workspace" else need
    mis = big[1:] if what == "misaligned" else None  # one element past a 16-byte boundary
    e_arg = _parr([mis] + embs[1:]) if mis is not None else _parr(embs)
    if fwd and what != "short-workspace":
        refused(what, "d2r_route_aggregate_fwd", CODE[dtype], e_arg, None if refs is None else _parr(refs), gates.data_ptr(), B, L, D, nc, P,
                _parr([g.t for g in outs]), probs.ptr, ne * ne, _st())
    refused(what, "d2r_route_aggregate_bwd", CODE[dtype], e_arg, None if refs is None else _parr(refs), gates.data_ptr(), _parr([src] * ne),
            _parr([src]), None, ne * ne, B, L, D, nc, P, _parr([g.t for g in dembs]), _parr([g.t for g in drefs]), dg.ptr, ws.ptr, ws_bytes,
            _st())
    untouched(what, *outs, probs, *dembs, *drefs, dg)
    ws.intact(what)
    assert bool(torch.isnan(ws.t).all()), f"{what}: a refused call wrote to the workspace"


# ================================================================================================================================
# 2. d2r_meanpool_fwd / bwd / bwd_multi
# ================================================================================================================================
def _pool_fwd_cases():
    out = []
    for dt in DT:
        v = VEC[dt]
        n = 0
        for D in (v, 16 * v - v, 16 * v, 768, 1032):
            for L in (1, 15, 16, 17, 200):
                out.append(dict(dt=dt, D=D, L=L, nsrc=(1, 2, 6, 8)[n % 4], B=(1, 3)[(n // 4) % 2]))
                n += 1
    for c in out:
        c["id"] = "%s-D%d-L%d-B%d-s%d" % (DT_IDS[c["dt"]], c["D"], c["L"], c["B"], c["nsrc"])
    return out


POOL_FWD_CASES = _pool_fwd_cases()


def pool_fwd_ops(c):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    return dict(c, srcs=[torch.randn(c["B"], c["L"], c["D"], generator=g).to(c["dt"]) for _ in range(c["nsrc"])])


def pool_fwd_ref(o, wd):
    """Thread (column pack, row group rg) adds rows rg, rg + 16, ... in order; the 16 partials are added in order; one division:
    n = cdiv(L, 16) + 16 + 1."""
    B, L, D = o["B"], o["L"], o["D"]
    vals, terms = [], []
    for s in o["srcs"]:
        x = s.to(wd)
        parts = [seq([x[:, l] for l in range(rg, L, 16)]) if rg < L else torch.zeros(B, D, dtype=wd) for rg in range(16)]
        vals.append(seq(parts) / float(L))
        terms.append(x.abs().sum(1) / L)
    return {"pooled": (torch.stack(vals).reshape(-1, D), torch.stack(terms).reshape(-1, D), -(-L // 16) + 17, F32, "pool.fwd")}


@gpu_test
@pytest.mark.parametrize("case", POOL_FWD_CASES, ids=[c["id"] for c in POOL_FWD_CASES])
def test_meanpool_fwd(gpu, case):
    o = pool_fwd_ops(case)
    srcs = [s.to(gpu) for s in o["srcs"]]

    def once():
        G = {"pooled": Guarded(gpu, F32, case["nsrc"] * case["B"], case["D"])}
        call("d2r_meanpool_fwd", CODE[case["dt"]], _parr(srcs), case["nsrc"], case["B"], case["L"], case["D"], G["pooled"].ptr, _st())
        return G
    G = run_twice(case["id"], once)
    check_bounded(f"meanpool_fwd[{case['id']}]", G["pooled"].t, pool_fwd_ref(o, torch.float64)["pooled"])


def _pool_bwd_cases():
    out = []
    for dt in DT:
        v = VEC[dt]
        # cdiv(B L D / VEC, 256) against the 2048-block cap: 524288 packs
        for tag, B, L, D in (("tiny", 1, 1, v), ("odd", 3, 17, 16 * v - v), ("below", 4, 1024, 128 * v), ("above", 4, 1025, 128 * v)):
            for acc in (0, 1):
                out.append(dict(dt=dt, B=B, L=L, D=D, acc=acc, id="%s-%s-B%d-L%d-D%d-acc%d" % (DT_IDS[dt], tag, B, L, D, acc)))
    return out


POOL_BWD_CASES = _pool_bwd_cases()


def pool_bwd_ops(c, n=1):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    return dict(c, g=torch.randn(n, c["B"], c["D"], generator=g), old=[torch.randn(c["B"], c["L"], c["D"], generator=g).to(c["dt"]) for _ in range(n)])


def pool_acc_ref(o, wd, j=0):
    """accumulate = 1: old + g * (1 / L): a reciprocal, a product, an add (n = 3)."""
    B, L, D = o["B"], o["L"], o["D"]
    invL = (torch.ones((), dtype=wd) / L)
    add = (o["g"][j].to(wd) * invL)[:, None, :].expand(B, L, D)
    old = o["old"][j].to(wd)
    return {"dx": ((old + add).reshape(B * L, D), (old.abs() + add.abs()).reshape(B * L, D), 3, o["dt"], "pool.acc")}


def pool_exact(o, j=0):
    """accumulate = 0: from_f(g * (1.f / L)): one fp32 product, bit-exact."""
    B, L, D = o["B"], o["L"], o["D"]
    invL = torch.ones((), dtype=F32) / torch.tensor(float(o["L"]), dtype=F32)
    return (o["g"][j] * invL).to(o["dt"])[:, None, :].expand(B, L, D).reshape(B * L, D)


def _indicator_g(o, n=1):
    """One nonzero per pooled gradient: 2^(j+1) at a (sample, column) of its own."""
    g = torch.zeros_like(o["g"])
    for j in range(n):
        g[j, (j + 1) % o["B"], (3 * j + 1) % o["D"]] = 2.0 ** (j + 1)
    return dict(o, g=g)


@gpu_test
@pytest.mark.parametrize("case", POOL_BWD_CASES, ids=[c["id"] for c in POOL_BWD_CASES])
def test_meanpool_bwd(gpu, case):
    B, L, D, dt = case["B"], case["L"], case["D"], case["dt"]
    base = pool_bwd_ops(case)
    for o in (base, _indicator_g(base)):
        gd = o["g"][0].to(gpu).contiguous()

        def once():
            G = {"dx": Guarded(gpu, dt, B * L, D, fill=o["old"][0] if case["acc"] else None)}
            call("d2r_meanpool_bwd", CODE[dt], gd.data_ptr(), B, L, D, G["dx"].ptr, case["acc"], _st())
            return G
        G = run_twice(case["id"], once)
        if case["acc"]:
            check_bounded(f"meanpool_bwd[{case['id']}]", G["dx"].t, pool_acc_ref(o, torch.float64)["dx"])
        else:
            assert_bits(f"meanpool_bwd[{case['id']}]", G["dx"].t, pool_exact(o))


def _pool_multi_cases():
    out = []
    for dt in LOWP:
        # 262144 packs per source against the 1024-block cap
        for tag, B, L, D in (("tiny", 1, 1, 8), ("below", 2, 1024, 1024), ("above", 2, 1025, 1024)):
            for n, mask in ((1, 0), (1, 1), (3, 0b101), (3, 0b111), (8, 0), (8, 0xFF), (8, 0xAA)):
                out.append(dict(dt=dt, B=B, L=L, D=D, n=n, mask=mask, id="%s-%s-B%d-L%d-D%d-n%d-mask%x" % (DT_IDS[dt], tag, B, L, D, n, mask)))
    return out


POOL_MULTI_CASES = _pool_multi_cases()


@gpu_test
@pytest.mark.parametrize("case", POOL_MULTI_CASES, ids=[c["id"] for c in POOL_MULTI_CASES])
def test_meanpool_bwd_multi(gpu, case):
    B, L, D, dt, n, mask = (case[k] for k in ("B", "L", "D", "dt", "n", "mask"))
    base = pool_bwd_ops(case, n)
    for o in (base, _indicator_g(base, n)):
        gd = o["g"].to(gpu).contiguous()

        def once():
            G = {f"dx{j}": Guarded(gpu, dt, B * L, D, fill=o["old"][j] if (mask >> j) & 1 else None) for j in range(n)}
            call("d2r_meanpool_bwd_multi", CODE[dt], gd.data_ptr(), n, B, L, D, _parr([G[f"dx{j}"].t for j in range(n)]), mask, _st())
            return G
        G = run_twice(case["id"], once)
        for j in range(n):
            tag = f"meanpool_bwd_multi[{case['id']}].dx{j}"
            if (mask >> j) & 1:
                check_bounded(tag, G[f"dx{j}"].t, pool_acc_ref(o, torch.float64, j)["dx"])
            else:
                assert_bits(tag, G[f"dx{j}"].t, pool_exact(o, j))


@gpu_test
def test_meanpool_refusals(gpu):
    B, L, D = 2, 5, 64
    x = torch.zeros(B, L, D, dtype=BF, device=gpu)
    pooled = Guarded(gpu, F32, 9 * B, D)
    for nsrc in (0, 9):
        refused("nsrc", "d2r_meanpool_fwd", CODE[BF], _parr([x] * 9), nsrc, B, L, D, pooled.ptr, _st())
    refused("D%VEC", "d2r_meanpool_fwd", CODE[BF], _parr([x]), 1, B, L, 60, pooled.ptr, _st())
    refused("D%VEC", "d2r_meanpool_fwd", CODE[F32], _parr([x]), 1, B, L, 62, pooled.ptr, _st())
    g = torch.zeros(2, B, D, device=gpu)
    dx = Guarded(gpu, BF, B * L, D)
    refused("alias", "d2r_meanpool_bwd_multi", CODE[BF], g.data_ptr(), 2, B, L, D, _parr([dx.t, dx.t]), 0, _st())
    refused("n=9", "d2r_meanpool_bwd_multi", CODE[BF], g.data_ptr(), 9, B, L, D, _parr([dx.t] * 9), 0, _st())
    refused("fp32", "d2r_meanpool_bwd_multi", CODE[F32], g.data_ptr(), 1, B, L, D, _parr([dx.t]), 0, _st())
    refused("D%VEC", "d2r_meanpool_bwd", CODE[BF], g.data_ptr(), B, L, 60, dx.ptr, 0, _st())
    untouched("meanpool refusals", pooled, dx)


# ================================================================================================================================
# 3. d2r_bert_embed_fwd / bwd
# ================================================================================================================================
NTOK = {1: (1, 1), 63: (3, 21), 64: (2, 32), 65: (5, 13), 129: (3, 43), 8192: (4, 2048), 8193: (3, 2731)}
PAD_ID = 0


def bert_ids(pattern, ntok, g):
    """ids and the vocabulary size; every id is inside the table.  Pad tokens (id 0) sit inside `distinct`, between the duplicates of
    `dupin` / `dupacross` / `leader64` (indices 12, 66, 4100: none of the indices the patterns set) and make up `allpad`; `equal` is one id
    for ALL tokens and has none."""
    ids = 1 + torch.randperm(ntok, generator=g)
    if pattern == "distinct":
        if ntok > 4:
            ids[ntok // 2] = PAD_ID
    elif pattern == "equal":
        ids[:] = 5
    elif pattern == "allpad":
        ids[:] = PAD_ID
    elif pattern == "dupin":       # duplicates inside one 64-token chunk (and inside the last, short one)
        for i in (3, 17, 60, 62):
            if i < ntok:
                ids[i] = ids[min(1, ntok - 1)]
        if ntok > 70:
            ids[ntok - 1] = ids[ntok - 3]
    elif pattern == "dupacross":   # duplicates that straddle 64-token scan chunks, first occurrence not chunk-aligned
        for i in (10, 63, 64, 70, 127, 128, ntok - 1):
            if 0 <= i < ntok:
                ids[i] = ids[min(10, ntok - 1)]
        if ntok > 8000:
            ids[5000:5200:7] = ids[4097]
            ids[8191] = ids[4097]
    elif pattern == "leader64":    # the first token carrying the id sits at index 64 (a multiple of the scan chunk); more follow
        if ntok > 64:
            for i in (65, 127, 128, ntok - 1):
                if i < ntok:
                    ids[i] = ids[64]
    if pattern in ("dupin", "dupacross", "leader64"):
        for i in (12, 66, 4100):
            if i < ntok - 3:
                ids[i] = PAD_ID
    return ids.long(), ntok + 8  # unused ids: ntok + 1 .. ntok + 7


def _bert_cases():
    fwd, bwd = [], []
    pats = ["distinct", "equal", "allpad", "dupin", "dupacross", "leader64"]
    types = [("ty1", 1, False), ("ty2", 2, False), ("ty3", 3, False), ("ty3absent", 3, True)]
    for dt in DT:
        n = 0
        for ntok in NTOK:
            for D in (4, 260, 768, 1024):
                if ntok >= 8192 and D not in (4, 768):
                    continue
                for pat in pats:
                    if pat in ("dupacross", "leader64") and ntok < 65:
                        continue
                    if ntok >= 8192 and D == 768 and pat not in ("distinct", "dupacross"):
                        continue
                    if ntok < 8192 and D in (260, 1024) and pat not in ("distinct", "dupin", "dupacross"):
                        continue
                    ty = types[n % 4]
                    n += 1
                    bwd.append(dict(dt=dt, ntok=ntok, D=D, pat=pat, ty=ty, id="%s-n%d-D%d-%s-%s" % (DT_IDS[dt], ntok, D, pat, ty[0])))
        for ntok in (1, 65, 8193):
            for D in (4, 260, 768, 1024, 1028):
                if ntok == 8193 and D not in (4, 1028):
                    continue
                fwd.append(dict(dt=dt, ntok=ntok, D=D, pat="dupacross" if ntok > 64 else "distinct", ty=types[2],
                                id="%s-n%d-D%d" % (DT_IDS[dt], ntok, D)))
    return fwd, bwd


BERT_FWD_CASES, BERT_BWD_CASES = _bert_cases()


def bert_ops(c):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    B, L = NTOK[c["ntok"]]
    ids, vocab = bert_ids(c["pat"], c["ntok"], g)
    _, ntype, absent = c["ty"]
    tt = torch.randint(0, ntype, (c["ntok"],), generator=g)
    if absent:
        tt[tt == 1] = 2
    elif c["ntok"] >= ntype:
        tt[:ntype] = torch.arange(ntype)
    D = c["D"]
    return dict(c, B=B, L=L, ids=ids, tt=tt.long(), vocab=vocab, ntype=ntype, dY=torch.randn(c["ntok"], D, generator=g).to(c["dt"]),
                word=torch.randn(vocab, D, generator=g), pos=torch.randn(L, D, generator=g), type=torch.randn(ntype, D, generator=g))


@gpu_test
@pytest.mark.parametrize("case", BERT_FWD_CASES, ids=[c["id"] for c in BERT_FWD_CASES])
def test_bert_embed_fwd(gpu, case):
    """out = from_f((word[id] + type[tt]) + pos[l]): two fp32 adds in a stated order, bit-exact.  Second pass: indicator tables."""
    o = bert_ops(case)
    B, L, D, dt, ntok = o["B"], o["L"], o["D"], o["dt"], o["ntok"]
    t0 = ntok // 2
    ind = dict(word=torch.zeros_like(o["word"]), pos=torch.zeros_like(o["pos"]), type=torch.zeros_like(o["type"]))
    ind["word"][int(o["ids"][t0]), 1 % D] = 2.0
    ind["pos"][L - 1, 2 % D] = 4.0
    ind["type"][int(o["tt"][t0]), D - 1] = 8.0
    ids_d, tt_d = o["ids"].to(gpu), o["tt"].to(gpu)
    for tabs in (o, ind):
        w, p, t = tabs["word"].to(gpu), tabs["pos"].to(gpu), tabs["type"].to(gpu)

        def once():
            G = {"out": Guarded(gpu, dt, ntok, D)}
            call("d2r_bert_embed_fwd", CODE[dt], ids_d.data_ptr(), tt_d.data_ptr(), w.data_ptr(), p.data_ptr(), t.data_ptr(), B, L, D, o["vocab"],
                 o["ntype"], G["out"].ptr, _st())
            return G
        G = run_twice(case["id"], once)
        l = torch.arange(ntok) % L
        want = ((tabs["word"][o["ids"]] + tabs["type"][o["tt"]]) + tabs["pos"][l]).to(dt)
        assert_bits(f"bert_embed_fwd[{case['id']}]", G["out"].t, want)


def bert_bwd_ref(o, wd):
    """dword[id] += the dY rows of the id's tokens added in token order (n = the row's own token count); dpos[l] += sum over b in order (n = B + 1);
    dtype[ty] += 16 per-wave partials (tokens w, w + 16, ... of the type in order) added in wave order (n = cdiv(ntok, 16) + 17)."""
    ntok, D, B, L, ntype, vocab = o["ntok"], o["D"], o["B"], o["L"], o["ntype"], o["vocab"]
    dy = o["dY"].to(wd)
    ids, tt = o["ids"], o["tt"]
    live = ids != PAD_ID
    want = wd == torch.float64
    acc = torch.zeros(vocab, D, dtype=wd)
    if want:
        acc.index_add_(0, ids[live], dy[live])
    else:
        cnt = torch.bincount(ids[live], minlength=vocab)
        single = live & (cnt[ids] == 1)
        acc[ids[single]] = dy[single]
        for t in (live & ~single).nonzero().reshape(-1).tolist():
            acc[int(ids[t])] += dy[t]
    aabs = torch.zeros(vocab, D, dtype=wd).index_add_(0, ids[live], dy[live].abs())
    pre_w, pre_p, pre_t = o["word"].to(wd), o["pos"].to(wd), o["type"].to(wd)
    count = torch.bincount(ids[live], minlength=vocab).clamp_min(1).double()[:, None]  # the chain of a row: one add per token of its id
    res = {"dword": (pre_w + acc, pre_w.abs() + aabs, count, F32, "bert.dword")}
    d3 = dy.view(B, L, D)
    res["dpos"] = (pre_p + seq([d3[b] for b in range(B)]), pre_p.abs() + d3.abs().sum(0), B + 1, F32, "bert.dpos")
    rows = -(-ntok // 16)
    pad = torch.zeros(rows * 16, D, dtype=wd)
    pad[:ntok] = dy
    ttp = torch.full((rows * 16,), -1, dtype=torch.long)
    ttp[:ntok] = tt
    vals = []
    for ty in range(ntype):
        m = (pad * (ttp == ty)[:, None].to(wd)).view(rows, 16, D)
        vals.append(seq([seq([m[r] for r in range(rows)])[w] for w in range(16)]) if not want else m.sum((0, 1)))
    tabs = torch.zeros(ntype, D, dtype=wd).index_add_(0, tt, dy.abs())
    res["dtype"] = (pre_t + torch.stack(vals), pre_t.abs() + tabs, rows + 17, F32, "bert.dtype")
    return res


@gpu_test
@pytest.mark.parametrize("case", BERT_BWD_CASES, ids=[c["id"] for c in BERT_BWD_CASES])
def test_bert_embed_bwd(gpu, case):
    o = bert_ops(case)
    B, L, D, dt, ntok = o["B"], o["L"], o["D"], o["dt"], o["ntok"]
    ids_d, tt_d, dy = o["ids"].to(gpu), o["tt"].to(gpu), o["dY"].to(gpu)

    def once():
        G = {"dword": Guarded(gpu, F32, o["vocab"], D, fill=o["word"]), "dpos": Guarded(gpu, F32, L, D, fill=o["pos"]),
             "dtype": Guarded(gpu, F32, o["ntype"], D, fill=o["type"])}
        call("d2r_bert_embed_bwd", CODE[dt], dy.data_ptr(), ids_d.data_ptr(), tt_d.data_ptr(), B, L, D, o["ntype"], PAD_ID, G["dword"].ptr,
             G["dpos"].ptr, G["dtype"].ptr, _st())
        return G
    G = run_twice(case["id"], once)
    for name, spec in bert_bwd_ref(o, torch.float64).items():
        check_bounded(f"bert_embed_bwd[{case['id']}].{name}", G[name].t, spec)
    used = torch.zeros(o["vocab"], dtype=torch.bool)
    used[o["ids"][o["ids"] != PAD_ID]] = True
    assert int((~used).sum()) >= 8  # pad and the seven ids past ntok at least
    assert_bits(f"bert_embed_bwd[{case['id']}]: rows of pad / unused ids", G["dword"].t.cpu()[~used], o["word"][~used])
    tused = torch.zeros(o["ntype"], dtype=torch.bool)
    tused[o["tt"]] = True
    assert_bits(f"bert_embed_bwd[{case['id']}]: rows of absent types", G["dtype"].t.cpu()[~tused], o["type"][~tused])


@gpu_test
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_embed_refusals(gpu, dtype):
    B, L = 2, 3
    ids, tt = torch.ones(B * L, dtype=torch.long, device=gpu), torch.zeros(B * L, dtype=torch.long, device=gpu)
    for D in (1028, 6, 0):
        dy = torch.zeros(B * L * 1028, dtype=dtype, device=gpu)
        G = [Guarded(gpu, F32, 4, 1028), Guarded(gpu, F32, L, 1028), Guarded(gpu, F32, 2, 1028)]
        refused(f"D={D}", "d2r_bert_embed_bwd", CODE[dtype], dy.data_ptr(), ids.data_ptr(), tt.data_ptr(), B, L, D, 2, PAD_ID, G[0].ptr, G[1].ptr,
                G[2].ptr, _st())
        untouched(f"bert_embed_bwd D={D}", *G)
    out = Guarded(gpu, dtype, B * L, 8)
    tab = torch.zeros(64, device=gpu)
    refused("D%4", "d2r_bert_embed_fwd", CODE[dtype], ids.data_ptr(), tt.data_ptr(), tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), B, L, 6, 4, 2,
            out.ptr, _st())
    refused("unaligned table", "d2r_bert_embed_fwd", CODE[dtype], ids.data_ptr(), tt.data_ptr(), tab[1:].data_ptr(), tab.data_ptr(), tab.data_ptr(),
            B, L, 8, 4, 2, out.ptr, _st())
    px = torch.zeros(3 * 8 * 8, device=gpu)
    refused("H%p", "d2r_patchify", CODE[dtype], px.data_ptr(), 1, 8, 8, 3, out.ptr, _st())
    untouched("embed refusals", out)


# ================================================================================================================================
# 4. d2r_patchify, d2r_clip_embed_finish / bwd
# ================================================================================================================================
PATCH_CASES = [("p1-8x12", 2, 8, 12, 1), ("p16-32x64", 2, 32, 64, 16), ("p32-64x64", 2, 64, 64, 32), ("p32-96x32", 1, 96, 32, 32),
               ("p16-above-cap-448x464", 2, 448, 464, 16), ("p1-above-cap-600x601", 1, 600, 601, 1)]


@gpu_test
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
@pytest.mark.parametrize("name,B,H,W,p", PATCH_CASES, ids=[c[0] for c in PATCH_CASES])
def test_patchify(gpu, dtype, name, B, H, W, p):
    """A permutation and a cast: bit-exact.  cdiv(B * 3 * H * W, 256) > 4096 -> grid-stride walk.  Second pass: one nonzero pixel."""
    g = torch.Generator().manual_seed(_seed(name))
    px = torch.randn(B, 3, H, W, generator=g)
    one = torch.zeros_like(px)
    one[B - 1, 1, H - 2 if H > 1 else 0, W // 2 + 1 if W > 2 else 0] = 2.0
    gh, gw, K = H // p, W // p, 3 * p * p
    for src in (px, one):
        d = src.to(gpu)

        def once():
            G = {"patches": Guarded(gpu, dtype, B * gh * gw, K)}
            call("d2r_patchify", CODE[dtype], d.data_ptr(), B, H, W, p, G["patches"].ptr, _st())
            return G
        G = run_twice(name, once)
        want = src.view(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, K).to(dtype)
        assert_bits(f"patchify[{name}]", G["patches"].t, want)


CLIP_CASES = [("n1-B1-D768", 1, 1, 768), ("n1-B3-D260", 3, 1, 260), ("n50-B1-D768", 1, 50, 768), ("n50-B4-D100", 4, 50, 100),
              ("n5-B2-D1", 2, 5, 1), ("n50-B30-D768-above-cap", 30, 50, 768), ("n197-B7-D1000-above-cap", 7, 197, 1000)]


def clip_ops(name, B, ntok, D, dt):
    g = torch.Generator().manual_seed(_seed(name))
    return dict(B=B, ntok=ntok, D=D, dt=dt, dX=torch.randn(B, ntok, D, generator=g).to(dt))


def clip_bwd_ref(o, wd):
    """dpos[t] = sum over b in order (n = B)."""
    x = o["dX"].to(wd)
    return {"dpos": (seq([x[b] for b in range(o["B"])]), x.abs().sum(0), o["B"], F32, "clip.dpos")}


@gpu_test
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
@pytest.mark.parametrize("name,B,ntok,D", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_clip_embed(gpu, dtype, name, B, ntok, D):
    """finish: x[b, t] = from_f((t == 0 ? cls : x[b, t]) + pos[t]) in place, bit-exact (random and indicator operands); bwd: dpos bounded,
    dcls == dpos[0] bit for bit."""
    g = torch.Generator().manual_seed(_seed(name) + 1)
    x, cls, pos = torch.randn(B, ntok, D, generator=g).to(dtype), torch.randn(D, generator=g), torch.randn(ntok, D, generator=g)
    xi, ci, pi = torch.zeros_like(x), torch.zeros_like(cls), torch.zeros_like(pos)
    xi[B - 1, ntok - 1, D // 2], ci[D - 1], pi[ntok // 2, D // 3] = 2.0, 4.0, 8.0
    xi[0, 0, 0] = 16.0  # the class-token slot of the input is not read
    for xs, cs, ps in ((x, cls, pos), (xi, ci, pi)):
        cd, pd = cs.to(gpu), ps.to(gpu)

        def once():
            G = {"x": Guarded(gpu, dtype, B * ntok, D, fill=xs)}
            call("d2r_clip_embed_finish", CODE[dtype], G["x"].ptr, cd.data_ptr(), pd.data_ptr(), B, ntok, D, _st())
            return G
        G = run_twice(name, once)
        base = xs.float().clone()
        base[:, 0] = cs
        assert_bits(f"clip_embed_finish[{name}]", G["x"].t, (base + ps).to(dtype).reshape(B * ntok, D))
    o = clip_ops(name, B, ntok, D, dtype)
    dX = o["dX"].to(gpu)

    def once_b():
        G = {"dcls": Guarded(gpu, F32, D), "dpos": Guarded(gpu, F32, ntok, D)}
        call("d2r_clip_embed_bwd", CODE[dtype], dX.data_ptr(), B, ntok, D, G["dcls"].ptr, G["dpos"].ptr, _st())
        return G
    G = run_twice(name, once_b)
    check_bounded(f"clip_embed_bwd[{name}].dpos", G["dpos"].t, clip_bwd_ref(o, torch.float64)["dpos"])
    assert_bits(f"clip_embed_bwd[{name}].dcls", G["dcls"].t, G["dpos"].t[0])


# ================================================================================================================================
# 5. d2r_colsum / d2r_colsum_add
# ================================================================================================================================
def _slices(M):
    return min(256, max(1, -(-M // 32)))


def _colsum_cases():
    out = []
    for dt in DT:
        v = VEC[dt]
        for M in (0, 1, 32, 33, 8192, 8193, 20000):
            # path: vec (aligned, pitch a multiple of 16 bytes, N % VEC == 0); scalar by N, by pitch, by a misaligned X
            for path, N, ldx, shift in (("vec", 9 * v, 0, 0), ("vecld", 64 * v + v, 2 * v, 0), ("scalarN", 9 * v + 1, v - 1, 0),
                                        ("scalarld", 9 * v, 1, 0), ("scalarX", 9 * v, 0, 1)):
                if M > 8192 and path == "vecld":
                    continue
                out.append(dict(dt=dt, M=M, N=N, ld=N + ldx, shift=shift, path=path, id="%s-M%d-N%d-%s" % (DT_IDS[dt], M, N, path)))
    return out


COLSUM_CASES = _colsum_cases()


def colsum_ops(c):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    return dict(c, X=torch.randn(c["M"], c["N"], generator=g).to(c["dt"]), sink=torch.randn(c["N"], generator=g))


def colsum_ref(o, wd):
    """Vector kernel: S = min(256, cdiv(M, 32)) slices of rows_per = cdiv(M, S) rows; row group rg of 4 adds rows r0 + rg, r0 + rg + 4, ...
    in order, then sh0 + sh1 + sh2 + sh3; sum_partials: part group grp of 4 walks partials grp, grp + 4, ... in four accumulators
    ((a0 + a1) + (a2 + a3)), then (s0 + s1) + (s2 + s3).  Scalar kernel: slice y adds rows y, y + S, ... in order.
    n = cdiv(rows_per, 4) + 4 + S (vector), cdiv(M, S) + S (scalar); S = 1 goes straight to the output."""
    M, N, vec = o["M"], o["N"], o["path"].startswith("vec")
    x = o["X"].to(wd)
    S = _slices(M)
    zero = torch.zeros(N, dtype=wd)
    parts = []
    if vec:
        rp = -(-M // S)
        for y in range(S):
            r0, r1 = y * rp, min(M, y * rp + rp)
            sh = [seq([zero] + [x[m] for m in range(r0 + rg, r1, 4)]) for rg in range(4)]
            parts.append(((sh[0] + sh[1]) + sh[2]) + sh[3])
        n = -(-rp // 4) + 4 + S
    else:
        parts = [seq([zero] + [x[m] for m in range(y, M, S)]) for y in range(S)]
        n = -(-M // S) + S
    if S == 1:
        val = parts[0]
    else:
        sh = []
        for grp in range(4):
            a = [zero, zero, zero, zero]
            p = grp
            while p + 12 < S:
                a = [a[u] + parts[p + 4 * u] for u in range(4)]
                p += 16
            while p < S:
                a[0] = a[0] + parts[p]
                p += 4
            sh.append((a[0] + a[1]) + (a[2] + a[3]))
        val = (sh[0] + sh[1]) + (sh[2] + sh[3])
    return {"out": (val, x.abs().sum(0), n, F32, "colsum")}


@gpu_test
@pytest.mark.parametrize("case", COLSUM_CASES, ids=[c["id"] for c in COLSUM_CASES])
def test_colsum(gpu, case):
    o = colsum_ops(case)
    dt, M, N = o["dt"], o["M"], o["N"]
    X = Guarded(gpu, dt, M, N, ld=o["ld"], shift=o["shift"], fill=o["X"])  # the pitch gap of the input holds the sentinel too
    need = _lib().load().d2r_colsum_workspace(M, N)
    assert need == _slices(M) * N * 4
    xptr = X.buf[PAD + o["shift"]:].data_ptr()  # (an empty tensor has no data pointer: M = 0 still passes a valid address)

    def once():
        G = {"out": Guarded(gpu, F32, N), "ws": nan_ws(gpu, need)}
        call("d2r_colsum", CODE[dt], xptr, o["ld"], M, N, G["out"].ptr, G["ws"].ptr, need, _st())
        return G
    G = run_twice(case["id"], once)
    check_bounded(f"colsum[{case['id']}]", G["out"].t, colsum_ref(o, torch.float64)["out"])
    if M == 0:
        assert_bits(f"colsum[{case['id']}]: no rows", G["out"].t, torch.zeros(N))
    if M <= 32:
        assert bool(torch.isnan(G["ws"].t).all()), "one slice goes straight to the output: the workspace is not written"

        def once_add():
            A = {"sink": Guarded(gpu, F32, N, fill=o["sink"]), "ws": nan_ws(gpu, need)}
            call("d2r_colsum_add", CODE[dt], xptr, o["ld"], M, N, A["sink"].ptr, A["ws"].ptr, need, _st())
            return A
        A = run_twice(case["id"] + " colsum_add", once_add)
        assert_bits(f"colsum_add[{case['id']}] == sink + colsum", A["sink"].t, o["sink"] + G["out"].t.cpu())
    else:
        sink = Guarded(gpu, F32, N)
        refused("M > 32", "d2r_colsum_add", CODE[dt], xptr, o["ld"], M, N, sink.ptr, G["ws"].ptr, need, _st())
        untouched("colsum_add M > 32", sink)
    out = Guarded(gpu, F32, N)
    refused("short workspace", "d2r_colsum", CODE[dt], xptr, o["ld"], M, N, out.ptr, G["ws"].ptr, need - 4, _st())
    refused("ld < N", "d2r_colsum", CODE[dt], xptr, N - 1, M, N, out.ptr, G["ws"].ptr, need, _st())
    untouched("colsum refusals", out)


# ================================================================================================================================
# 6. d2r_saf_dweights, d2r_saf_dscores, d2r_lincomb
# ================================================================================================================================
def _saf_cases():
    out = []
    for dt in LOWP:
        for B, n in ((1, 1), (1, 3), (1, 4), (1, 5), (3, 21), (2, 64), (2, 65)):
            for E in (8, 504, 512, 520, 768):
                if (B, n) in ((1, 4), (2, 64)) and E not in (8, 768):
                    continue
                out.append(dict(dt=dt, B=B, n=n, E=E, id="%s-B%d-n%d-E%d" % (DT_IDS[dt], B, n, E)))
        out.append(dict(dt=dt, B=64, n=197, E=768, id="%s-B64-n197-E768-above-cap" % DT_IDS[dt]))  # B n E / 8 > 4096 * 256
    return out


SAF_CASES = _saf_cases()


def saf_ops(c):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    B, n, E, dt = c["B"], c["n"], c["E"], c["dt"]
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(c, dwsum=r(B, E).to(dt), S=r(B, n, E).to(dt), w=torch.rand(B, n, generator=g).to(dt), da=r(B, n), w_saf=r(E).to(dt))


def saf_ref(o, wd):
    """dw[b, i] = <dwsum[b], S[b, i]>: lane l adds packs l, l + 64, ... (8 products each) in order, 6 shuffle levels:
    n = 8 cdiv(E, 512) + 6 + 1.  dS = w dwsum + da w_saf: two products and an add (n = 3)."""
    B, n, E = o["B"], o["n"], o["E"]
    d, s = o["dwsum"].to(wd)[:, None, :], o["S"].to(wd)
    prod = (d * s).reshape(B * n, E)
    trips = -(-E // 512)
    padw = torch.zeros(B * n, trips * 512, dtype=wd)
    padw[:, :E] = prod
    lanes = padw.view(B * n, trips, 64, 8)
    acc = seq([lanes[:, t, :, j] for t in range(trips) for j in range(8)])  # [rows, 64]
    w = 64
    while w > 1:  # butterfly
        w //= 2
        acc = acc[:, :w] + acc[:, w:2 * w]
    res = {"dw": (acc[:, 0], prod.abs().sum(-1), 8 * trips + 7, F32, "saf.dw")}
    a, b = o["w"].to(wd)[:, :, None] * d, o["da"].to(wd)[:, :, None] * o["w_saf"].to(wd)
    res["dS"] = ((a + b).reshape(B * n, E), (a.abs() + b.abs()).reshape(B * n, E), 3, o["dt"], "saf.ds")
    return res


@gpu_test
@pytest.mark.parametrize("case", SAF_CASES, ids=[c["id"] for c in SAF_CASES])
def test_saf_products(gpu, case):
    o = saf_ops(case)
    B, n, E, dt = o["B"], o["n"], o["E"], o["dt"]
    d = {k: o[k].to(gpu) for k in ("dwsum", "S", "w", "da", "w_saf")}

    def once():
        G = {"dw": Guarded(gpu, F32, B * n), "dS": Guarded(gpu, dt, B * n, E)}
        call("d2r_saf_dweights", CODE[dt], d["dwsum"].data_ptr(), d["S"].data_ptr(), B, n, E, G["dw"].ptr, _st())
        call("d2r_saf_dscores", CODE[dt], d["w"].data_ptr(), d["dwsum"].data_ptr(), d["da"].data_ptr(), d["w_saf"].data_ptr(), B, n, E, G["dS"].ptr,
             _st())
        return G
    G = run_twice(case["id"], once)
    for name, spec in saf_ref(o, torch.float64).items():
        check_bounded(f"saf[{case['id']}].{name}", G[name].t, spec)


@gpu_test
def test_saf_refusals(gpu):
    x = torch.zeros(64, dtype=BF, device=gpu)
    f = torch.zeros(64, device=gpu)
    dw, dS = Guarded(gpu, F32, 8), Guarded(gpu, BF, 8, 8)
    refused("E%8", "d2r_saf_dweights", CODE[BF], x.data_ptr(), x.data_ptr(), 1, 2, 12, dw.ptr, _st())
    refused("fp32", "d2r_saf_dweights", CODE[F32], x.data_ptr(), x.data_ptr(), 1, 2, 8, dw.ptr, _st())
    refused("unaligned", "d2r_saf_dweights", CODE[BF], x[1:].data_ptr(), x.data_ptr(), 1, 2, 8, dw.ptr, _st())
    refused("E=0", "d2r_saf_dscores", CODE[BF], x.data_ptr(), x.data_ptr(), f.data_ptr(), x.data_ptr(), 1, 2, 0, dS.ptr, _st())
    refused("unaligned", "d2r_saf_dscores", CODE[BF], x.data_ptr(), x.data_ptr(), f.data_ptr(), x[1:].data_ptr(), 1, 2, 8, dS.ptr, _st())
    untouched("saf refusals", dw, dS)


LINCOMB_CASES = [dict(n=n, id="n%d" % n) for n in (1, 2, 8)]


def lincomb_ops(c):
    g = torch.Generator().manual_seed(_seed(c["id"]))
    return dict(c, x=torch.randn(c["n"], generator=g), coef=torch.randn(c["n"], generator=g))


def lincomb_ref(o, wd):
    """out = sum_k coef_k x_k from zero, in order: n products and n adds (n_chain = n + 1)."""
    p = o["coef"].to(wd) * o["x"].to(wd)
    return {"out": (seq([torch.zeros((), dtype=wd)] + [p[k] for k in range(o["n"])]).reshape(1), p.abs().sum().reshape(1), o["n"] + 1, F32,
                    "lincomb")}


@gpu_test
@pytest.mark.parametrize("case", LINCOMB_CASES, ids=[c["id"] for c in LINCOMB_CASES])
def test_lincomb(gpu, case):
    o = lincomb_ops(case)
    xs = [o["x"][k:k + 1].to(gpu) for k in range(o["n"])]
    coef = (C.c_float * o["n"])(*[float(v) for v in o["coef"]])

    def once():
        G = {"out": Guarded(gpu, F32, 1)}
        call("d2r_lincomb", _parr(xs), coef, o["n"], G["out"].ptr, _st())
        return G
    G = run_twice(case["id"], once)
    check_bounded(f"lincomb[{case['id']}]", G["out"].t, lincomb_ref(o, torch.float64)["out"])


@gpu_test
def test_lincomb_refusals(gpu):
    x = torch.ones(1, device=gpu)
    out = Guarded(gpu, F32, 1)
    coef = (C.c_float * 9)(*([1.0] * 9))
    for n in (0, 9):
        refused(f"n={n}", "d2r_lincomb", _parr([x] * 9), coef, n, out.ptr, _st())
    refused("null input", "d2r_lincomb", _parr([x, None]), coef, 2, out.ptr, _st())
    untouched("lincomb refusals", out)


# ================================================================================================================================
# 7. the constants of the bounds, from the rounding model (no GPU)
# ================================================================================================================================
def model_table():
    """{key: (worst ratio, case id)} of the fp32 rounding model over every bounded case table."""
    worst = {}

    def take(ref_fn, ops, cid):
        for k, r in model_ratios(ref_fn, ops).items():
            if r > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (r, cid)

    for c in AGG_CASES:
        take(agg_ref, agg_ops(c), c["id"])
    for c in POOL_FWD_CASES:
        take(pool_fwd_ref, pool_fwd_ops(c), c["id"])
    for c in POOL_BWD_CASES:
        if c["acc"]:
            take(pool_acc_ref, pool_bwd_ops(c), c["id"])
    for c in POOL_MULTI_CASES:
        o = pool_bwd_ops(c, c["n"])
        for j in range(c["n"]):
            if (c["mask"] >> j) & 1:
                take(lambda ops, wd, j=j: pool_acc_ref(ops, wd, j), o, c["id"])
    for c in BERT_BWD_CASES:
        take(bert_bwd_ref, bert_ops(c), c["id"])
    for dt in DT:
        for name, B, ntok, D in CLIP_CASES:
            take(clip_bwd_ref, clip_ops(name, B, ntok, D, dt), "%s-%s" % (DT_IDS[dt], name))
    for c in COLSUM_CASES:
        take(colsum_ref, colsum_ops(c), c["id"])
    for c in SAF_CASES:
        take(saf_ref, saf_ops(c), c["id"])
    for c in LINCOMB_CASES:
        take(lincomb_ref, lincomb_ops(c), c["id"])
    return worst


def test_bound_constants_from_the_rounding_model():
    """Re-derives MODEL_WORST on the CPU and checks it, and the file of record, against what the tests use."""
    worst = model_table()
    assert set(worst) == set(MODEL_WORST)
    text = open(RATIO_FILE).read()
    for k in sorted(worst):
        r, cid = worst[k]
        print(f"model worst ratio {k:12s} {r:.4f}  C = {3 * MODEL_WORST[k]:.3f}  ({cid})")
    for k in sorted(worst):
        r = worst[k][0]
        # the record is the re-derived figure rounded UP to three decimals
        assert r <= MODEL_WORST[k] <= r + 0.00101, f"{k}: recorded {MODEL_WORST[k]} vs re-derived {r:.4f}"
        assert f"| {k} | {MODEL_WORST[k]:.3f} | {3 * MODEL_WORST[k]:.3f} |" in text, f"{k}: {RATIO_FILE} does not record this constant"


def test_case_ids_are_unique():
    for table in (AGG_CASES, POOL_FWD_CASES, POOL_BWD_CASES, POOL_MULTI_CASES, BERT_FWD_CASES, BERT_BWD_CASES, COLSUM_CASES, SAF_CASES):
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)
