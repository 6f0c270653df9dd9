"""PatchDropout (--patch_dropout) on the MI355X: the three *_keep kernels through the raw C ABI on both of their paths, clip_embed_keep
against clip_embed and against an fp64 restatement, the whole model against the oracle with the same kept rows, and the trainer.

Bounds are the ones the existing tests use for the counterparts: d2r_patchify / d2r_clip_embed_finish are bit-exact and
d2r_clip_embed_bwd is checked with the "clip.dpos" constant in test_gpu_routing_embed_paths; the fp32 embedding against fp64 with
test_gpu_kernels.check; the model with the figures of test_gpu_model.test_default_init_logits_vs_oracle (loss, logits) and
test_default_init_gradients_vs_oracle (parameter gradients)."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_kernel_edges import CODE, DT, DT_IDS, _SENT, Guarded, _st, call, f64, within_ulp  # noqa: F401  (the shared helpers)
from test_gpu_routing_embed_paths import assert_bits, check_bounded, refused, untouched

pytestmark = pytest.mark.gpu

F32 = torch.float32
IMAGES = [(96, 32), (64, 16), (56, 14)]  # (image size, patch): np = 9 and 16 on the 16-byte path, np = 16 element by element
IMAGE_IDS = ["96p32", "64p16", "56p14"]


def _bits(t):
    return t.contiguous().view(_SENT[t.dtype][0])


def _keep_sets(B, n, seed=0):
    """{K: int32 [B, K]} for K in {1, np // 2, np}, chosen on the CPU.  For B = 3 and K = np // 2: position 0 is kept by all three
    samples, position 1 + b by sample b alone, position np - 1 by none; the rest comes from a window of a shared pool."""
    sets = {1: torch.tensor([[(3 * b + 2) % n] for b in range(B)], dtype=torch.int32),
            n: torch.arange(n, dtype=torch.int32).repeat(B, 1)}
    K = n // 2
    if B == 3:
        pool = list(range(4, n - 1))
        rows = [sorted([0, 1 + b] + pool[b:b + K - 2]) for b in range(B)]
    else:
        g = torch.Generator().manual_seed(seed + n)
        rows = [sorted(torch.randperm(n, generator=g)[:K].tolist()) for _ in range(B)]
    sets[K] = torch.tensor(rows, dtype=torch.int32)
    for k, s in sets.items():
        assert tuple(s.shape) == (B, k) and bool((s[:, 1:] > s[:, :-1]).all()) and int(s.min()) >= 0 and int(s.max()) < n
    if B == 3:
        counts = torch.zeros(n, dtype=torch.long)
        for r in sets[K].tolist():
            counts[r] += 1
        assert 1 < K < n and bool((counts == 3).any()) and bool((counts == 1).any()) and bool((counts == 0).any()), \
            "precondition: a position kept by all samples, one kept by exactly one, one kept by none"
    return sets


def _kp(h_keep, gpu):
    return h_keep, h_keep.to(gpu)


# ================================================================================================================================
# 1. The three kernels through the raw ABI
# ================================================================================================================================
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("image", IMAGES, ids=IMAGE_IDS)
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_patchify_keep_is_a_bit_exact_gather(gpu, dtype, image, B):
    """patches[b*K + j] is patch keep[b, j] of sample b, rounded to the dtype: bit for bit the rows of a full unfold.  All-aligned
    operands (the 16-byte path for p = 32 and 16), pixels or patches one element off 16 bytes (element by element) and a second run
    give the same bits; guards intact; the pixels are not written; K = np with the identity equals d2r_patchify."""
    S, p = image
    gw = S // p
    n, Kd = gw * gw, 3 * p * p
    px = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(S + B))
    full = px.view(B, 3, gw, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, n, Kd).to(dtype)
    pxd = px.to(gpu)
    for K, h_keep in _keep_sets(B, n).items():
        h_keep, keep = _kp(h_keep, gpu)
        want = torch.stack([full[b, h_keep[b].long()] for b in range(B)]).reshape(B * K, Kd)
        runs = []
        for variant in ("aligned", "pixels+1", "patches+1", "again"):
            P = Guarded(gpu, F32, B * 3 * S * S, shift=int(variant == "pixels+1"), fill=pxd)
            O = Guarded(gpu, dtype, B * K, Kd, shift=int(variant == "patches+1"))
            call("d2r_patchify_keep", CODE[dtype], P.ptr, B, S, S, p, h_keep.data_ptr(), keep.data_ptr(), K, O.ptr, _st())
            torch.cuda.synchronize()
            P.intact(f"patchify_keep {variant}.pixels")
            O.intact(f"patchify_keep {variant}.patches")
            assert torch.equal(_bits(P.t), _bits(pxd.reshape(-1))), f"{variant}: the pixels were written"
            runs.append(O.t.clone())
        assert torch.equal(_bits(runs[0].cpu()), _bits(want)), f"K={K}: not the kept patches of a full unfold"
        for variant, r in zip(("pixels+1", "patches+1", "again"), runs[1:]):
            assert torch.equal(_bits(r), _bits(runs[0])), f"K={K}: {variant} differs from the aligned run"
        if K == n:
            O = Guarded(gpu, dtype, B * n, Kd)
            call("d2r_patchify", CODE[dtype], pxd.data_ptr(), B, S, S, p, O.ptr, _st())
            torch.cuda.synchronize()
            assert torch.equal(_bits(O.t), _bits(runs[0])), "K = np with the identity differs from d2r_patchify"


@pytest.mark.parametrize("D", [8, 768])
@pytest.mark.parametrize("n", [9, 16], ids=["np9", "np16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_clip_embed_finish_keep(gpu, dtype, B, n, D):
    """x[b, 0] = cls + pos[0], x[b, 1 + j] = x[b, 1 + j] + pos[1 + keep[b, j]]: one fp32 add rounded to the dtype, compared bit for bit
    with the same expression in torch (the bound of test_gpu_routing_embed_paths.test_clip_embed).  x, cls or pos one element off 16
    bytes and a second run give the same bits; guards intact; cls and pos are not written; the identity equals the existing entry."""
    g = torch.Generator().manual_seed(100 * n + D + B)
    cls, pos = torch.randn(D, generator=g), torch.randn(1 + n, D, generator=g)
    for K, h_keep in _keep_sets(B, n).items():
        h_keep, keep = _kp(h_keep, gpu)
        x = torch.randn(B, 1 + K, D, generator=g).to(dtype)
        x[:, 0] = 16.0  # the class-token slot of the input is not read
        rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + h_keep.long()], 1)
        base = x.float().clone()
        base[:, 0] = cls
        want = (base + pos[rows]).to(dtype).reshape(B * (1 + K), D)
        runs = []
        for variant in ("aligned", "x+1", "cls+1", "pos+1", "again"):
            X = Guarded(gpu, dtype, B * (1 + K), D, shift=int(variant == "x+1"), fill=x.to(gpu))
            Cg = Guarded(gpu, F32, D, shift=int(variant == "cls+1"), fill=cls.to(gpu))
            Pg = Guarded(gpu, F32, 1 + n, D, shift=int(variant == "pos+1"), fill=pos.to(gpu))
            call("d2r_clip_embed_finish_keep", CODE[dtype], X.ptr, Cg.ptr, Pg.ptr, h_keep.data_ptr(), keep.data_ptr(), B, K, n, D, _st())
            torch.cuda.synchronize()
            for G, nm in ((X, "x"), (Cg, "cls"), (Pg, "pos")):
                G.intact(f"finish_keep {variant}.{nm}")
            assert torch.equal(_bits(Cg.t.cpu()), _bits(cls)) and torch.equal(_bits(Pg.t.cpu()), _bits(pos)), f"{variant}: an input was written"
            runs.append(X.t.clone())
        assert_bits(f"clip_embed_finish_keep[K={K}]", runs[0], want)
        for variant, r in zip(("x+1", "cls+1", "pos+1", "again"), runs[1:]):
            assert torch.equal(_bits(r), _bits(runs[0])), f"K={K}: {variant} differs from the aligned run"
        if K == n:
            X = Guarded(gpu, dtype, B * (1 + n), D, fill=x.to(gpu))
            cd, pd = cls.to(gpu), pos.to(gpu)
            call("d2r_clip_embed_finish", CODE[dtype], X.ptr, cd.data_ptr(), pd.data_ptr(), B, 1 + n, D, _st())
            torch.cuda.synchronize()
            assert torch.equal(_bits(X.t), _bits(runs[0])), "K = np with the identity differs from d2r_clip_embed_finish"


@pytest.mark.parametrize("D", [8, 768])
@pytest.mark.parametrize("n", [9, 16], ids=["np9", "np16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_clip_embed_bwd_keep(gpu, dtype, B, n, D):
    """dpos[0] = sum_b dX[b, 0]; dpos[1 + q] = the sum over the samples that kept q, ascending b: against fp64 with the per-element
    bound of test_gpu_routing_embed_paths for d2r_clip_embed_bwd (n = B sequential fp32 adds, constant "clip.dpos").  Positions no
    sample kept are exact +0 although dpos started as NaN; dcls is dpos[0] bit for bit; dX is not written; dX, dpos or dcls one
    element off 16 bytes and a second run give the same bits; the identity equals the existing entry point."""
    g = torch.Generator().manual_seed(1000 * n + D + B)
    nan = torch.full((1 + n, D), float("nan"))
    for K, h_keep in _keep_sets(B, n).items():
        h_keep, keep = _kp(h_keep, gpu)
        dX = torch.randn(B, 1 + K, D, generator=g).to(dtype)
        x64 = dX.double()
        ref, terms = torch.zeros(1 + n, D, dtype=torch.float64), torch.zeros(1 + n, D, dtype=torch.float64)
        kept = torch.zeros(1 + n, dtype=torch.bool)
        for b in range(B):  # ascending b
            rows = [0] + [1 + q for q in h_keep[b].tolist()]
            for j, r in enumerate(rows):
                ref[r] = ref[r] + x64[b, j]
                terms[r] = terms[r] + x64[b, j].abs()
                kept[r] = True
        runs = []
        for variant in ("aligned", "dX+1", "dpos+1", "dcls+1", "again"):
            X = Guarded(gpu, dtype, B * (1 + K), D, shift=int(variant == "dX+1"), fill=dX.to(gpu))
            Pg = Guarded(gpu, F32, 1 + n, D, shift=int(variant == "dpos+1"), fill=nan.to(gpu))
            Cg = Guarded(gpu, F32, D, shift=int(variant == "dcls+1"))
            call("d2r_clip_embed_bwd_keep", CODE[dtype], X.ptr, h_keep.data_ptr(), keep.data_ptr(), B, K, n, D, Cg.ptr, Pg.ptr, _st())
            torch.cuda.synchronize()
            for G, nm in ((X, "dX"), (Pg, "dpos"), (Cg, "dcls")):
                G.intact(f"bwd_keep {variant}.{nm}")
            assert torch.equal(_bits(X.t.cpu()), _bits(dX.reshape(B * (1 + K), D))), f"{variant}: dX was written"
            assert torch.equal(_bits(Cg.t), _bits(Pg.t[0])), f"{variant}: dcls is not dpos[0] bit for bit"
            runs.append(Pg.t.clone())
        got = runs[0].cpu()
        check_bounded(f"clip_embed_bwd_keep[{DT_IDS[dtype]} B{B} np{n} D{D} K{K}].dpos", got, (ref, terms, B, F32, "clip.dpos"))
        assert bool((got[~kept].view(torch.int32) == 0).all()), f"K={K}: a position no sample kept is not +0"
        assert K == n or bool((~kept).any())
        for variant, r in zip(("dX+1", "dpos+1", "dcls+1", "again"), runs[1:]):
            assert torch.equal(_bits(r), _bits(runs[0])), f"K={K}: {variant} differs from the aligned run"
        if K == n:
            Pg, Cg, dXd = Guarded(gpu, F32, 1 + n, D), Guarded(gpu, F32, D), dX.to(gpu)
            call("d2r_clip_embed_bwd", CODE[dtype], dXd.data_ptr(), B, 1 + n, D, Cg.ptr, Pg.ptr, _st())
            torch.cuda.synchronize()
            assert torch.equal(_bits(Pg.t), _bits(runs[0])), "K = np with the identity differs from d2r_clip_embed_bwd"


BAD_KEEP = {"index == np": ([[0, 9], [0, 1]], 2), "negative index": ([[-1, 2], [0, 1]], 2), "repeated index": ([[0, 1], [2, 2]], 2),
            "descending pair": ([[0, 1], [3, 2]], 2), "K = 0": ([[0], [0]], 0), "K = np + 1": ([list(range(10))] * 2, 10)}


@pytest.mark.parametrize("what", list(BAD_KEEP))
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_bad_keep_sets_are_refused_before_any_launch(gpu, dtype, what):
    """np = 9 (96 / 32), B = 2: each of the three entry points refuses the set on its host copy; the outputs, pre-filled with the
    sentinel, are unchanged.  (The device copy holds a valid set: nothing would be out of range even if a kernel were launched.)"""
    rows, K = BAD_KEEP[what]
    B, n, D, S, p = 2, 9, 8, 96, 32
    h_keep = torch.tensor(rows, dtype=torch.int32)
    keep = torch.arange(max(K, 1), dtype=torch.int32).clamp_max(n - 1).repeat(B, 1).to(gpu)
    px = torch.zeros(B, 3, S, S, device=gpu)
    Kout = max(1, min(K, n))
    patches = Guarded(gpu, dtype, B * Kout, 3 * p * p)
    refused(what, "d2r_patchify_keep", CODE[dtype], px.data_ptr(), B, S, S, p, h_keep.data_ptr(), keep.data_ptr(), K, patches.ptr, _st())
    x = Guarded(gpu, dtype, B * (1 + Kout), D)
    tab = torch.zeros(1 + n, D, device=gpu)
    refused(what, "d2r_clip_embed_finish_keep", CODE[dtype], x.ptr, tab.data_ptr(), tab.data_ptr(), h_keep.data_ptr(), keep.data_ptr(), B, K, n,
            D, _st())
    dX = torch.zeros(B * (1 + Kout) * D, dtype=dtype, device=gpu)
    dcls, dpos = Guarded(gpu, F32, D), Guarded(gpu, F32, 1 + n, D)
    refused(what, "d2r_clip_embed_bwd_keep", CODE[dtype], dX.data_ptr(), h_keep.data_ptr(), keep.data_ptr(), B, K, n, D, dcls.ptr, dpos.ptr, _st())
    untouched(what, patches, x, dcls, dpos)
    from d2r_amd import _lib
    assert b"d2r_clip_embed_bwd_keep" in _lib.load().d2r_last_error()


# ================================================================================================================================
# 2. clip_embed_keep
# ================================================================================================================================
def _embed_operands(dtype, gpu, B=3, S=96, p=32, E=768):
    from test_gpu_kernels import rnd
    n = (S // p) ** 2
    px = rnd(B, 3, S, S)
    w = rnd(E, 3, p, p, scale=0.05).to(dtype).float()  # exactly representable in dtype: the 16-bit shadow is exact
    cls, pos = rnd(E, seed=3), rnd(1 + n, E, seed=4)
    return n, px, w, cls, pos


def _run_embed(fn, px, w, cls, pos, dtype, gpu, gy):
    from d2r_amd import functional as F
    ts = [t.to(gpu).requires_grad_(True) for t in (w, cls, pos)]
    y = fn(px.to(gpu), ts[0], F.cast(ts[0].detach(), dtype), ts[1], ts[2])
    y.backward(gy.to(gpu).to(y.dtype))
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for t in ts]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_clip_embed_keep_with_the_identity_is_clip_embed(gpu, dtype):
    """K = np and keep[b, j] = j: output, dW, dcls and dpos are bit-identical to clip_embed's."""
    from d2r_amd import functional as F
    B, p = 3, 32
    n, px, w, cls, pos = _embed_operands(dtype, gpu, B=B)
    h_keep = torch.arange(n, dtype=torch.int32).repeat(B, 1)
    keep = h_keep.to(gpu)
    gy = torch.randn(B, 1 + n, 768, generator=torch.Generator().manual_seed(8))
    a = _run_embed(lambda x, w, wc, c, pe: F.clip_embed(x, w, wc, c, pe, p), px, w, cls, pos, dtype, gpu, gy)
    b = _run_embed(lambda x, w, wc, c, pe: F.clip_embed_keep(x, w, wc, c, pe, p, h_keep, keep), px, w, cls, pos, dtype, gpu, gy)
    for name, u, v in zip(("y", "dW", "dcls", "dpos"), a, b):
        assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(_bits(u), _bits(v)), f"{name} differs from clip_embed"
        assert bool(torch.isfinite(u.float()).all()) and float(u.float().abs().max()) > 0


def test_clip_embed_keep_fp32_against_an_fp64_restatement(gpu):
    """A proper subset, fp32: oracle.vision_embed in fp64, then index_select of the kept rows per sample, with autograd for dW, dcls
    and dpos; the bound of the fp32 embedding test (test_gpu_kernels.check: 2e-5 of the largest reference magnitude)."""
    from oracle import d2r_oracle as O
    from d2r_amd import functional as F
    from test_gpu_kernels import check
    B, p = 3, 32
    n, px, w, cls, pos = _embed_operands(torch.float32, gpu, B=B)
    h_keep = _keep_sets(B, n)[n // 2]
    K = h_keep.shape[1]
    gy = torch.randn(B, 1 + K, 768, generator=torch.Generator().manual_seed(9))
    got = _run_embed(lambda x, w, wc, c, pe: F.clip_embed_keep(x, w, wc, c, pe, p, h_keep, h_keep.to(gpu)), px, w, cls, pos,
                     torch.float32, gpu, gy)
    assert tuple(got[0].shape) == (B, 1 + K, 768)
    pre = "model.vision_embeddings"
    sd = {pre + ".patch_embedding.weight": w.double().requires_grad_(True), pre + ".class_embedding": cls.double().requires_grad_(True),
          pre + ".position_embedding.weight": pos.double().requires_grad_(True)}
    full = O.vision_embed(sd, px.double(), O.OracleConfig(image_size=96, patch_size=p))
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + h_keep.long()], 1)
    ref = torch.stack([full[b].index_select(0, rows[b]) for b in range(B)])
    ref.backward(gy.double())
    want = [ref.detach()] + [sd[k].grad for k in (pre + ".patch_embedding.weight", pre + ".class_embedding", pre + ".position_embedding.weight")]
    for name, u, v in zip(("y", "dW", "dcls", "dpos"), got, want):
        print(f"clip_embed_keep fp32 {name}: max err {float((u.double().cpu() - v).abs().max()):.3e}, scale {float(v.abs().max()):.3e}")
        check(f"clip_embed_keep.{name}", u, v, torch.float32)
    unkept = torch.ones(1 + n, dtype=torch.bool)
    unkept[rows.flatten()] = False
    assert bool(unkept.any()) and bool((got[3][unkept.to(gpu)].view(torch.int32) == 0).all()), "dpos of a position no sample kept is not +0"


# ================================================================================================================================
# 3. The whole model against the oracle
# ================================================================================================================================
_ORACLE = {}


def _oracle_reference(P, seed):
    """The fp64 oracle run of the model test, computed once and shared by its dtypes (left unchanged): the construction-time init of
    test_gpu_model.test_default_init_gradients_vs_oracle (2 + 2 layers, 96 / 32, B = 4, L = 24), O.vision_embed patched for the run to
    gather the rows a twin of the model's sampler draws -> (B, K, the model on the CPU, batch, loss, logits, {name: gradient})."""
    if (P, seed) in _ORACLE:
        return _ORACLE[(P, seed)]
    from oracle import d2r_oracle as O
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.patch_dropout import PatchDropout
    torch.manual_seed(2023)
    layers, B, L = 2, 4, 24
    tc = TextConfig(num_hidden_layers=layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=layers, image_size=96, patch_size=32)
    base = M.UnimoModelF(default_args(DR_step=3), vc, tc)
    sd = {k: v.detach().clone() for k, v in base.state_dict().items()}
    cfg = O.OracleConfig(text_layers=layers, vision_layers=layers, image_size=96, patch_size=32, DR_step=3)
    batch = O.synthetic_batch(cfg, B, L, seed=6)
    ids, mask, tt, labels, images = batch
    h_keep = PatchDropout(P, 9, seed=seed, rank=0).draw(B)  # the twin of the model's sampler: the same first draw
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + h_keep.long()], 1)
    full_embed = O.vision_embed

    def kept_embed(sd_, px, cfg_):
        full = full_embed(sd_, px, cfg_)
        return torch.stack([full[b].index_select(0, rows[b]) for b in range(px.shape[0])])

    osd = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone())
           for k, v in sd.items()}
    O.vision_embed = kept_embed
    try:
        lo, logits_o, _ = O.forward(osd, cfg, ids, mask, tt, labels, images.double(), train=True)
        lo.backward()
    finally:
        O.vision_embed = full_embed
    ograd = {k: v.grad for k, v in osd.items() if v.is_floating_point() and v.grad is not None}
    _ORACLE[(P, seed)] = (B, h_keep.shape[1], base, batch, float(lo.detach()), logits_o.detach(), ograd)
    return _ORACLE[(P, seed)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_model_with_patch_dropout_against_the_oracle(gpu, dtype):
    """Train mode, dropout 0, 2 + 2 layers, 96 px images in 32 px patches (np = 9), B = 4, P = 0.5 (K = 4), DR_step 3: the oracle in
    fp64 with its vision_embed patched to gather the rows a twin sampler draws.  Loss and logits within
    test_gpu_model.test_default_init_logits_vs_oracle's bounds (fp32 1e-4, bf16 2e-3), the parameter gradients within
    test_default_init_gradients_vs_oracle's (fp32: global cosine >= 0.99999, p90 of the per-tensor rel-L2 <= 1e-3, every part's cosine
    >= 0.9999; bf16: cosine >= 0.93, median <= 0.30, p90 <= 0.60, the fp32-headed parts >= 0.99, every part >= 0.7).
    The sampler's seed is chosen on the oracle alone: every gradient passes Block's signed square root, whose derivative is unbounded
    at 0, so a draw that puts a pre-activation next to 0 is ill-conditioned in fp32 for ANY implementation.  The oracle's own fp32 run
    against its fp64 run, same statistic (p90 of the per-tensor rel-L2): all patches (the existing test's case) 3.0e-4; kept rows
    with sampler seed 0: 1.1e-4, 1: 7.1e-4, 2: 4.1e-4, 3: 6.2e-4, 77: 2.9e-3 (the oracle in fp32 misses the 1e-3 bound itself there;
    the HIP path measured 5.7e-3 on that draw, with loss and logits within 3e-8 / 1.4e-7).  Seed 0 is the well-conditioned draw.
    Measured on an MI355X with seed 0: fp32 loss / logits err 1.6e-7 / 9.7e-8, cosine 1.000000, p90 5.6e-5, worst part 1.00000; bf16
    loss / logits err 6.6e-5 / 4.4e-4, cosine 0.976, median 0.149, p90 0.326, worst part 0.940."""
    from d2r_amd.params import ParamStore
    P, SEED = 0.5, 0
    B, K, base, (ids, mask, tt, labels, images), lo, logits_o, ograd = _oracle_reference(P, SEED)
    model = copy.deepcopy(base)  # the oracle's weights
    model.to(gpu).set_compute_dtype(dtype).train()
    ParamStore(model, dtype)
    assert model.model.set_patch_dropout(P, seed=SEED, rank=0).K == K
    loss, logits = model(ids.to(gpu), mask.to(gpu), tt.to(gpu), labels.to(gpu), images.to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    assert tuple(model.last_aux["vision_encode_out"].shape) == (B, 1 + K, 768)
    e_loss = abs(float(loss) - lo)
    e_logit = float((logits.detach().double().cpu() - logits_o).abs().max())
    lim = {torch.float32: 1e-4, torch.bfloat16: 2e-3}[dtype]
    dot = nn_g = nn_r = 0.0
    rels, by_part = [], {}
    for name, p in model.named_parameters():
        ref = ograd.get(name)
        if ref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{name}: dead in the oracle, live here"
            continue
        got = p.grad.detach().double().cpu()
        assert torch.isfinite(got).all(), name
        rels.append((float((got - ref).norm()), float(ref.norm())))
        key = ".".join(name.split(".")[:3]) if name.startswith("model.") else name.split(".")[0]
        a = by_part.setdefault(key, [0.0, 0.0, 0.0])
        d_, g_, r_ = float((got * ref).sum()), float(got.pow(2).sum()), float(ref.pow(2).sum())
        a[0], a[1], a[2] = a[0] + d_, a[1] + g_, a[2] + r_
        dot, nn_g, nn_r = dot + d_, nn_g + g_, nn_r + r_
    cos = dot / (nn_g * nn_r) ** 0.5
    gmax = max(r for _, r in rels)
    rel = np.asarray([e / (r + 1e-3 * gmax) for e, r in rels])
    part_cos = {k: d_ / max((g_ * r_) ** 0.5, 1e-300) for k, (d_, g_, r_) in by_part.items()}
    print(f"[patch-dropout model {DT_IDS[dtype]}] loss err {e_loss:.2e} logits err {e_logit:.2e} (limit {lim:.0e})  global cosine {cos:.6f}  "
          f"per-tensor rel-L2: median {np.median(rel):.2e} p90 {np.quantile(rel, 0.9):.2e} max {rel.max():.2e} over {len(rel)} tensors; "
          f"worst part cosine {min(part_cos.values()):.5f} ({min(part_cos, key=part_cos.get)})")
    assert e_loss <= lim and e_logit <= lim, (e_loss, e_logit, lim)
    emb = "model.vision_embeddings"
    assert any(k.startswith(emb) for k in part_cos), "the vision embedding has no gradient"
    if dtype == torch.float32:
        assert cos >= 0.99999 and np.quantile(rel, 0.9) <= 1e-3, (cos, np.quantile(rel, 0.9))
        assert min(part_cos.values()) >= 0.9999, part_cos
    else:
        assert cos >= 0.93 and np.median(rel) <= 0.30 and np.quantile(rel, 0.9) <= 0.60, (cos, np.median(rel), np.quantile(rel, 0.9))
        for k in ("fc", "model.block_fusion.linear_out", "model.self_text.0", "model.self_vision.0", "model.text_cls_pool.dense",
                  "model.vision_cls_pool.dense"):
            assert part_cos[k] >= 0.99, (k, part_cos[k])
        assert min(part_cos.values()) >= 0.7, part_cos


# ================================================================================================================================
# 4. The trainer
# ================================================================================================================================
_TRAINER_BASE = {}


def _train_two_steps(gpu, dtype, name, patch_dropout, call_set=False, **extra):
    """Two training steps (one epoch of two batches of 4, BERT dropout on, 64 px images in 32 px patches: np = 4) of a model with 2
    encoder layers per tower -> (weights, step losses, the default generator's state afterwards, the log lines on PatchDropout, model)."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.train import MSDTrainer
    from test_gpu_dataset_cache import _logger
    torch.manual_seed(31)
    torch.cuda.manual_seed_all(31)
    tc = TextConfig(num_hidden_layers=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    vc = VisionConfig(num_hidden_layers=2, image_size=64, patch_size=32)
    mix = extra.pop("aug_mixup", 0.0)
    args = default_args(DR_step=3, compute_dtype=dtype, device=str(gpu), num_epochs=1, batch_size=4, warmup_ratio=0.0, save_path=None,
                        lr=1e-4, seed=31, patch_dropout=patch_dropout, **extra)
    if "model" not in _TRAINER_BASE:  # the seeded construction (242 M parameters) is done once; every run starts from a copy of it
        _TRAINER_BASE["model"] = M.UnimoModelF(args, vc, tc)
    model = copy.deepcopy(_TRAINER_BASE["model"])
    torch.manual_seed(31)  # every run enters the trainer with the same state of the default generator
    if call_set:
        model.model.set_patch_dropout(0.0, 31, 0)
    mixer = None
    if mix:
        from d2r_amd.mix import Mixer
        mixer = Mixer(64, mixup_alpha=mix, seed=31, rank=0)
    logger, catch = _logger(f"patch-dropout-trainer-{name}")
    train = make_loader(SyntheticMSDDataset(8, 16, 64, 3, seed=1, num_image_tokens=5), 4, True, 0, drop_last=True)
    tr = MSDTrainer(train_data=train, dev_data=None, test_data=None, model=model, args=args, logger=logger, writer=None, mixer=mixer)
    tr.train(None, None)
    torch.cuda.synchronize()
    assert tr.step == 2
    losses = [float(l.split("loss:")[1].split()[0]) for l in catch.lines if l.startswith("step ")]
    return tr.store.flat_w.clone(), losses, torch.get_rng_state(), [l for l in catch.lines if "PatchDropout" in l], model


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_trainer_with_patch_dropout(gpu, dtype):
    """P = 0.5 on np = 4 patches (K = 2).  One seed twice: bit-identical weights and losses.  Against P = 0: other weights, the same
    state of torch's default generator afterwards.  P = 0 is bit for bit a model on which set_patch_dropout(0, ...) was called by hand.
    The log line names K.  In eval mode the trained model's logits do not depend on the sampler.  With --drop_path 0.2, --aug_mixup
    0.8 and --max_grad_norm 1 on top, a step is finite and reproducible."""
    tag = DT_IDS[dtype]
    w1, l1, s1, a1, model = _train_two_steps(gpu, dtype, f"{tag}-a", 0.5)
    w2, l2, s2, a2, _ = _train_two_steps(gpu, dtype, f"{tag}-b", 0.5)
    w0, l0, s0, a0, model0 = _train_two_steps(gpu, dtype, f"{tag}-off", 0.0)
    w3, l3, s3, a3, _ = _train_two_steps(gpu, dtype, f"{tag}-set0", 0.0, call_set=True)
    assert len(l1) == 1 and np.isfinite(l1[0]) and bool(torch.isfinite(w1).all())
    assert torch.equal(w1, w2) and l1 == l2, "two runs with one seed differ"
    assert not torch.equal(w1, w0), "patch_dropout changed nothing"
    assert torch.equal(s1, s0), "PatchDropout moved torch's default generator"
    assert torch.equal(w0, w3) and l0 == l3 and torch.equal(s0, s3), "set_patch_dropout(0) changed the run"
    assert len(a1) == 1 and "K = 2" in a1[0] and "np = 4" in a1[0] and "P = 0.5" in a1[0] and "3 image tokens" in a1[0], a1
    assert not a0 and not a3
    assert model.model.vision_embeddings.patch_dropout.K == 2 and model0.model.vision_embeddings.patch_dropout is None
    # eval mode: the logits of the trained model with the sampler set, and cleared
    model.eval()
    gen = torch.Generator().manual_seed(9)
    ids = torch.randint(1000, 30000, (4, 16), generator=gen).to(gpu)
    images = torch.randn(4, 3, 64, 64, generator=gen).to(gpu)
    labels = torch.tensor([0, 1, 2, 1], device=gpu)
    with torch.no_grad():
        _, logits_set = model(ids, torch.ones_like(ids), torch.zeros_like(ids), labels, images)
        logits_set = logits_set.clone()
        assert tuple(model.last_aux["vision_encode_out"].shape) == (4, 5, 768), "eval mode dropped patches"
        model.model.set_patch_dropout(0.0)
        _, logits_cleared = model(ids, torch.ones_like(ids), torch.zeros_like(ids), labels, images)
    assert torch.equal(logits_set, logits_cleared) and bool(torch.isfinite(logits_set).all())
    # together with stochastic depth, MixUp and gradient clipping
    combo = dict(drop_path=0.2, aug_mixup=0.8, max_grad_norm=1.0)
    w4, l4, _, a4, _ = _train_two_steps(gpu, dtype, f"{tag}-combo-a", 0.5, **combo)
    w5, l5, _, _, _ = _train_two_steps(gpu, dtype, f"{tag}-combo-b", 0.5, **combo)
    assert len(l4) == 1 and np.isfinite(l4[0]) and bool(torch.isfinite(w4).all()) and len(a4) == 1
    assert torch.equal(w4, w5) and l4 == l5, "two runs with drop_path, MixUp and clipping differ"
    assert not torch.equal(w4, w1)


# ================================================================================================================================
# 5. The device cache
# ================================================================================================================================
@pytest.mark.parametrize("dtype,decode", [(torch.bfloat16, "device"), (torch.float32, "host")], ids=["bf16_device_decode", "fp32_host_decode"])
def test_cached_and_uncached_training_agree_with_patch_dropout(gpu, tmp_path, dtype, decode):
    """test_gpu_dataset_cache.test_training_with_the_cache_is_bit_identical_to_training_without with --patch_dropout 0.5 (np = 4,
    K = 2): the same seed gives the same losses, dev metrics and weights whether the batches come from the loaders or the cache."""
    from d2r_amd.cache import cache_loaders, release_workers
    from d2r_amd.train import MSDTrainer
    from test_gpu_dataset_cache import _loader, _logger, _small_model, _tokenizer, make_dir
    data, img, vocab = make_dir(tmp_path)
    tok = _tokenizer(vocab)
    results = []
    for use_cache in (False, True):
        torch.manual_seed(31)
        torch.cuda.manual_seed_all(31)
        model, args = _small_model(dtype, gpu)
        args.patch_dropout, args.seed = 0.5, 31
        logger, catch = _logger(f"patch-dropout-cache-{dtype}-{use_cache}")
        loaders = {"train": _loader(data, img, tok, "train", True, decode, S=64, workers=0),
                   "dev": _loader(data, img, tok, "dev", False, decode, S=64, workers=0)}  # no worker processes: they take a minute to start
        if use_cache:
            loaders = cache_loaders(loaders, str(gpu), logger)
        tr = MSDTrainer(train_data=loaders["train"], dev_data=loaders["dev"], test_data=None, model=model, args=args, logger=logger,
                        writer=None)
        tr.train(None, None)
        torch.cuda.synchronize()
        metrics = [l for l in catch.lines if l.startswith("  ") and " = " in l and not l.startswith("  Num") and "Batch size" not in l
                   and "Learning rate" not in l and "Evaluate begin" not in l and "PatchDropout" not in l]
        losses = [l.split("samples/s")[0] for l in catch.lines if l.startswith("step ")]
        results.append((tr.store.flat_w.clone(), metrics, losses, [l for l in catch.lines if "PatchDropout" in l]))
        if not use_cache:
            for dl in loaders.values():
                release_workers(dl)
    (w0, m0, l0, p0), (w1, m1, l1, p1) = results
    assert len(p0) == len(p1) == 1 and "K = 2" in p0[0]
    assert len(l0) == 2 and l0 == l1, (l0, l1)
    assert m0 == m1 and any("f_score" in l for l in m0), (m0, m1)
    assert torch.equal(w0, w1), "the cached run's weights differ in %d elements" % int((w0 != w1).sum())
