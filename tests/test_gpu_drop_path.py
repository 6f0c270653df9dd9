"""Stochastic depth (--drop_path) on the MI355X: d2r_drop_path through the raw C ABI against fp64 on every dispatch path, the two
encoder layers (one-call against op-by-op, exact properties of a dropped sample, fp32 against an fp64 restatement), and the trainer.
The mask reference is the numpy splitmix64 of test_gpu_kernel_edges._keep_ref: over sample indices for the path mask, over element
indices for the element mask."""
import numpy as np
import pytest
import torch

from test_gpu_kernel_edges import CODE, DT, DT_IDS, _SENT, Guarded, _keep_ref, _st, call, f64, within_ulp
from test_gpu_kernels import LOWP

pytestmark = pytest.mark.gpu

P_PATH = 0.5
SHAPES = [(1, 1003), (5, 1003), (7, 1000), (37, 8), (1003, 1), (9, 622216)]


def _pick_seed(pred, B=None, p=P_PATH, start=1):
    """The first seed >= start whose path mask (keep per sample, numpy bool [B]) satisfies `pred`: chosen on the CPU."""
    for seed in range(start, start + 100000):
        if pred(_keep_ref(B, p, seed).numpy() if B is not None else seed):
            return seed
    raise AssertionError("no seed found")


def _mixed(k):
    return bool(k.any()) and not bool(k.all())


# one seed that keeps and drops at least one sample of every multi-sample shape; for the single sample, one seed each way
SEED_PATH = _pick_seed(lambda s: all(_mixed(_keep_ref(B, P_PATH, s).numpy()) for B, _ in SHAPES if B > 1))
SEED_ONE_KEPT = _pick_seed(lambda k: bool(k[0]), B=1)
SEED_ONE_DROPPED = _pick_seed(lambda k: not bool(k[0]), B=1)
SEED_ELEM = 0x1234567890ABCDEF


def _bits(t, dtype):
    return t.contiguous().view(_SENT[dtype][0])


# ================================================================================================================================
# 1. The kernel against fp64
# ================================================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_drop_path_kernel_against_fp64_on_every_path(gpu, dtype, shape):
    """All-aligned operands (16-byte packs when per_sample is a multiple of the pack width), x / add / y one element off 16 bytes in
    turn (element by element) and in place (y == x) give the same bits; kept samples are add + x / ((1 - p_path)(1 - p_elem)) on the
    kept elements within one ulp (+ the fp32 rounding of the terms); a dropped sample is a bit copy of add (+0 without it) although
    its x holds inf and NaN; guard bands stay intact; a second run repeats the bits; p_path = 0 is d2r_dropout bit for bit."""
    B, n = shape
    N = B * n
    it = _SENT[dtype][0]
    g = torch.Generator().manual_seed(N)
    x = (1.0 + torch.rand(N, generator=g)).to(dtype)  # never 0: y != add <=> kept
    add = torch.randn(N, generator=g).to(dtype)
    for seed_path in ([SEED_PATH] if B > 1 else [SEED_ONE_KEPT, SEED_ONE_DROPPED]):
        keep_b = _keep_ref(B, P_PATH, seed_path)
        if B > 1:
            assert bool(keep_b.any()) and not bool(keep_b.all()), "precondition: a kept and a dropped sample"
        keep_rows = keep_b.repeat_interleave(n)
        xp, ap = x.clone(), add.clone()
        dropped = (~keep_b).nonzero().flatten().tolist()
        if dropped:  # poison the dropped branch, and plant a -0.0 in the skip connection that must come through as it is
            lo = dropped[0] * n
            xp[lo] = float("inf")
            xp[lo + n - 1] = float("nan")
            ap[lo + (n - 1) // 2] = -0.0
        x64, a64 = f64(x), f64(add)
        xd, ad = xp.to(gpu), ap.to(gpu)
        for p_elem in (0.0, 0.1):
            keep_i = _keep_ref(N, p_elem, SEED_ELEM)
            for with_add in (False, True):
                name = f"drop_path[{DT_IDS[dtype]} {B}x{n} seed={seed_path} p_elem={p_elem} add={with_add}]"
                runs = []
                for variant in ("aligned", "x+1", "add+1", "y+1", "in_place", "again"):
                    X = Guarded(gpu, dtype, N, shift=int(variant == "x+1"), fill=xd)
                    A = Guarded(gpu, dtype, N, shift=int(variant == "add+1"), fill=ad)
                    Y = X if variant == "in_place" else Guarded(gpu, dtype, N, shift=int(variant == "y+1"))
                    call("d2r_drop_path", CODE[dtype], X.ptr, A.ptr if with_add else None, Y.ptr, B, n, P_PATH, seed_path, p_elem,
                         SEED_ELEM, _st())
                    torch.cuda.synchronize()
                    for G, nm in ((X, "x"), (A, "add"), (Y, "y")):
                        G.intact(f"{name} {variant}.{nm}")
                    assert torch.equal(_bits(A.t, dtype), _bits(ad, dtype)), f"{name} {variant}: add was written"
                    if variant != "in_place":
                        assert torch.equal(_bits(X.t, dtype), _bits(xd, dtype)), f"{name} {variant}: x was written"
                    runs.append(Y.t.clone())
                for variant, r in zip(("x+1", "add+1", "y+1", "in_place", "again"), runs[1:]):
                    assert torch.equal(_bits(r, dtype), _bits(runs[0], dtype)), f"{name}: {variant} differs from the aligned run"
                got = runs[0].cpu()
                # dropped samples: a select
                want_bits = _bits(ap, dtype) if with_add else torch.zeros(N, dtype=it)
                assert torch.equal(_bits(got, dtype)[~keep_rows], want_bits[~keep_rows]), f"{name}: a dropped sample is not a copy of add"
                # kept samples: fp64
                ref = keep_i.double() / (1 - p_elem) * x64 / (1 - P_PATH) + (a64 if with_add else 0.0)
                mag = x64.abs() / ((1 - P_PATH) * (1 - p_elem)) + a64.abs()
                if bool(keep_rows.any()):
                    within_ulp(name, got[keep_rows], ref[keep_rows], mag[keep_rows], dtype)
                if not with_add:
                    assert torch.equal(got != 0, keep_rows & keep_i), f"{name}: kept elements differ from the counter-based generator"
    # p_path = 0: bit for bit d2r_dropout with the same (p_elem, seed_elem)
    for p_elem in (0.0, 0.1):
        for with_add in (False, True):
            outs = []
            for fn in ("d2r_drop_path", "d2r_dropout"):
                X, A, Y = Guarded(gpu, dtype, N, fill=x.to(gpu)), Guarded(gpu, dtype, N, fill=add.to(gpu)), Guarded(gpu, dtype, N)
                if fn == "d2r_drop_path":
                    call(fn, CODE[dtype], X.ptr, A.ptr if with_add else None, Y.ptr, B, n, 0.0, SEED_PATH, p_elem, SEED_ELEM, _st())
                else:
                    call(fn, CODE[dtype], X.ptr, A.ptr if with_add else None, Y.ptr, N, p_elem, SEED_ELEM, _st())
                torch.cuda.synchronize()
                Y.intact(f"{fn} p_path=0")
                outs.append(_bits(Y.t, dtype).cpu())
            assert torch.equal(outs[0], outs[1]), f"p_path = 0, p_elem = {p_elem}, add = {with_add}: differs from d2r_dropout"


# ================================================================================================================================
# 2. - 4. The encoder layers
# ================================================================================================================================
def _make_layer(kind, gpu, dtype, B=None):
    """(layer, B, L, is_bert): the shapes of test_gpu_kernels.test_encoder_layer_one_call_matches_op_by_op."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig
    torch.manual_seed(3)
    if kind.startswith("bert"):
        pd = 0.1 if kind == "bert-dropout" else 0.0
        layer = M.BertLayer(TextConfig(num_hidden_layers=1, hidden_dropout_prob=pd, attention_probs_dropout_prob=pd))
        return layer, B or 3, 37, True
    return M.CLIPEncoderLayer(VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)), B or 2, 50, False


def _prepare(layer, gpu, lowp):
    """The layer on the device in train mode with a ParamStore (the one-call path needs its 16-bit shadows and gradient sinks)."""
    from d2r_amd import modules as M
    from d2r_amd.params import ParamStore

    class Wrap(M.D2RModule):
        def __init__(self, layer):
            super().__init__()
            self.layer = layer

    model = Wrap(layer).to(gpu)
    model.set_compute_dtype(lowp).train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "LayerNorm" in n or "layer_norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    return model, ParamStore(model, lowp)


def _patch_seeds(monkeypatch, F, path_seeds):
    elem, path = iter(range(7000, 7100)), iter(path_seeds)
    monkeypatch.setattr(F, "_next_dropout_seed", lambda: next(elem))
    monkeypatch.setattr(F, "_next_drop_path_seed", lambda: next(path))


@pytest.mark.parametrize("lowp", LOWP, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["bert", "clip", "bert-dropout"])
def test_encoder_layer_with_drop_path_one_call_matches_op_by_op(gpu, kind, lowp, monkeypatch):
    """p_path = 0.5 on both paths with the same seeds (each branch keeps one sample and drops another): the forward is bit-identical,
    the backward within the bounds of test_gpu_kernels.test_encoder_layer_one_call_matches_op_by_op.  The train output differs from
    the eval output, and the eval output is bit for bit that of a layer with p_path = 0."""
    from d2r_amd import functional as F
    from d2r_amd import modules as M
    layer, B, L, bert = _make_layer(kind, gpu, lowp)
    model, store = _prepare(layer, gpu, lowp)
    layer.p_path = P_PATH
    s_att = _pick_seed(_mixed, B=B)
    s_ffn = _pick_seed(_mixed, B=B, start=s_att + 1)
    assert _mixed(_keep_ref(B, P_PATH, s_att).numpy()) and _mixed(_keep_ref(B, P_PATH, s_ffn).numpy())
    x0 = torch.randn(B, L, 768, device=gpu).to(lowp)
    gy = torch.randn(B, L, 768, device=gpu).to(lowp)
    mask = torch.zeros(B, L, device=gpu)
    mask[0, L // 2:] = -10000.0
    run = (lambda x: layer(x, mask)) if bert else layer
    res = {}
    for composite in (False, True):
        M.COMPOSITE_LAYERS = composite
        _patch_seeds(monkeypatch, F, [s_att, s_ffn])
        try:
            store.zero_grad()
            x = x0.clone().requires_grad_(True)
            y = run(x)
            assert (type(y.grad_fn).__name__ == "_EncoderLayerBackward") == composite
            y.backward(gy)
            torch.cuda.synchronize()
            res[composite] = (y.detach().clone(), x.grad.clone(), store.flat_g.clone())
        finally:
            M.COMPOSITE_LAYERS = True
    (y0, dx0, g0), (y1, dx1, g1) = res[False], res[True]
    assert torch.equal(y0, y1), "forward differs"
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    print(f"drop_path layer[{kind} {lowp}]: dx rel {rel(dx1, dx0):.3e}")
    assert rel(dx1, dx0) < 1e-2, rel(dx1, dx0)
    for n, p, o, k, _ in store.entries:
        r = float((g1[o:o + k] - g0[o:o + k]).norm() / (g0[o:o + k].norm() + 1e-3 * g0.norm()))  # floor: a key bias has a mathematically zero gradient
        assert r < 2e-2, (n, r)
    layer.eval()
    with torch.no_grad():
        y_eval = run(x0)
        layer.p_path = 0.0
        y_eval0 = run(x0)
    assert not torch.equal(y_eval, y1), "the train output equals the eval output: no mask was applied"
    assert torch.equal(y_eval, y_eval0), "p_path changed the eval output"


def _sink(store, ptr, count):
    o = (ptr - store.flat_g.data_ptr()) // 4
    assert 0 <= o and o + count <= store.flat_g.numel()
    return slice(o, o + count)


def test_pre_ln_layer_dropped_sample_is_the_identity_bit_for_bit(gpu, monkeypatch):
    """One-call CLIP layer, bf16.  A sample dropped on both branches: y[b] is x[b] and dx[b] is dy[b], bit for bit (a select, and
    zero gradients into the skip connections).  Every sample dropped on the attention branch: the gradient sinks of w_qkv, b_qkv,
    w_o, b_o, pre-filled with random values, are bit-unchanged by the backward call (the FFN sinks are not)."""
    from d2r_amd import functional as F
    lowp = torch.bfloat16
    layer, B, L, _ = _make_layer("clip", gpu, lowp, B=3)
    model, store = _prepare(layer, gpu, lowp)
    layer.p_path = P_PATH
    x0 = torch.randn(B, L, 768, device=gpu).to(lowp)
    gy = torch.randn(B, L, 768, device=gpu).to(lowp)

    def run(seeds):
        _patch_seeds(monkeypatch, F, seeds)
        store.zero_grad()
        store.flat_g.copy_(torch.randn(store.flat_g.shape, generator=torch.Generator().manual_seed(11)).to(gpu))
        before = store.flat_g.clone()
        x = x0.clone().requires_grad_(True)
        y = layer(x)
        assert type(y.grad_fn).__name__ == "_EncoderLayerBackward"
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach(), x.grad, before, store.flat_g.clone()

    # sample 1 dropped on both branches, sample 0 kept on both
    pred = lambda k: bool(k[0]) and not bool(k[1])
    s_att = _pick_seed(pred, B=B)
    s_ffn = _pick_seed(pred, B=B, start=s_att + 1)
    y, dx, _, _ = run([s_att, s_ffn])
    i16 = torch.int16
    assert torch.equal(y[1].view(i16), x0[1].view(i16)), "y[b] of a sample dropped on both branches is not x[b]"
    assert torch.equal(dx[1].view(i16), gy[1].view(i16)), "dx[b] of a sample dropped on both branches is not dy[b]"
    assert not torch.equal(y[0], x0[0]) and not torch.equal(dx[0], gy[0])

    # every sample dropped on the attention branch, the FFN branch mixed
    s_att = _pick_seed(lambda k: not bool(k.any()), B=B)
    s_ffn = _pick_seed(_mixed, B=B)
    assert not bool(_keep_ref(B, P_PATH, s_att).any())
    _, _, before, after = run([s_att, s_ffn])
    t, E, Fi = layer._bundle_cache.template, 768, 3072
    for name, ptr, count in (("w_qkv", t.gw_qkv, 3 * E * E), ("b_qkv", t.gb_qkv, 3 * E), ("w_o", t.gw_o, E * E), ("b_o", t.gb_o, E)):
        s = _sink(store, ptr, count)
        assert torch.equal(before[s].view(torch.int32), after[s].view(torch.int32)), f"the sink of {name} changed"
    for name, ptr, count in (("w_1", t.gw_1, Fi * E), ("w_2", t.gw_2, E * Fi), ("b_2", t.gb_2, E)):
        s = _sink(store, ptr, count)
        assert not torch.equal(before[s], after[s]), f"the sink of {name} did not change: the backward pass did not run"


def _ref_attention(q, k, v, H, scale, mask):
    B, L, E = q.shape
    sp = lambda t: t.view(B, L, H, E // H).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask[:, None, None, :]
    return (torch.softmax(s, -1) @ sp(v)).transpose(1, 2).reshape(B, L, E)


def _ref_layer(bert, P, x, mask, branch):
    """The layer restated in plain torch (fp64, CPU).  P: parameters by the layer's own names; branch(k, t): what the residual branch
    k (0 attention, 1 FFN) becomes in front of its skip connection (element mask, path mask, their scales)."""
    lin = lambda t, n: t @ P[n + ".weight"].t() + P[n + ".bias"]
    ln = lambda t, n, eps: torch.nn.functional.layer_norm(t, (t.shape[-1],), P[n + ".weight"], P[n + ".bias"], eps)
    if bert:
        H, pre = 12, "attention.self."
        ctx = _ref_attention(lin(x, pre + "query"), lin(x, pre + "key"), lin(x, pre + "value"), H, (x.shape[-1] // H) ** -0.5, mask)
        a = ln(x + branch(0, lin(ctx, "attention.output.dense")), "attention.output.LayerNorm", 1e-12)
        h = torch.nn.functional.gelu(lin(a, "intermediate.dense"))
        return ln(a + branch(1, lin(h, "output.dense")), "output.LayerNorm", 1e-12)
    H, pre = 12, "self_attn."
    h = ln(x, "layer_norm1", 1e-5)
    ctx = _ref_attention(lin(h, pre + "q_proj"), lin(h, pre + "k_proj"), lin(h, pre + "v_proj"), H, (x.shape[-1] // H) ** -0.5, None)
    x1 = x + branch(0, lin(ctx, pre + "out_proj"))
    f = lin(ln(x1, "layer_norm2", 1e-5), "mlp.fc1")
    return x1 + branch(1, lin(f * torch.sigmoid(1.702 * f), "mlp.fc2"))


FP32_EPS = 2.0 ** -23


@pytest.mark.parametrize("kind", ["bert", "bert-dropout", "clip"])
def test_fp32_layer_with_drop_path_against_an_fp64_restatement(gpu, kind, monkeypatch):
    """The fp32 op-by-op layer (an un-prepared model: separate q / k / v, plain autograd gradients) against the restatement above
    with the masks of the reference generator; y, dx and every parameter gradient by relative L2 (a gradient's norm is floored by
    1e-3 of the norm of all gradients: the key bias has a mathematically zero one).  The same comparison at p_path = 0 runs the
    code as it was before stochastic depth and measures what fp32 arithmetic costs here; at p_path = 0.5 every figure may be 4 times
    that (two branches, each amplified by at most 1 / (1 - p) = 2), and never needs to be below 8 fp32 epsilons (9.5e-7).
    "bert-dropout": hidden dropout 0.1 on both dense outputs as well (the attention probabilities stay undropped: their element
    index is the fused core's business, tested elsewhere).
    Measured on an MI355X, p_path = 0 -> p_path = 0.5 (the largest figure over y, dx and the gradients, and dx alone):
    bert 9.46e-7 -> 9.88e-7 (dx 2.51e-7 -> 3.70e-7), bert-dropout 9.40e-7 -> 9.94e-7 (dx 2.61e-7 -> 3.82e-7), clip 1.06e-6 ->
    1.01e-6 (dx 2.34e-7 -> 3.21e-7); the largest ratio of any single figure is 1.7 (the attention-output bias of bert-dropout,
    3.03e-7 -> 5.06e-7)."""
    from d2r_amd import functional as F
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig
    p_hid = 0.1 if kind == "bert-dropout" else 0.0
    if kind.startswith("bert"):
        torch.manual_seed(3)
        layer, B, L, bert = M.BertLayer(TextConfig(num_hidden_layers=1, hidden_dropout_prob=p_hid, attention_probs_dropout_prob=0.0)), 3, 37, True
    else:
        layer, B, L, bert = _make_layer("clip", gpu, torch.float32)
    layer = layer.to(gpu).train()
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if "LayerNorm" in n or "layer_norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    E = 768
    gen = torch.Generator().manual_seed(5)
    x0, gy = torch.randn(B, L, E, generator=gen), torch.randn(B, L, E, generator=gen)
    mask = torch.zeros(B, L)
    mask[0, L // 2:] = -10000.0
    s_path = [_pick_seed(_mixed, B=B), 0]
    s_path[1] = _pick_seed(_mixed, B=B, start=s_path[0] + 1)

    def errors(p_path):
        layer.p_path = p_path
        _patch_seeds(monkeypatch, F, s_path)
        layer.zero_grad()
        x = x0.to(gpu).requires_grad_(True)
        y = layer(x, mask.to(gpu)) if bert else layer(x)
        assert type(y.grad_fn).__name__ != "_EncoderLayerBackward"
        y.backward(gy.to(gpu))
        torch.cuda.synchronize()

        def branch(k, t):  # seeds as _patch_seeds hands them out: element seeds 7000, 7001 (attention, FFN), then the path seeds
            if p_hid > 0:
                t = t * _keep_ref(B * L * E, p_hid, 7000 + k).view(B, L, E).double() / (1 - p_hid)
            if p_path > 0:
                t = t * _keep_ref(B, p_path, s_path[k]).view(B, 1, 1).double() / (1 - p_path)
            return t

        P = {n: p.detach().cpu().double().requires_grad_(True) for n, p in layer.named_parameters()}
        xr = x0.double().requires_grad_(True)
        yr = _ref_layer(bert, P, xr, mask.double() if bert else None, branch)
        yr.backward(gy.double())
        rel = lambda a, b, floor=0.0: float((a.detach().cpu().double() - b).norm() / (b.norm() + floor))
        out = {"y": rel(y, yr.detach()), "dx": rel(x.grad, xr.grad)}
        live = [n for n, p in layer.named_parameters() if p.grad is not None]
        assert sorted(live) == sorted(n for n, p in P.items() if p.grad is not None) and len(live) >= 16
        floor = 1e-3 * float(torch.cat([P[n].grad.flatten() for n in live]).norm())
        for n, p in layer.named_parameters():
            if p.grad is not None:
                out[n] = rel(p.grad, P[n].grad, floor)
        return out

    e0, e1 = errors(0.0), errors(P_PATH)
    for q in e0:
        print(f"drop_path fp32[{kind}] {q}: p_path=0 {e0[q]:.3e}  p_path={P_PATH} {e1[q]:.3e}  allowed {max(4 * e0[q], 8 * FP32_EPS):.3e}")
    print(f"drop_path fp32[{kind}] largest: p_path=0 {max(e0.values()):.3e}  p_path={P_PATH} {max(e1.values()):.3e}")
    bad = {q: (e0[q], e1[q]) for q in e0 if not e1[q] <= max(4 * e0[q], 8 * FP32_EPS)}
    assert not bad, bad


# ================================================================================================================================
# 5. The trainer
# ================================================================================================================================
def _train_two_steps(gpu, dtype, name, drop_path, call_set=None):
    """Two training steps (one epoch of two batches of 4, BERT dropout on) of a model with 2 encoder layers per tower ->
    (weights, step losses, the default generator's state afterwards, the log lines on stochastic depth, the model)."""
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.train import MSDTrainer
    from test_gpu_dataset_cache import _logger
    torch.manual_seed(31)
    torch.cuda.manual_seed_all(31)
    tc = TextConfig(num_hidden_layers=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    vc = VisionConfig(num_hidden_layers=2, image_size=64, patch_size=32)
    args = default_args(DR_step=3, compute_dtype=dtype, device=str(gpu), num_epochs=1, batch_size=4, warmup_ratio=0.0, save_path=None,
                        lr=1e-4, seed=31, drop_path=drop_path)
    model = M.UnimoModelF(args, vc, tc)
    if call_set is not None:
        model.model.set_drop_path(call_set)
    logger, catch = _logger(f"drop-path-trainer-{name}")
    train = make_loader(SyntheticMSDDataset(8, 16, 64, 3, seed=1, num_image_tokens=5), 4, True, 0, drop_last=True)
    tr = MSDTrainer(train_data=train, dev_data=None, test_data=None, model=model, args=args, logger=logger, writer=None)
    tr.train(None, None)
    torch.cuda.synchronize()
    assert tr.step == 2
    losses = [float(l.split("loss:")[1].split()[0]) for l in catch.lines if l.startswith("step ")]
    return tr.store.flat_w.clone(), losses, torch.get_rng_state(), [l for l in catch.lines if "tochastic depth" in l], model


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_trainer_with_drop_path(gpu, dtype):
    """Rates [0, 0.2] on two layers per tower (layer 0 takes the path it always took).  One seed twice: bit-identical weights and
    losses.  Against drop_path = 0: other weights, the same state of torch's default generator afterwards (dropout seeds and the
    sampler untouched).  drop_path = 0 is bit for bit a model on which set_drop_path(0) was called by hand.  In eval mode the trained
    model's logits do not depend on p_path."""
    tag = DT_IDS[dtype]
    w1, l1, s1, a1, model = _train_two_steps(gpu, dtype, f"{tag}-a", 0.2)
    w2, l2, s2, a2, _ = _train_two_steps(gpu, dtype, f"{tag}-b", 0.2)
    w0, l0, s0, a0, model0 = _train_two_steps(gpu, dtype, f"{tag}-off", 0.0)
    w3, l3, s3, a3, _ = _train_two_steps(gpu, dtype, f"{tag}-set0", 0.0, call_set=0.0)
    assert len(l1) == 1 and np.isfinite(l1[0]) and bool(torch.isfinite(w1).all())
    assert torch.equal(w1, w2) and l1 == l2, "two runs with one seed differ"
    assert not torch.equal(w1, w0), "drop_path changed nothing"
    assert torch.equal(s1, s0), "stochastic depth moved torch's default generator"
    assert torch.equal(w0, w3) and l0 == l3 and torch.equal(s0, s3), "set_drop_path(0) changed the run"
    assert len(a1) == 1 and "text tower [0, 0.2]" in a1[0] and "vision tower [0, 0.2]" in a1[0], a1
    assert not a0 and not a3
    assert [l.p_path for l in model.model.encoder.text_layer] == [0.0, 0.2]
    assert [l.p_path for l in model.model.encoder.vision_layers] == [0.0, 0.2]
    assert all(l.p_path == 0.0 for l in model0.model.encoder.text_layer)
    # eval mode: the logits of the trained model with p_path set, and cleared
    model.eval()
    gen = torch.Generator().manual_seed(9)
    ids = torch.randint(1000, 30000, (4, 16), generator=gen).to(gpu)
    images = torch.randn(4, 3, 64, 64, generator=gen).to(gpu)
    labels = torch.tensor([0, 1, 2, 1], device=gpu)
    with torch.no_grad():
        _, logits_set = model(ids, torch.ones_like(ids), torch.zeros_like(ids), labels, images)
        logits_set = logits_set.clone()
        model.model.set_drop_path(0.0)
        _, logits_cleared = model(ids, torch.ones_like(ids), torch.zeros_like(ids), labels, images)
    assert torch.equal(logits_set, logits_cleared) and bool(torch.isfinite(logits_set).all())
