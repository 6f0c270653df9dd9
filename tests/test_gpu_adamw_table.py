"""GPU: AdamW with per-parameter hyper-parameters (d2r_adamw_step_table / _dev; FusedAdamW(layer_lr_decay=..., decay_exempt_1d=...),
an extension beyond the reference) - the raw entry point against an fp64 model, bit-identity under every cut of the range into
launches, a dropped step, FusedAdamW against torch.optim.AdamW with a group per parameter, the captured step, complementary
sharded ranges and the CLI."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the raw ABI -------------------------------------------------------------------------------------------------------------
# n = 4099 is no multiple of 4; three one-element segments inside the first pack; a boundary inside a pack (7, 1030, 3000 % 4 == 0
# is on a pack but off the span); boundaries on (1024, 2048) and off (1030, 3000) the 1,024-element span of a workgroup's pass.
# Neighbours always differ in the scale or the decay (or both), and in the group.
N = 4099
SEGS = [(1, 1.0, 0.0, 0), (2, 0.5, 0.0, 1), (3, 0.25, 0.5, 0), (7, 1.0, 0.5, 1), (1024, 0.5, 0.0, 0), (1030, 0.0, 0.5, 1),
        (2048, 1.0, 0.0, 0), (3000, 0.0, 0.0, 1), (4099, 0.25, 0.5, 0)]
LR = (1e-3, 2e-3)  # of the two groups
B1, B2, EPS = 0.9, 0.999, 1e-8
GSCALE, COEF, OMD = 0.5, 0.625, 0.25
GUARD = 64  # elements of NaN on either side of every buffer: 256 bytes of fp32, 128 of the shadow - the base pointers stay aligned
DT = {None: None, "bf16": torch.bfloat16, "fp16": torch.float16}


def _per_element(col):
    out, a = np.zeros(N), 0
    for seg in SEGS:
        out[a:seg[0]] = seg[col]
        a = seg[0]
    return out


def _inputs(steps=3, seed=5):
    gen = torch.Generator().manual_seed(seed)
    w0 = (torch.rand(N, generator=gen) * 2 - 1) * 0.1
    grads = [torch.randn(N, generator=gen) * 1e-2 for _ in range(steps)]
    return w0, grads


class _Bufs:
    """w, g, m, v, ema (fp32) and the shadow between NaN guard bands; `view(x)` is the live part."""

    def __init__(self, gpu, w0, lp):
        self.names = ["w", "g", "m", "v", "ema"] + (["w16"] if lp is not None else [])
        for k in self.names:
            setattr(self, k, torch.full((N + 2 * GUARD,), float("nan"), dtype=lp if k == "w16" else torch.float32, device=gpu))
        self.view("w").copy_(w0)
        self.view("ema").copy_(w0)
        self.view("m").zero_()
        self.view("v").zero_()
        self.view("g").zero_()
        if lp is not None:
            self.view("w16").copy_(w0.to(lp))

    def view(self, k):
        return getattr(self, k)[GUARD:GUARD + N]

    def ptr(self, k):
        return getattr(self, k).data_ptr() + GUARD * getattr(self, k).element_size()

    def bits(self):
        return {k: getattr(self, k).view(torch.int32 if k != "w16" else torch.int16).clone() for k in self.names}

    def guards_intact(self):
        for k in self.names:
            t = getattr(self, k)
            assert bool(torch.isnan(t[:GUARD]).all()) and bool(torch.isnan(t[GUARD + N:]).all()), f"guard band of {k} was written"


def _upload_table(gpu):
    from d2r_amd import _lib
    arr = (_lib.AdamwSeg * len(SEGS))(*[_lib.AdamwSeg(e, s, wd, q, 0) for e, s, wd, q in SEGS])
    _lib.call("d2r_adamw_table_check", arr, len(SEGS), N, 2)
    return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(gpu)


def _run(gpu, lp_name, clip_ema, cuts, skip=None, steps=3):
    """`steps` steps from the shared inputs, each as one launch per (begin, end) of `cuts`; -> the buffers."""
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    w0, grads = _inputs(steps)
    b = _Bufs(gpu, w0, DT[lp_name])
    table = _upload_table(gpu)
    coef = torch.tensor([COEF], dtype=torch.float32, device=gpu)
    lr = (ctypes.c_float * 2)(*LR)
    for t, G in enumerate(grads, 1):
        b.view("g").copy_(G)
        for lo, hi in cuts:
            _lib.call("d2r_adamw_step_table", b.ptr("w"), b.ptr("g"), b.ptr("m"), b.ptr("v"), b.ptr("w16") if lp_name else None,
                      {None: _lib.BF16, "bf16": _lib.BF16, "fp16": _lib.F16}[lp_name], lo, hi, table.data_ptr(), len(SEGS), N, lr, 2,
                      B1, B2, EPS, t, GSCALE, None if skip is None else skip.data_ptr(), coef.data_ptr() if clip_ema else None,
                      b.ptr("ema") if clip_ema else None, OMD if clip_ema else 0.0, _stream())
    torch.cuda.synchronize()
    return b


def _fp64_model(clip_ema, steps=3):
    w0, grads = _inputs(steps)
    f = lambda x: float(np.float32(x))
    lr_eff = (np.float32(np.array(LR, dtype=np.float32)[_per_element(3).astype(int)]) * np.float32(_per_element(1))).astype(np.float64)
    wd = _per_element(2)
    b1, b2, eps = f(B1), f(B2), f(EPS)
    w, m, v = w0.double().numpy().copy(), np.zeros(N), np.zeros(N)
    e = w.copy()
    for t, G in enumerate(grads, 1):
        g = G.double().numpy() * GSCALE * (COEF if clip_ema else 1.0)
        w = w * (1.0 - lr_eff * wd)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        bc1, bc2s = f(1.0 - b1 ** t), f(math.sqrt(1.0 - b2 ** t))
        w = w - (lr_eff / bc1) * (m / (np.sqrt(v) / bc2s + eps))
        e = e + OMD * (w - e)
    return dict(w=w, m=m, v=v, ema=e, lr_eff=lr_eff, gmax=max(float(G.abs().max()) for G in grads) * GSCALE)


@pytest.mark.parametrize("clip_ema", [False, True], ids=["plain", "clip_ema"])
@pytest.mark.parametrize("lp_name", [None, "bf16", "fp16"], ids=["no_shadow", "bf16", "fp16"])
def test_raw_abi_matches_fp64_model(gpu, lp_name, clip_ema):
    """Three steps of one launch over [0, n).  |w - fp64| <= 1e-2 * lr_eff of the element's segment (the bound of this kernel family,
    tests/test_gpu_grad_clip.py): with |w| <= 0.1 an fp32 ulp of w is 7.5e-9, far below; a neighbour's scale or decay misses it by
    5x and more.  A scale-0 segment has no budget: w stays bit-identical there, while m and v move and the shadow is the cast of w.
    m, v: three steps of at most three roundings (2^-24 relative each) of values up to gmax (gmax^2): 1e-6 * gmax (gmax^2) covers
    9 * 6e-8.  ema: a convex combination of the weights, so within their bound, plus 6 k u M of its own roundings (k = 3 steps, u = 2^-24,
    M = 0.11 >= |w|: the bound derived in tests/test_gpu_ema.py)."""
    w0, _ = _inputs()
    ref = _fp64_model(clip_ema)
    b = _run(gpu, lp_name, clip_ema, [(0, N)])
    b.guards_intact()
    w, m, v = (b.view(k).double().cpu().numpy() for k in ("w", "m", "v"))
    err = np.abs(w - ref["w"])
    frozen = ref["lr_eff"] == 0.0
    assert frozen.sum() == (1030 - 1024) + (3000 - 2048)
    worst = float((err[~frozen] / ref["lr_eff"][~frozen]).max())
    print(f"    max |w - fp64| / lr_eff = {worst:.3e} (bound 1e-2)")
    assert bool((err[~frozen] <= 1e-2 * ref["lr_eff"][~frozen]).all()), worst
    assert torch.equal(b.view("w").cpu()[torch.from_numpy(frozen)], w0[torch.from_numpy(frozen)]), "a scale-0 segment moved"
    assert bool((np.abs(m - ref["m"]) <= 1e-6 * ref["gmax"]).all()) and bool((np.abs(v - ref["v"]) <= 1e-6 * ref["gmax"] ** 2).all())
    assert bool((np.abs(m[frozen]) > 0).all()) and bool((v[frozen] > 0).all()), "m, v of a scale-0 segment must still be updated"
    if lp_name:
        assert torch.equal(b.view("w16"), b.view("w").to(DT[lp_name])), "the shadow is not the cast of w"
    if clip_ema:
        e = b.view("ema").double().cpu().numpy()
        assert bool((np.abs(e - ref["ema"]) <= 1e-2 * ref["lr_eff"] + 6 * 3 * 2.0 ** -24 * 0.11).all())
        assert torch.equal(b.view("ema").cpu()[torch.from_numpy(frozen)], w0[torch.from_numpy(frozen)])
    else:
        assert torch.equal(b.view("ema").cpu(), w0), "ema was written without being asked for"
    again = _run(gpu, lp_name, clip_ema, [(0, N)])
    for k, x in b.bits().items():
        assert torch.equal(x, again.bits()[k]), f"{k} differs between two runs from the same inputs"


@pytest.mark.parametrize("clip_ema", [False, True], ids=["plain", "clip_ema"])
def test_partition_invariance_bit_for_bit(gpu, clip_ema):
    base = _run(gpu, "bf16", clip_ema, [(0, N)])
    thirds = [(0, 1028), (1028, 2052), (2052, N)]
    chunks = [(a, min(a + 516, N)) for a in range(0, N, 516)]
    assert all(a % 4 == 0 for a, _ in thirds + chunks) and len(chunks) == 8
    for what, cuts in (("three launches", thirds), ("chunks of 516", chunks), ("chunks, last first", chunks[::-1])):
        got = _run(gpu, "bf16", clip_ema, cuts)
        got.guards_intact()
        for k in ("w", "m", "v", "ema", "w16"):
            assert torch.equal(got.view(k), base.view(k)), (what, k)
    assert not torch.equal(base.view("w").cpu(), _inputs()[0])


@pytest.mark.parametrize("form", ["eager", "dev"])
def test_raised_skip_flag_changes_nothing(gpu, form):
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    w0, grads = _inputs()
    b = _Bufs(gpu, w0, torch.bfloat16)
    b.view("g").copy_(grads[0])
    b.view("m").copy_(grads[1])
    b.view("v").copy_(grads[2] ** 2)
    before = b.bits()
    table = _upload_table(gpu)
    flag = torch.ones(1, dtype=torch.int32, device=gpu)
    coef = torch.tensor([COEF], dtype=torch.float32, device=gpu)
    head = (b.ptr("w"), b.ptr("g"), b.ptr("m"), b.ptr("v"), b.ptr("w16"), _lib.BF16, 0, N, table.data_ptr(), len(SEGS), N)
    if form == "eager":
        _lib.call("d2r_adamw_step_table", *head, (ctypes.c_float * 2)(*LR), 2, B1, B2, EPS, 1, 1.0, flag.data_ptr(), coef.data_ptr(),
                  b.ptr("ema"), OMD, _stream())
    else:
        hyper = torch.tensor([[LR[0], 0.1, 0.0316, 1.0], [LR[1], 0.1, 0.0316, 1.0]], dtype=torch.float32, device=gpu)
        omd = torch.tensor([OMD], dtype=torch.float32, device=gpu)
        _lib.call("d2r_adamw_step_table_dev", *head, hyper.data_ptr(), 2, B1, B2, EPS, flag.data_ptr(), coef.data_ptr(), b.ptr("ema"),
                  omd.data_ptr(), _stream())
    torch.cuda.synchronize()
    for k, x in b.bits().items():
        assert torch.equal(x, before[k]), f"{k} changed in a dropped step"


# ---- FusedAdamW --------------------------------------------------------------------------------------------------------------
def _tiny(dtype):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    tc = TextConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=2, image_size=64, patch_size=32)
    args = default_args(DR_step=3, compute_dtype=dtype, device="cuda:0", num_epochs=2, batch_size=4, warmup_ratio=0.0,
                        save_path=None, lr=3e-5)
    return M.UnimoModelF(args, vc, tc), args


_STORES = {}


def _store(gpu, dtype):
    """One store per dtype for the whole module (building the model is most of a test's time); the tests restore its weights."""
    from d2r_amd.params import ParamStore
    if dtype not in _STORES:
        torch.manual_seed(21)
        model, _ = _tiny(dtype)
        model.to(gpu).train()
        model.set_compute_dtype(dtype)
        st = ParamStore(model, dtype)
        _STORES[dtype] = (st, st.flat_w.clone())
    st, w0 = _STORES[dtype]
    st.flat_w.copy_(w0)
    st.refresh_lowp()
    st.flat_g.zero_()
    return st


def _grads(store, steps, seed, sigma):
    mask = torch.zeros(store.n, dtype=torch.bool)
    for _, _, o, k, _ in store.entries:
        mask[o:o + k] = True
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(store.n, generator=gen) * sigma * mask).to(store.flat_g.device) for _ in range(steps)]


@pytest.mark.parametrize("variant", ["plain", "clip", "ema"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fused_adamw_matches_torch_adamw_with_a_group_per_parameter(gpu, dtype, variant):
    """2 + 2 layers, layer_lr_decay 0.5, no decay on 1-D parameters, three steps; |w - torch| <= 1e-2 * lr of the parameter (the
    smallest scale is 0.5 ** 3, so the bound is at least 1.25e-6, well above the rounding of weights of size 1)."""
    from d2r_amd.params import FusedAdamW, ema_one_minus_decay, layer_lr_scale
    store = _store(gpu, dtype)
    assert (store.n_text_layers, store.n_vision_layers) == (2, 2)
    n_live = store.live_numel()
    grads = _grads(store, 3, seed=7, sigma=1.0 / math.sqrt(n_live))  # total norm ~1
    lr, wd, c = 1e-3, 1e-2, 0.25
    opt = FusedAdamW(store, lr=lr, weight_decay=wd, layer_lr_decay=0.5, decay_exempt_1d=True,
                     max_grad_norm=c if variant == "clip" else None, ema_decay=0.9 if variant == "ema" else None)
    assert opt.table is not None and 50 < len(opt.table) <= len(store.entries)
    assert opt.tower_lr_scales == (0.125, 0.125)
    lr_of = {n: (5e-2 if g == 3 else lr) * layer_lr_scale(n, 2, 2, 0.5) for n, _, _, _, g in store.entries}
    assert min(lr_of.values()) == lr * 0.125
    tp = {n: store.flat_w[o:o + k].detach().clone().view(p.shape) for n, p, o, k, _ in store.entries}
    for t in tp.values():
        t.requires_grad_(True)
    topt = torch.optim.AdamW([dict(params=[tp[n]], lr=lr_of[n], weight_decay=0.0 if p.dim() <= 1 else wd)
                              for n, p, _, _, _ in store.entries])
    E, M = store.flat_w.double(), store.flat_w.abs().double()
    for step, G in enumerate(grads, 1):
        store.flat_g.copy_(G)
        opt.step()
        for n, p, o, k, _ in store.entries:
            tp[n].grad = G[o:o + k].view(p.shape).clone()
        if variant == "clip":
            tnorm = torch.nn.utils.clip_grad_norm_(list(tp.values()), c)
            torch.cuda.synchronize()
            got = float(opt.last_grad_norm)
            assert abs(got - float(tnorm)) <= 1e-6 * float(tnorm), (step, got, float(tnorm))
            assert float(tnorm) > c and float(opt._clip["out"][1]) < 1.0
        topt.step()
        if variant == "ema":  # the fp64 recurrence over the path's own weights, with the bound derived in tests/test_gpu_ema.py
            E = E + float(np.float32(ema_one_minus_decay(0.9, step))) * (store.flat_w.double() - E)
            M = torch.maximum(M, store.flat_w.abs().double())
    torch.cuda.synchronize()
    worst = 0.0
    for n, p, o, k, g in store.entries:
        d = float((store.flat_w[o:o + k] - tp[n].detach().reshape(-1)).abs().max())
        worst = max(worst, d / lr_of[n])
        assert d <= 1e-2 * lr_of[n], (n, d, lr_of[n])
    print(f"    max |w - torch| / lr of the parameter = {worst:.3e} (bound 1e-2)")
    if dtype == torch.bfloat16:
        assert torch.equal(store.flat_lp, store.flat_w.to(torch.bfloat16))
    if variant == "ema":
        assert bool(((opt.ema.double() - E).abs() <= 6.0 * 3 * 2.0 ** -24 * M * (1.0 + 2.0 ** -20)).all())


def test_options_off_keep_the_launch_per_group(gpu):
    """layer_lr_decay None or 1 without the exemption builds no table: the optimiser steps exactly as before."""
    from d2r_amd.params import FusedAdamW
    store = _store(gpu, torch.bfloat16)
    grads = _grads(store, 2, seed=3, sigma=1e-3)
    runs = []
    for kw in (dict(), dict(layer_lr_decay=1.0, decay_exempt_1d=False), dict(layer_lr_decay=None)):
        store = _store(gpu, torch.bfloat16)
        opt = FusedAdamW(store, lr=1e-3, **kw)
        assert opt.table is None
        for G in grads:
            store.flat_g.copy_(G)
            opt.step()
        torch.cuda.synchronize()
        runs.append((store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))


@pytest.mark.parametrize("variant", ["plain", "clip_ema"])
def test_graph_replay_is_bit_identical_to_eager(gpu, variant):
    """stage_hyper + a captured step_captured (one d2r_adamw_step_table_dev) against eager step() over four steps while the
    schedule moves the group rates."""
    from d2r_amd.params import FusedAdamW, LinearWarmupSchedule
    store = _store(gpu, torch.bfloat16)
    grads = _grads(store, 4, seed=13, sigma=1e-3)
    c = 0.5 * float(grads[0].double().norm())
    w0 = store.flat_w.clone()
    runs = []
    for graph in (False, True):
        store = _store(gpu, torch.bfloat16)
        opt = FusedAdamW(store, lr=1e-3, layer_lr_decay=0.5, decay_exempt_1d=True,
                         **(dict(max_grad_norm=c, ema_decay=0.9) if variant == "clip_ema" else {}))
        sched = LinearWarmupSchedule(opt, 2, 6)
        if graph:
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                opt.step_captured()
        lrs = []
        for G in grads:
            store.flat_g.copy_(G)
            lrs.append(tuple(sched.get_last_lr()))
            if graph:
                opt.stage_hyper()
                cg.replay()
                opt.after_replay()
            else:
                opt.step()
            sched.step()
        torch.cuda.synchronize()
        runs.append((store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone(),
                     opt.ema.clone() if opt.ema is not None else w0, lrs, opt.step_count))
    assert len(set(runs[0][5])) == 4, runs[0][5]  # the rates moved every step
    assert not torch.equal(runs[0][0], w0)
    for what, a, b in zip(("w", "m", "v", "lp", "ema"), runs[0][:5], runs[1][:5]):
        assert torch.equal(a, b), what
    assert runs[0][5:] == runs[1][5:]


def test_complementary_sharded_ranges_reproduce_the_unsharded_step(gpu):
    """Two optimisers over one store take complementary element_ranges, cut at 4-aligned points INSIDE segments; each updates its
    own ranges of the shared weights (and of its own m, v, ema).  Put together: the unsharded step, bit for bit."""
    from d2r_amd.params import FusedAdamW
    store = _store(gpu, torch.bfloat16)
    grads = _grads(store, 3, seed=17, sigma=1e-3)
    kw = dict(lr=1e-3, layer_lr_decay=0.5, decay_exempt_1d=True, ema_decay=0.9)
    ref = FusedAdamW(store, **kw)
    for G in grads:
        store.flat_g.copy_(G)
        ref.step()
    torch.cuda.synchronize()
    want = (store.flat_w.clone(), ref.m.clone(), ref.v.clone(), ref.ema.clone(), store.flat_lp.clone())
    # cut points: 4-aligned, strictly inside a segment, spread over the buffer
    inside, a0 = [], 0
    for e, *_ in ref.table:
        x = (a0 + (e - a0) // 2) // 4 * 4
        if a0 < x < e:
            inside.append(x)
        a0 = e
    cuts = [inside[len(inside) * k // 7] for k in range(1, 7)]
    assert len(set(cuts)) == 6 and all(x % 4 == 0 for x in cuts)
    bounds = [0] + cuts + [store.n]
    ranges = list(zip(bounds[:-1], bounds[1:]))
    store = _store(gpu, torch.bfloat16)
    a, b = FusedAdamW(store, **kw), FusedAdamW(store, **kw)
    a.element_ranges, b.element_ranges = ranges[0::2], ranges[1::2]
    for G in grads:
        store.flat_g.copy_(G)
        a.step()
        b.step()
    torch.cuda.synchronize()
    own_a = torch.zeros(store.n, dtype=torch.bool, device=gpu)
    for lo, hi in a.element_ranges:
        own_a[lo:hi] = True
    got = (store.flat_w, torch.where(own_a, a.m, b.m), torch.where(own_a, a.v, b.v), torch.where(own_a, a.ema, b.ema), store.flat_lp)
    for what, x, y in zip(("w", "m", "v", "ema", "lp"), got, want):
        assert torch.equal(x, y), what
    assert not torch.equal(a.m, want[1]) and not torch.equal(b.m, want[1])  # each took only its own ranges


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def _cli(args, cwd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "d2r_amd.run", *args], cwd=str(cwd), env=env,
                       capture_output=True, text=True)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


def test_cli_logs_the_table_and_ignores_the_flags_with_only_test(gpu, tmp_path):
    save = str(tmp_path / "out") + "/"
    line = ["--num_epochs", "1", "--train_samples", "32", "--eval_samples", "16", "--encoder_layers", "2", "--layer_lr_decay", "0.8",
            "--wd_exempt_1d", "--weight_decay", "0.05"]
    small = ["--batch_size", "8", "--image_size", "64", "--max_seq", "16", "--num_workers", "0", "--dtype", "bf16", "--save_path", save]
    log = _cli(line + small, tmp_path)
    m = re.search(r"(\d+) segments in one launch \(layer_lr_decay 0\.8, weight decay 0\.05, none on 1-D parameters\); "
                  r"smallest lr scale: text tower (\S+), vision tower (\S+)", log)
    assert m, log[-3000:]
    assert int(m.group(1)) > 50
    assert abs(float(m.group(2)) - 0.8 ** 3) < 1e-6 and abs(float(m.group(3)) - 0.8 ** 3) < 1e-6
    assert re.search(r"step \d+ loss:", log)
    ck = os.path.join(save, "best_model.pth")
    assert os.path.exists(ck)
    log2 = _cli(line + small + ["--only_test", "--load_path", ck], tmp_path)
    assert "--layer_lr_decay / --wd_exempt_1d / --weight_decay are ignored with --only_test" in log2
    assert "segments in one launch" not in log2 and "Running training" not in log2
