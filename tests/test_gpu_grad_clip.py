"""GPU: gradient clipping by global norm (FusedAdamW(max_grad_norm=...), an extension beyond the reference) - the fp64 norm
pass against numpy, its overflow flag, parity with clip_grad_norm_ + torch.optim.AdamW, bit-identity where clipping must not
change anything (coef == 1, a power-of-two loss scale, hipGraph replay), the CLI and two data-parallel ranks."""
import ctypes
import math
import os
import re
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(dtype):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    tc = TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)
    args = default_args(DR_step=3, compute_dtype=dtype, device="cuda:0", num_epochs=2, batch_size=4, warmup_ratio=0.0,
                        save_path=None, lr=3e-5)
    return M.UnimoModelF(args, vc, tc), args


def _store(gpu, dtype, seed=21):
    from d2r_amd.params import ParamStore
    torch.manual_seed(seed)
    model, _ = _tiny(dtype)
    model.to(gpu).train()
    model.set_compute_dtype(dtype)
    return ParamStore(model, dtype)


def _grads(store, steps, seed, sigma):
    """One gradient per step over the live elements (alignment padding stays 0, as the dW kernels leave it)."""
    mask = torch.zeros(store.n, dtype=torch.bool)
    for _, _, o, k, _ in store.entries:
        mask[o:o + k] = True
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(store.n, generator=gen) * sigma * mask).to(store.flat_g.device) for _ in range(steps)]


def _norm_pass(g, ranges, max_norm=1.0, unscale=1.0, flag=None):
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    slab = torch.full((_lib.GRAD_NORM_PARTS,), float("nan"), dtype=torch.float64, device=g.device)  # every partial must be written
    out = torch.zeros(2, dtype=torch.float32, device=g.device)
    arr = (ctypes.c_int64 * max(1, 2 * len(ranges)))(*[x for r in ranges for x in r])
    _lib.call("d2r_grad_sumsq", g.data_ptr(), arr, len(ranges), slab.data_ptr(), slab.numel(), _stream())
    _lib.call("d2r_grad_norm_finish", slab.data_ptr(), slab.numel(), unscale, None, max_norm, out.data_ptr(),
              None if flag is None else flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    return slab.cpu(), out.cpu()


def _ref_sumsq(g, ranges):
    tot = 0.0
    for a, b in ranges:
        for c in range(a, b, 1 << 24):
            x = g[c:min(b, c + (1 << 24))].double()
            tot += float(torch.dot(x, x))
    return tot


def _values(n, regime, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, generator=gen, device="cuda")
    if regime == "tiny":
        x *= 1e-30  # squares underflow in fp32
    elif regime == "huge":
        x *= 1e30  # squares overflow in fp32
    elif regime == "mix":
        e = torch.randint(0, 3, (n,), generator=gen, device="cuda")
        x *= torch.tensor([1e-30, 1.0, 1e30], device="cuda")[e]
    return x


@pytest.mark.parametrize("n", [0, 1, 3, 4, 1023, (1 << 20) + 5, 300_000_003])
def test_norm_pass_matches_fp64(gpu, n):
    regimes = ("normal", "mix") if n > 1e8 else ("normal", "tiny", "huge", "mix")
    buf = torch.empty(n + 8, dtype=torch.float32, device=gpu)
    for ri, regime in enumerate(regimes):
        g = buf[:n]
        g.copy_(_values(n, regime, seed=n % 1000 + ri))
        host = g.cpu()
        splits = [[(0, n)]]
        if n > 64:  # a list of ranges with 16-byte aligned starts, one of them empty, ends anywhere
            q = n // 3 // 4 * 4
            splits.append([(0, q - 5), (q, q), (q, 2 * q + 1), (2 * q + 4, n)])
        for ranges in splits:
            ref = _ref_sumsq(host, ranges)
            slab, out = _norm_pass(g, ranges)
            assert not torch.isnan(slab).any(), "a partial was not written"
            tot = float(slab.sum())
            assert abs(tot - ref) <= 1e-12 * ref, (regime, ranges, tot, ref)
            want = math.sqrt(ref)
            assert abs(float(out[0]) - want) <= 1e-7 * want, (regime, float(out[0]), want)
            q = np.float32(1.0) / (np.float32(float(out[0])) + np.float32(1e-6))  # torch's fp32 coefficient for max_norm 1
            assert float(out[1]) == float(min(np.float32(1.0), q))
            slab2, out2 = _norm_pass(g, ranges)
            assert torch.equal(slab, slab2) and torch.equal(out, out2), "not reproducible"
        del host
    if n == 0:
        assert float(out[0]) == 0.0 and float(out[1]) == 1.0


def test_norm_pass_raises_the_overflow_flag(gpu):
    n = 4099  # 1024 packs and a tail of 3 elements
    base = torch.randn(n, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    _norm_pass(base, [(0, n)], flag=flag)
    assert int(flag) == 0
    for pos in (0, 1234, 4096, n - 1):  # first element, a packed element, a tail element, the last element
        for bad in (float("inf"), float("-inf"), float("nan")):
            g = base.clone()
            g[pos] = bad
            flag.zero_()
            _, out = _norm_pass(g, [(0, n)], flag=flag)
            assert int(flag) == 1, (pos, bad)
            assert not math.isfinite(float(out[0]))
    # an element outside the summed ranges does not count
    g = base.clone()
    g[4000] = float("inf")
    flag.zero_()
    _norm_pass(g, [(0, 3996)], flag=flag)
    assert int(flag) == 0
    # huge but finite: no overflow in the fp64 sum, no flag (the fp32 norm itself, 1.5e40, is inf - as torch's fp32 norm would be)
    flag.zero_()
    _, out = _norm_pass(base.clamp(-1.0, 1.0) * 3e38, [(0, n)], flag=flag)
    assert int(flag) == 0


@pytest.mark.parametrize("clips", [True, False], ids=["clipping", "not_clipping"])
def test_three_steps_match_clip_grad_norm_and_torch_adamw(gpu, clips):
    from d2r_amd.params import FusedAdamW
    store = _store(gpu, torch.float32)
    n_live = store.live_numel()
    grads = _grads(store, 3, seed=7, sigma=1.0 / math.sqrt(n_live))  # total norm ~1
    c = 0.25 if clips else 10.0
    lr = 1e-3
    opt = FusedAdamW(store, lr=lr, max_grad_norm=c)  # fc_lr 5e-2 as in the trainer
    # torch: the same live tensors, the reference's grouping
    tp = {n: store.flat_w[o:o + k].detach().clone().view(p.shape) for n, p, o, k, _ in store.entries}
    for t in tp.values():
        t.requires_grad_(True)
    groups = [dict(params=[tp[n] for n, _, _, _, gg in store.entries if gg == g], lr=(5e-2 if g == 3 else lr), weight_decay=1e-2)
              for g in range(4)]
    topt = torch.optim.AdamW([g for g in groups if g["params"]])
    for step, G in enumerate(grads):
        store.flat_g.copy_(G)
        opt.step()
        for n, p, o, k, _ in store.entries:
            tp[n].grad = G[o:o + k].view(p.shape).clone()
        tnorm = torch.nn.utils.clip_grad_norm_(list(tp.values()), c)
        topt.step()
        torch.cuda.synchronize()
        got = float(opt.last_grad_norm)
        assert abs(got - float(tnorm)) <= 1e-6 * float(tnorm), (step, got, float(tnorm))
        assert (float(tnorm) > c) == clips
        assert (float(opt._clip["out"][1]) < 1.0) == clips
    for n, p, o, k, g in store.entries:
        lr_g = 5e-2 if g == 3 else lr
        d = float((store.flat_w[o:o + k] - tp[n].detach().reshape(-1)).abs().max())
        assert d <= 1e-2 * lr_g, (n, d, lr_g)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_huge_max_norm_is_bit_identical_to_no_clipping(gpu, dtype):
    from d2r_amd.params import FusedAdamW
    store = _store(gpu, dtype)
    grads = _grads(store, 3, seed=9, sigma=1e-3)
    w0 = store.flat_w.clone()
    runs = []
    for mgn in (None, 1e30):
        store.flat_w.copy_(w0)
        store.refresh_lowp()
        opt = FusedAdamW(store, lr=1e-3, max_grad_norm=mgn)
        for G in grads:
            store.flat_g.copy_(G)
            opt.step()
        torch.cuda.synchronize()
        if mgn is not None:
            assert float(opt._clip["out"][1]) == 1.0
        runs.append((store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone()))
    for what, a, b in zip(("w", "m", "v", "lp"), *runs):
        assert torch.equal(a, b), what


def test_fp16_loss_scaled_gradients_clip_like_unscaled_ones(gpu):
    from d2r_amd.params import FusedAdamW
    S = 2.0 ** 14
    store = _store(gpu, torch.float16)
    grads = _grads(store, 3, seed=11, sigma=1e-3)
    c = 0.5 * float(grads[0].double().norm())  # clips
    w0 = store.flat_w.clone()
    runs = []
    for scaled in (False, True):
        store.flat_w.copy_(w0)
        store.refresh_lowp()
        opt = FusedAdamW(store, lr=1e-3, max_grad_norm=c)
        if scaled:
            opt.enable_loss_scaling(init_scale=S)
        norms = []
        for G in grads:
            store.flat_g.copy_(G * S if scaled else G)
            opt.step()
            norms.append(opt._clip["out"].clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(norms), store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone()))
    assert bool((runs[0][0][:, 1] < 1).all())
    for what, a, b in zip(("norm/coef", "w", "m", "v", "lp"), *runs):
        assert torch.equal(a, b), what
    # an overflowed step is dropped on the device, whatever the norm; the host halves the scale one step later
    before = (store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone())
    G = grads[0] * S
    G[12345] = float("inf")
    store.flat_g.copy_(G)
    opt.step()
    torch.cuda.synchronize()
    assert int(opt._scaler["flag"]) == 1
    for what, a, b in zip(("w", "m", "v", "lp"), before, (store.flat_w, opt.m, opt.v, store.flat_lp)):
        assert torch.equal(a, b), what
    opt._scaler_consume()
    assert opt.loss_scale == S / 2 and opt._scaler["skipped"] == 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_graph_replay_with_clipping_is_bit_identical_to_eager(gpu, dtype):
    """stage_hyper + a captured step_captured (norm pass, finish, AdamW reading coef) against eager step() over four steps; in
    fp16 the second step overflows, so the loss scale changes before the fourth."""
    from d2r_amd.params import FusedAdamW
    store = _store(gpu, dtype)
    grads = _grads(store, 4, seed=13, sigma=1e-3)
    c = 0.5 * float(grads[0].double().norm())
    w0 = store.flat_w.clone()
    runs = []
    for graph in (False, True):
        store.flat_w.copy_(w0)
        store.refresh_lowp()
        opt = FusedAdamW(store, lr=1e-3, max_grad_norm=c)
        if dtype == torch.float16:
            opt.enable_loss_scaling(init_scale=2.0 ** 12)
        if graph:
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                opt.step_captured()
        norms, scales = [], []
        for t, G in enumerate(grads):
            G = G * opt.loss_scale
            if dtype == torch.float16 and t == 1:
                G[777] = float("inf")
            scales.append(opt.loss_scale)
            store.flat_g.copy_(G)
            if graph:
                opt.stage_hyper()
                cg.replay()
                opt.after_replay()
            else:
                opt.step()
            norms.append(opt._clip["out"].clone())
        torch.cuda.synchronize()
        if dtype == torch.float16:
            opt._scaler_consume()
        runs.append((torch.stack(norms), store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone(), scales,
                     opt.step_count, opt.loss_scale))
    if dtype == torch.float16:
        assert runs[0][5][-1] != runs[0][5][0], runs[0][5]  # the scale changed within the run
    assert not torch.equal(runs[0][1], w0)
    for what, a, b in zip(("norm/coef", "w", "m", "v", "lp"), runs[0][:5], runs[1][:5]):
        assert torch.equal(a.nan_to_num(), b.nan_to_num()), what
    assert runs[0][5:] == runs[1][5:]


def test_sharded_capture_with_clipping_is_refused(gpu):
    from d2r_amd.params import FusedAdamW
    store = _store(gpu, torch.bfloat16)
    opt = FusedAdamW(store, lr=1e-3, max_grad_norm=1.0)
    opt.element_ranges = [(0, store.n)]
    opt.norm_element_ranges = [(0, store.n)]
    with pytest.raises(RuntimeError, match="sharded"):
        opt.step_captured()


def test_cli_logs_the_gradient_norm(gpu, tmp_path):
    cmd = [sys.executable, "-m", "d2r_amd.run", "--max_grad_norm", "1.0", "--num_epochs", "1", "--train_samples", "64",
           "--eval_samples", "8", "--batch_size", "8", "--encoder_layers", "1", "--image_size", "64", "--max_seq", "16",
           "--num_workers", "0", "--save_path", str(tmp_path) + "/", "--dtype", "bf16"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    norms = [float(x) for x in re.findall(r"grad_norm:(\S+)", r.stderr)]
    assert len(norms) == 4 and all(math.isfinite(x) and x > 0 for x in norms), r.stderr[-3000:]


def test_two_ranks_all_reduce_and_sharded_norms_agree(gpu, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "probes", "dp_grad_clip_two_ranks.py"), str(tmp_path)]
    proc = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True,
                            env=dict(os.environ, D2R_PROBE_DUMP_S="150"))
    try:
        out, err = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        out, err = proc.communicate()
        pytest.fail("the two ranks did not finish in 300 s: hang.\n--- stdout\n" + out[-3000:] + "\n--- stderr\n" + err[-6000:])
    assert proc.returncode == 0, "two-rank clipping probe failed\n--- stdout\n" + out[-3000:] + "\n--- stderr\n" + err[-6000:]
    res = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in (0, 1)]
    for r in res:
        for mode in ("all_reduce", "shard"):
            assert r[mode]["finite"] and r[mode]["same_ranks"], (mode, r[mode])
            assert all(c < 1.0 for c in r[mode]["coefs"]), r[mode]  # clipping triggered
        assert r["shard"]["gathered"] == 2 * r["shard"]["nseg"] * 2048
        for a, b in zip(r["all_reduce"]["totals"], r["shard"]["totals"]):
            assert abs(a - b) <= 1e-12 * a, (a, b)
        for a, b in zip(r["all_reduce"]["norms"], r["shard"]["norms"]):
            assert abs(a - b) <= 2.5e-7 * a, (a, b)  # fp32 roundings of (nearly) the same fp64 norm
    # every rank holds the same norm and coefficient, bit for bit
    for mode in ("all_reduce", "shard"):
        assert res[0][mode]["norms"] == res[1][mode]["norms"] and res[0][mode]["coefs"] == res[1][mode]["coefs"], mode
