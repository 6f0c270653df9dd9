"""GPU: the weight EMA of the fused AdamW step (FusedAdamW(ema_decay=...), an extension beyond the reference) - the _ema entry
points against an fp64 recurrence and, bit for bit, against the entry points without it on every dispatch path; a dropped step;
d2r_swap_f32; bit-identity of everything else with EMA on and off; hipGraph replay; the trainer's checkpoint of averaged weights;
the CLI; two data-parallel ranks under the sharded optimiser."""
import ctypes
import logging
import math
import os
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD = 64  # elements of NaN on both sides of a guarded range (256 bytes: the range keeps the allocation's alignment)
# an empty range; tail-only ranges; a vector loop plus a tail; one and three trips of the grid-stride loop past the 2048-block cap
# (2048 blocks * 256 threads * 4 elements = 1 << 21)
SIZES = [0, 1, 3, 4, 5, 1023, (1 << 21) + 5, 3 * (1 << 21) + 1]
LR, B1, B2, EPS, WD, GSCALE, COEF = 1e-2, 0.9, 0.999, 1e-8, 1e-2, 0.5, 0.37


def _f(x):
    return ctypes.c_float(x)


class Guarded:
    """fp32 [n] between two NaN bands; the address is taken from the allocation (an empty view has none of its own)."""

    def __init__(self, values, n, off=0):
        self.n, self.off = n, off
        self.buf = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device="cuda")
        self.view = self.buf[GUARD + off:GUARD + off + n]
        self.view.copy_(values)
        self.ptr = self.buf.data_ptr() + 4 * (GUARD + off)

    def bands_intact(self):
        lo, hi = self.buf[:GUARD + self.off], self.buf[GUARD + self.off + self.n:]
        return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())


def _ptr(t, base):
    return base.data_ptr() if t.numel() == 0 else t.data_ptr()


def _inputs(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda: torch.randn(n, generator=gen, device="cuda")
    return dict(w=r(), m=r() * 1e-3, v=r().abs() * 1e-6, e=r(), g=[r() * 1e-3 for _ in range(3)])


def _omds():
    """1 - d_t at three points of the schedule of decay 0.999: deep in the warm-up, later in it, and past it."""
    from d2r_amd.params import ema_one_minus_decay
    return [ema_one_minus_decay(0.999, t) for t in (1, 50, 9000)]  # 9/11, 0.15, 0.001


def _run(inp, n, lowp, clip, dev_form, ema_on, skip=None):
    """Three steps through one entry point.  -> (w, m, v, shadow or None, guarded ema or None, [w after each step])."""
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    pad = torch.zeros(8, dtype=torch.float32, device="cuda")  # an address for the empty ranges
    w, m, v = inp["w"].clone(), inp["m"].clone(), inp["v"].clone()
    sh = None if lowp is None else torch.zeros(n, dtype=lowp, device="cuda")
    sh_dtype = _lib.F16 if lowp == torch.float16 else _lib.BF16
    ema = Guarded(inp["e"], n) if ema_on else None
    coef = torch.tensor([COEF], dtype=torch.float32, device="cuda") if clip else None
    hyper = torch.zeros(4, dtype=torch.float32, device="cuda")
    d_omd = torch.zeros(1, dtype=torch.float32, device="cuda")
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    trail = []
    for t, (g, omd) in enumerate(zip(inp["g"], _omds()), start=1):
        head = (_ptr(w, pad), _ptr(g, pad), _ptr(m, pad), _ptr(v, pad), None if sh is None else _ptr(sh, pad), sh_dtype, n)
        cp = None if coef is None else coef.data_ptr()
        if dev_form:
            hyper.copy_(torch.tensor([LR, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), GSCALE], dtype=torch.float32))
            d_omd.copy_(torch.tensor([omd], dtype=torch.float32))
            mid = (hyper.data_ptr(), _f(B1), _f(B2), _f(EPS), _f(WD), skip)
            if ema_on:
                _lib.call("d2r_adamw_step_dev_ema", *head, *mid, cp, ema.ptr, d_omd.data_ptr(), _stream())
            elif clip:
                _lib.call("d2r_adamw_step_dev_clip", *head, *mid, cp, _stream())
            else:
                _lib.call("d2r_adamw_step_dev", *head, *mid, _stream())
        else:
            mid = (_f(LR), _f(B1), _f(B2), _f(EPS), _f(WD), t, _f(GSCALE), skip)
            if ema_on:
                _lib.call("d2r_adamw_step_ema", *head, *mid, cp, ema.ptr, _f(omd), _stream())
            elif clip:
                _lib.call("d2r_adamw_step_clip", *head, *mid, cp, _stream())
            else:
                _lib.call("d2r_adamw_step", *head, *mid, _stream())
        trail.append(w.clone())
    torch.cuda.synchronize()
    return w, m, v, sh, ema, trail


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


@pytest.mark.parametrize("n", SIZES)
def test_ema_step_matches_fp64_and_leaves_adamw_bit_identical_on_every_path(gpu, n):
    """For every path (bf16 / fp16 / no shadow, with and without d_coef, eager and device-scalar form), three steps:
    w, m, v and the shadow equal the entry point without EMA bit for bit, and ema follows the fp64 recurrence
    E <- E + omd * (W - E) fed the kernel's own fp32 weights W after each step and the fp32 factor omd the kernel saw.

    Error bound, per element, with u = 2^-24 (half an ulp, relative) and M = max(|e_0|, |w_1|, |w_2|, |w_3|), which also bounds
    every |e_t| because e_t is a convex combination of them (0 <= omd <= 1): one step computes fl(e + fl(omd * fl(w - e))).
      fl(w - e):   |w - e| <= 2M, so the rounding is at most u * 2M;
      fl(omd * .): |omd * (w - e)| <= 2M, at most u * 2M (and the error inherited from the line above is scaled by omd <= 1);
      fl(e + .):   the sum is the new average, <= M <= 2M in magnitude, at most u * 2M.
    A step therefore adds at most 3 * u * 2M = 6 u M, and the error already in e is carried with the factor d_t = 1 - omd <= 1, so
    after k steps |e - E| <= 6 k u M.  (1 + 2^-20) covers the second-order terms and the fp64 reference's own roundings.  A fused
    multiply-add drops one of the three roundings: the bound is then looser than needed, never too tight."""
    inp = _inputs(n, seed=1000 + n % 997)
    omds32 = [float(np.float32(o)) for o in _omds()]
    u = 2.0 ** -24
    for lowp in (torch.bfloat16, torch.float16, None):
        for clip in (False, True):
            for dev_form in (False, True):
                tag = (n, str(lowp), "clip" if clip else "noclip", "dev" if dev_form else "eager")
                base = _run(inp, n, lowp, clip, dev_form, ema_on=False)
                got = _run(inp, n, lowp, clip, dev_form, ema_on=True)
                for what, a, b in zip(("w", "m", "v", "shadow"), base[:4], got[:4]):
                    if a is not None:
                        assert torch.equal(_bits(a), _bits(b)), (tag, what)
                for a, b in zip(base[5], got[5]):
                    assert torch.equal(_bits(a), _bits(b)), (tag, "w of an earlier step")
                ema = got[4]
                assert ema.bands_intact(), (tag, "a guard band of ema was written")
                if n:
                    assert not torch.equal(got[0], inp["w"]), (tag, "the weights did not move")
                    E, M = inp["e"].double(), inp["e"].abs().double()
                    for k, (W, omd) in enumerate(zip(got[5], omds32), start=1):
                        E = E + omd * (W.double() - E)
                        M = torch.maximum(M, W.abs().double())
                    err = (ema.view.double() - E).abs()
                    bound = 6.0 * 3 * u * M * (1.0 + 2.0 ** -20)
                    worst = float((err / bound.clamp_min(1e-300)).max())
                    print(f"    {tag}: max |ema - fp64| / bound = {worst:.3f}")
                    assert bool((err <= bound).all()), (tag, worst)
                    assert float((ema.view - inp["e"]).abs().max()) > 0, (tag, "ema did not move")
                again = _run(inp, n, lowp, clip, dev_form, ema_on=True)
                assert torch.equal(_bits(again[4].buf), _bits(ema.buf)), (tag, "not reproducible")


@pytest.mark.parametrize("dev_form", [False, True], ids=["eager", "dev"])
def test_a_dropped_step_leaves_ema_and_everything_else_untouched(gpu, dev_form):
    n = 4099  # 1024 packs and a tail of 3
    inp = _inputs(n, seed=5)
    flag = torch.ones(1, dtype=torch.int32, device=gpu)
    for lowp in (torch.bfloat16, torch.float16, None):
        w, m, v, sh, ema, _ = _run(inp, n, lowp, True, dev_form, ema_on=True, skip=flag.data_ptr())
        for what, a, b in zip(("w", "m", "v", "ema"), (w, m, v, ema.view), (inp["w"], inp["m"], inp["v"], inp["e"])):
            assert torch.equal(_bits(a), _bits(b)), (str(lowp), what)
        assert sh is None or not bool(sh.view(torch.int16).any()), "the shadow was written"
        assert ema.bands_intact()
    flag.zero_()  # control: with the flag down the same call does step
    w, _, _, _, ema, _ = _run(inp, n, None, True, dev_form, ema_on=True, skip=flag.data_ptr())
    assert not torch.equal(w, inp["w"]) and not torch.equal(ema.view, inp["e"])


@pytest.mark.parametrize("n,off", [(n, 0) for n in SIZES] + [(1023, 1), ((1 << 21) + 5, 1)],
                         ids=[f"n{n}" for n in SIZES] + ["n1023_misaligned", "n2097157_misaligned"])
def test_swap_is_an_exact_exchange(gpu, n, off):
    """off = 1: the first range starts 4 bytes past a 16-byte boundary, the second on one - the scalar path."""
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    gen = torch.Generator(device="cuda").manual_seed(n + off)
    x, y = torch.randn(n, generator=gen, device="cuda"), torch.randn(n, generator=gen, device="cuda")
    if n > 8:  # bit patterns a float move must not touch
        x[1], x[2], y[3], y[4] = float("inf"), -0.0, 1e-42, float("-inf")
    a, b = Guarded(x, n, off), Guarded(y, n)
    assert a.ptr % 16 == 4 * off and b.ptr % 16 == 0
    _lib.call("d2r_swap_f32", a.ptr, b.ptr, n, _stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.view), _bits(y)) and torch.equal(_bits(b.view), _bits(x))
    assert a.bands_intact() and b.bands_intact()
    _lib.call("d2r_swap_f32", a.ptr, b.ptr, n, _stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.view), _bits(x)) and torch.equal(_bits(b.view), _bits(y)), "swapping twice is not the identity"
    assert a.bands_intact() and b.bands_intact()


# ---- the optimiser on the tiny model (1 + 1 encoder layers, 64 x 64 images) -----------------------------------------------
def _tiny(dtype):
    from d2r_amd import modules as M
    from d2r_amd.config import TextConfig, VisionConfig, default_args
    tc = TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)
    args = default_args(DR_step=3, compute_dtype=dtype, device="cuda:0", num_epochs=1, batch_size=4, warmup_ratio=0.0,
                        save_path=None, lr=1e-4)
    return M.UnimoModelF(args, vc, tc), args


_STORES = {}


def _store(gpu, dtype):
    """One tiny ParamStore per dtype for the whole module (tests restore flat_w from w0 before they step)."""
    if dtype not in _STORES:
        from d2r_amd.params import ParamStore
        torch.manual_seed(21)
        model, _ = _tiny(dtype)
        model.to(gpu).train()
        model.set_compute_dtype(dtype)
        store = ParamStore(model, dtype)
        mask = torch.zeros(store.n, dtype=torch.bool)
        for _, _, o, k, _ in store.entries:
            mask[o:o + k] = True
        gen = torch.Generator().manual_seed(9)  # gradients over the live elements (alignment padding stays 0)
        grads = [(torch.randn(store.n, generator=gen) * 1e-3 * mask).to(gpu) for _ in range(4)]
        _STORES[dtype] = (model, store, store.flat_w.clone(), grads)
    model, store, w0, grads = _STORES[dtype]
    store.flat_w.copy_(w0)
    store.refresh_lowp()
    return store, w0, grads


def test_constructor_refuses_a_bad_decay_and_allocates_nothing_when_off(gpu):
    from d2r_amd.params import FusedAdamW
    store, _, _ = _store(gpu, torch.bfloat16)
    for bad in (1.0, -0.5, 2.0):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(store, lr=1e-3, ema_decay=bad)
    for off in (None, 0, 0.0):
        opt = FusedAdamW(store, lr=1e-3, ema_decay=off)
        assert opt.ema is None and opt.ema_decay is None
        with opt.ema_weights():  # a no-op
            pass
    opt = FusedAdamW(store, lr=1e-3, ema_decay=0.9)
    assert opt.ema.shape == store.flat_w.shape and opt.ema.dtype == torch.float32
    torch.cuda.synchronize()
    assert torch.equal(opt.ema, store.flat_w)  # seeded
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="already active"):
            with opt.ema_weights():
                pass


@pytest.mark.parametrize("dtype,mgn", [(torch.bfloat16, None), (torch.float16, None), (torch.bfloat16, 0.01)],
                         ids=["bf16", "fp16", "bf16_clip"])
def test_off_means_off(gpu, dtype, mgn):
    """Three steps with ema_decay=None and with 0.99 leave w, m, v and the shadow bit-identical to each other; the average itself
    follows the schedule (checked against the recurrence in fp64 with the derived bound of the kernel test)."""
    from d2r_amd.params import FusedAdamW, ema_one_minus_decay
    runs = []
    for decay in (None, 0.99):
        store, w0, grads = _store(gpu, dtype)
        opt = FusedAdamW(store, lr=1e-3, max_grad_norm=mgn, ema_decay=decay)
        if dtype == torch.float16:
            opt.enable_loss_scaling(init_scale=2.0 ** 10)
        trail = []
        for G in grads[:3]:
            store.flat_g.copy_(G * opt.loss_scale)
            opt.step()
            trail.append(store.flat_w.clone())
        torch.cuda.synchronize()
        if mgn is not None:
            assert float(opt._clip["out"][1]) < 1.0  # clipping took part
        runs.append((store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone()))
    for what, a, b in zip(("w", "m", "v", "lp"), *runs):
        assert torch.equal(a, b), what
    assert not torch.equal(runs[0][0], w0)
    E, M = w0.double(), w0.abs().double()
    for t, W in enumerate(trail, start=1):
        E = E + float(np.float32(ema_one_minus_decay(0.99, t))) * (W.double() - E)
        M = torch.maximum(M, W.abs().double())
    assert bool(((opt.ema.double() - E).abs() <= 6.0 * 3 * 2.0 ** -24 * M * (1.0 + 2.0 ** -20)).all())
    assert not torch.equal(opt.ema, w0) and not torch.equal(opt.ema, runs[1][0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_graph_replay_with_ema_is_bit_identical_to_eager(gpu, dtype):
    """stage_hyper (which uploads 1 - d_t) + a captured step_captured against eager step() over three steps, with clipping on so
    that both optional operands are in the capture; in fp16 the second step overflows and is dropped, ema included."""
    from d2r_amd.params import FusedAdamW
    runs = []
    for graph in (False, True):
        store, w0, grads = _store(gpu, dtype)
        c = 0.5 * float(grads[0].double().norm())
        opt = FusedAdamW(store, lr=1e-3, max_grad_norm=c, ema_decay=0.9)
        if dtype == torch.float16:
            opt.enable_loss_scaling(init_scale=2.0 ** 12)
        if graph:
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                opt.step_captured()
        emas = []
        for t, G in enumerate(grads[:3]):
            G = G * opt.loss_scale
            if dtype == torch.float16 and t == 1:
                G[777] = float("inf")
            store.flat_g.copy_(G)
            if graph:
                opt.stage_hyper()
                cg.replay()
                opt.after_replay()
            else:
                opt.step()
            emas.append(opt.ema.clone())
        torch.cuda.synchronize()
        if dtype == torch.float16:
            opt._scaler_consume()
        runs.append((torch.stack(emas), store.flat_w.clone(), opt.m.clone(), opt.v.clone(), store.flat_lp.clone(), opt.step_count,
                     opt.loss_scale))
    for what, a, b in zip(("ema", "w", "m", "v", "lp"), runs[0][:5], runs[1][:5]):
        assert torch.equal(a, b), what
    assert runs[0][5:] == runs[1][5:]
    emas = runs[0][0]
    assert not torch.equal(emas[0], w0) and not torch.equal(emas[2], emas[0])
    if dtype == torch.float16:
        assert torch.equal(emas[1], emas[0]), "the overflowed step moved ema"
        assert runs[0][5] == 2  # the dropped step does not count


def test_sharded_capture_with_ema_stays_refused(gpu):
    from d2r_amd.params import FusedAdamW
    store, _, _ = _store(gpu, torch.float16)
    opt = FusedAdamW(store, lr=1e-3, ema_decay=0.9)
    opt.enable_loss_scaling()
    opt.element_ranges = [(0, store.n)]
    with pytest.raises(RuntimeError, match="sharded"):
        opt.step_captured()


def test_state_dict_carries_ema_and_a_state_without_it_reseeds(gpu):
    from d2r_amd.params import FusedAdamW
    store, w0, grads = _store(gpu, torch.bfloat16)
    opt = FusedAdamW(store, lr=1e-3, ema_decay=0.9)
    store.flat_g.copy_(grads[0])
    opt.step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert torch.equal(sd["ema"], opt.ema) and not torch.equal(sd["ema"], store.flat_w)
    opt2 = FusedAdamW(store, lr=1e-3, ema_decay=0.9)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.ema, sd["ema"]) and opt2.step_count == 1
    del sd["ema"]
    opt2.load_state_dict(sd)
    torch.cuda.synchronize()
    assert torch.equal(opt2.ema, store.flat_w)
    assert "ema" not in FusedAdamW(store, lr=1e-3).state_dict()


def test_trainer_evaluates_and_saves_the_averaged_weights(gpu, tmp_path):
    from d2r_amd.data import SyntheticMSDDataset, make_loader
    from d2r_amd.train import MSDTrainer
    torch.manual_seed(0)
    model, args = _tiny(torch.bfloat16)
    args.save_path = str(tmp_path) + "/"
    args.ema_decay = 0.5
    mk = lambda n, seed, sh: make_loader(SyntheticMSDDataset(n, 16, 64, 3, seed=seed, num_image_tokens=5), 4, sh, 0, drop_last=sh)
    lines = []
    logger = logging.getLogger("ema-trainer-test")

    class Catch(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())

    logger.addHandler(Catch())
    logger.setLevel(logging.INFO)
    tr = MSDTrainer(train_data=mk(16, 1, True), dev_data=mk(8, 2, False), test_data=None, model=model, args=args, logger=logger,
                    writer=None)
    tr.train(None, None)  # four steps, then evaluate(1) from inside
    opt, store = tr.optimizer, tr.store
    assert opt.step_count == 4 and opt.ema is not None
    assert any("Weight EMA" in l and "0.5" in l and str(4 * store.n) in l for l in lines), lines[:12]
    torch.cuda.synchronize()
    before = (store.flat_w.clone(), store.flat_lp.clone(), opt.ema.clone())
    tr.best_dev_metric = 0  # so that this evaluation saves whatever its score
    res = tr.evaluate(1)
    torch.cuda.synchronize()
    assert 0.0 <= res["eval_accuracy"] <= 1.0
    for what, a, b in zip(("flat_w", "flat_lp", "ema"), before, (store.flat_w, store.flat_lp, opt.ema)):
        assert torch.equal(_bits(a), _bits(b)), f"evaluate() changed {what}"
    saved = torch.load(os.path.join(str(tmp_path), "best_model.pth"), map_location=gpu)
    differs = 0
    for name, p, o, k, _ in store.entries:
        assert torch.equal(_bits(saved[name].reshape(-1)), _bits(opt.ema[o:o + k])), name
        differs += int(not torch.equal(saved[name].reshape(-1), store.flat_w[o:o + k]))
    assert differs > 0, "the checkpoint holds the live weights"
    for name, p in store.dead:  # untouched by the optimiser, saved as they are
        assert torch.equal(saved[name], p.detach()), name
    model2, _ = _tiny(torch.bfloat16)
    model2.load_state_dict(saved, strict=True)  # every key of the model, nothing else: what --only_test --load_path does
    assert set(saved) == set(model2.state_dict())
    # test() without a checkpoint to load runs on the averaged weights through the swap and puts the live ones back
    tr.test_data, args.load_path = mk(8, 3, False), None
    tr.test(1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(store.flat_w), _bits(before[0])) and torch.equal(_bits(store.flat_lp), _bits(before[1]))


def test_cli_logs_the_ema_line_and_refuses_a_decay_of_one(gpu, tmp_path):
    common = ["--num_epochs", "1", "--train_samples", "16", "--eval_samples", "8", "--batch_size", "8", "--encoder_layers", "1",
              "--image_size", "64", "--max_seq", "16", "--num_workers", "0", "--save_path", str(tmp_path) + "/", "--dtype", "bf16"]
    r = subprocess.run([sys.executable, "-m", "d2r_amd.run", "--ema_decay", "1.0", *common], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--ema_decay" in r.stderr and "Running training" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "d2r_amd.run", "--ema_decay", "0.99", *common], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Weight EMA: decay 0.99" in r.stderr, r.stderr[-3000:]
    assert "Test Eval results" in r.stderr and os.path.exists(os.path.join(str(tmp_path), "best_model.pth"))


def test_two_ranks_sharded_ema_equals_one_rank(gpu, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "probes", "dp_ema_two_ranks.py"), str(tmp_path)]
    proc = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True,
                            env=dict(os.environ, D2R_PROBE_DUMP_S="150"))
    try:
        out, err = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        out, err = proc.communicate()
        pytest.fail("the two ranks did not finish in 300 s: hang.\n--- stdout\n" + out[-3000:] + "\n--- stderr\n" + err[-6000:])
    assert proc.returncode == 0, "two-rank EMA probe failed\n--- stdout\n" + out[-3000:] + "\n--- stderr\n" + err[-6000:]
    res = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in (0, 1)]
    for r in res:
        assert r["finite"] and r["moved"], r
        assert 0 < r["owned"] < r["n"] and r["stale_differs"], ("each rank must own a part only, or the gather is not exercised", r)
        for key in ("same_w_as_one_rank", "gathered_is_one_rank_ema", "same_ranks", "swapped_in_is_one_rank_ema", "lp_follows_swap",
                    "live_w_restored", "live_lp_restored", "state_dict_ema"):
            assert r[key], (key, r)
