"""The batched operand fetch of the 16-bit pack epilogue (d2r_amd/csrc/gemm_args.h epilogue_fetch; gemm_glds.hip, gemm8.hip), through the
raw descriptor, EXACTLY.

The LDS-DMA kernels load a lane's packs of G (gradient reference), R (residual) and the old C (beta != 0) in one batch in front of the
rolled pack loop, from addresses clamped into the operand, and fetch the bias before the K-loop.  What can go wrong is an operand pack
of the wrong row, column tile or slot, a clamped value that is used, or a fetch outside the operand.  Every intermediate of these cases is
exactly representable, so the result must EQUAL the fp64 expression, no bound:

    A [M, K]: row m is +-1 where k % (K / 16) == m % (K / 16), else 0 (16 terms per row, some in every K-tile);  B in {-1, 0, 1}
    => |A B| <= 16;  bias, R, old C integers in [-3, 3];  G in {0, +-0.5, +-1} (relu' in {0, 1}, tanh' = 1 - G^2 in {0, 0.75, 1})
    => every value is a multiple of 1/4 below 32: seven significant bits, exact in bf16 (8) and fp16 (11) and in the fp32 arithmetic.

Shapes: the smallest at which the batch can go wrong - M = 200, N = 136 for the 128-wide kernels (a second row tile with rows past M,
a last column tile with a single valid pack), M = 300, N = 264 for the 256-wide kernel; ldc > N, ldr != ldc.  K = 128 and 192: two and
three K-tiles.  K = 64 is run as well, but the dispatcher gives a single K-tile to the generic kernel whatever tile code is forced
(gemm.hip: the LDS-DMA kernels need K >= 128), so that case asserts variant 0 and the same exact result.  The in-launch split-K kernel
needs K >= 6144.  C and P are surrounded by NaN patterns (ldc padding, two extra rows) that must come back bit-identical, P and (with
beta = 0) C start as NaN, and every case runs twice and must equal itself.

GELU and quick-GELU (forward with P, gradient with G) cannot be exact: they run on random 16-bit operands through run_case of
test_gpu_gemm_paths.py, against fp64 within the per-element bound stated there."""
import ctypes as C
import functools

import pytest
import torch

from test_gpu_gemm_paths import (BF, GELU, H, LOWP, LOWP_IDS, NN, NONE, NT, QGELU, RELU, TANH, _bits, _code, _nan_like, _restore_tuning,
                                 _timer_families, case, run_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_tuning(gpu):
    """d2r_gemm_tuning state is process-global: every test starts and ends on the defaults."""
    _restore_tuning()
    yield
    _restore_tuning()


OPSETS = {
    "none": dict(),
    "bias": dict(bias=True),
    "R": dict(res=True),
    "beta1": dict(beta=1.0),
    "P_relu": dict(pre=True, act=RELU),
    "G_relu": dict(gact=RELU),
    "G_tanh_R_beta1": dict(gact=TANH, res=True, beta=1.0),
}
# (name, d2r_gemm_tuning tile code, kernel variant of the launch timer, M, N)
KERNELS = [("128x128w8", 6, 3, 200, 136), ("128x64", 5, 1, 200, 136), ("256x256", 11, 8, 300, 264)]
LAYOUTS = [(NT, "NT"), (NN, "NN")]


@functools.lru_cache(maxsize=None)
def _operands(layout, M, N, K, seed=0):
    """fp64 operands of one problem and its product, made once and shared (never modified) by every case of the shape."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K + layout)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).double()

    stride = max(K // 16, 1)
    k, m = torch.arange(K)[None, :], torch.arange(M)[:, None]
    A = torch.where(k % stride == m % stride, ints((M, K), 0, 1) * 2 - 1, torch.zeros(M, K, dtype=torch.float64))
    B = ints((K, N), -1, 1)
    o = dict(A=A, B=B, acc=A @ B, bias=ints((N,), -3, 3), R=ints((M, N), -3, 3), Cold=ints((M, N), -3, 3), G=ints((M, N), -2, 2) * 0.5)
    assert float(o["acc"].abs().max()) <= 16
    return o


def _expected(o, ops):
    v = o["acc"] + (o["bias"] if ops.get("bias") else 0.0)
    out = v.clamp_min(0.0) if ops.get("act", NONE) == RELU else v
    if ops.get("gact") == RELU:
        out = out * (o["G"] > 0).double()
    elif ops.get("gact") == TANH:
        out = out * (1.0 - o["G"] * o["G"])
    if ops.get("res"):
        out = out + o["R"]
    if ops.get("beta"):
        out = out + ops["beta"] * o["Cold"]
    return v, out


class Problem:
    """Device buffers and the descriptor of one exact problem; C and P sit in NaN-filled [M + 2, ldc] buffers."""

    def __init__(self, gpu, dt, layout, M, N, K, ops, seed=0, ws=None):
        from d2r_amd import _lib
        self.o, self.ops, self.dt, self.M, self.N = _operands(layout, M, N, K, seed), ops, dt, M, N
        o = self.o
        self.ldc, self.ldr = N + 16, N + 8
        self.A = o["A"].to(dt).to(gpu)
        self.B = (o["B"].t().contiguous() if layout == NT else o["B"]).to(dt).to(gpu)
        self.c_init = _nan_like((M + 2) * self.ldc, dt, "cpu").view(M + 2, self.ldc).clone()
        if ops.get("beta"):
            self.c_init[:M, :N] = o["Cold"].to(dt)
        self.Cg = self.c_init.to(gpu)
        self.Pg = _nan_like((M + 2) * self.ldc, dt, gpu).view(M + 2, self.ldc) if ops.get("pre") else None
        self.Rg = torch.zeros(M, self.ldr, dtype=dt)
        self.Rg[:, :N] = o["R"].to(dt)
        self.Rg = self.Rg.to(gpu) if ops.get("res") else None
        self.Gg = None
        if ops.get("gact"):
            g = torch.zeros(M, self.ldc, dtype=dt)
            g[:, :N] = o["G"].to(dt)
            self.Gg = g.to(gpu)
        self.biasg = o["bias"].float().to(gpu) if ops.get("bias") else None
        self.d = _lib.GemmDesc(dtype=_code(dt), c_dtype=_code(dt), layout=layout, act=ops.get("act", NONE), M=M, N=N, K=K, nb=1, nh=1, alpha=1.0,
                               beta=ops.get("beta", 0.0), A=self.A.data_ptr(), lda=K, B=self.B.data_ptr(), ldb=self.B.shape[1],
                               C=self.Cg.data_ptr(), ldc=self.ldc, bias=None if self.biasg is None else self.biasg.data_ptr(),
                               residual=None if self.Rg is None else self.Rg.data_ptr(), ldr=self.ldr if self.Rg is not None else 0,
                               preact=None if self.Pg is None else self.Pg.data_ptr())
        if self.Gg is not None:
            self.d.grad_ref, self.d.grad_act = self.Gg.data_ptr(), ops["gact"]
        if ws is not None:
            self.d.workspace, self.d.workspace_bytes = ws.data_ptr(), ws.numel()

    def reset(self):
        self.Cg.copy_(self.c_init)
        if self.Pg is not None:
            self.Pg.copy_(_nan_like(self.Pg.numel(), self.dt, self.Pg.device).view_as(self.Pg))

    def outputs(self):
        return [t.clone() for t in (self.Cg, self.Pg) if t is not None]

    def check(self, what):
        M, N = self.M, self.N
        v, out = _expected(self.o, self.ops)
        got = self.Cg.cpu()
        assert torch.equal(got[:M, :N].double(), out), f"{what}: C differs from the exact result in {int((got[:M, :N].double() != out).sum())} elements"
        nan = _nan_like(got.numel(), self.dt, "cpu").view_as(got)
        assert torch.equal(_bits(got[:M, N:]), _bits(nan[:M, N:])) and torch.equal(_bits(got[M:]), _bits(nan[M:])), f"{what}: C written outside the output"
        if self.Pg is not None:
            p = self.Pg.cpu()
            assert torch.equal(p[:M, :N].double(), v), f"{what}: preact differs from A B + bias"
            assert torch.equal(_bits(p[:M, N:]), _bits(nan[:M, N:])) and torch.equal(_bits(p[M:]), _bits(nan[M:])), f"{what}: preact written outside"


def _launch_twice(probs, launch, expect, nlaunch=1):
    from d2r_amd import _lib
    lib = _lib.load()
    runs = []
    for _ in range(2):
        for p in probs:
            p.reset()
        lib.d2r_gemm_timer(1)
        try:
            launch()
        finally:
            fams = _timer_families()
            lib.d2r_gemm_timer(0)
        torch.cuda.synchronize()
        assert len(fams) == nlaunch and all(f // 100 == expect for f in fams), f"expected {nlaunch} launch(es) of kernel variant {expect}, the launch timer says {fams}"
        runs.append([t for p in probs for t in p.outputs()])
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y)), "two launches of the same case differ"


CASES = [(kn, tile, var, M, N, lay, ln, K, on) for kn, tile, var, M, N in KERNELS for lay, ln in LAYOUTS for K in (64, 128, 192) for on in OPSETS]


@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
@pytest.mark.parametrize("kn,tile,var,M,N,lay,ln,K,on", CASES, ids=["%s-%s-K%d-%s" % (c[0], c[6], c[7], c[8]) for c in CASES])
def test_pack_epilogue_operands_exact(gpu, dt, kn, tile, var, M, N, lay, ln, K, on):
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    p = Problem(gpu, dt, lay, M, N, K, OPSETS[on])
    _lib.load().d2r_gemm_tuning(1, 1, tile)
    # a single K-tile is below the LDS-DMA kernels' K >= 128: the generic tiled kernel (variant 0) serves it, with the same exact result
    _launch_twice([p], lambda: _lib.call("d2r_gemm", C.byref(p.d), _stream()), var if K >= 128 else 0)
    p.check(f"{kn} {ln} K={K} {on}")


@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
@pytest.mark.parametrize("lay,ln", LAYOUTS, ids=[x[1] for x in LAYOUTS])
@pytest.mark.parametrize("K", [128, 192])
def test_grouped_forward_launch_one_problem_with_R_one_with_G(gpu, dt, lay, ln, K):
    """d2r_gemm_group: two independent problems in ONE launch of the 128 x 128 eight-wave tiles, the first with a residual only, the
    second with a gradient reference only - the operand pointers are per problem, a batch fetched from the neighbour's shows at once."""
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    probs = [Problem(gpu, dt, lay, 200, 136, K, dict(res=True), seed=1), Problem(gpu, dt, lay, 200, 136, K, dict(gact=RELU), seed=2)]
    descs = (_lib.GemmDesc * 2)(probs[0].d, probs[1].d)
    _launch_twice(probs, lambda: _lib.call("d2r_gemm_group", descs, 2, _stream()), 3)
    for i, p in enumerate(probs):
        p.check(f"grouped {ln} K={K} problem {i}")


@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
@pytest.mark.parametrize("lay,ln", LAYOUTS, ids=[x[1] for x in LAYOUTS])
@pytest.mark.parametrize("on", ["bias", "G_tanh_R_beta1"])
def test_in_launch_splitk_operands_exact(gpu, dt, lay, ln, on):
    """The in-launch split-K kernel (K >= 6144 over few tiles, workspace given): only the finishing workgroup of a tile runs the
    epilogue, with the bias it fetched before its K-loop and the batch it fetches after the partial sums have met."""
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    ws = torch.zeros(16 << 20, dtype=torch.uint8, device=gpu)
    p = Problem(gpu, dt, lay, 200, 136, 6144, OPSETS[on], ws=ws)
    _launch_twice([p], lambda: _lib.call("d2r_gemm", C.byref(p.d), _stream()), 3)
    assert bool(ws.any()), "no partial sums in the workspace: the launch was not split"
    p.check(f"split-K {ln} {on}")


GELU_CASES = [(kn, tile, var, M, N, lay, ln, act) for kn, tile, var, M, N in KERNELS for lay, ln in LAYOUTS[:1] for act in (GELU, QGELU)]


@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
@pytest.mark.parametrize("kn,tile,var,M,N,lay,ln,act", GELU_CASES, ids=["%s-%s-act%d" % (c[0], c[6], c[7]) for c in GELU_CASES])
def test_gelu_forward_and_gradient_within_the_stated_bound(gpu, dt, kn, tile, var, M, N, lay, ln, act):
    run_case(gpu, case(var, dt=dt, layout=lay, M=M, N=N, K=128, bias=True, act=act, pre=True, tune=(tile,)))
    run_case(gpu, case(var, dt=dt, layout=NN, M=M, N=N, K=128, gact=act, tune=(tile,)))
