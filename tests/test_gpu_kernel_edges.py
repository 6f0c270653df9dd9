"""Edge-case parity of the small kernels (rowops.hip, misc.hip, elementwise.hip) on every dispatch path, against plain fp64 CPU
expressions of the same operations.  Every output lives inside a larger allocation whose other elements (before, after, and in the
ld gap between rows) hold a sentinel bit pattern; each test asserts that the sentinels are bit-for-bit unchanged.

Branch                                                        Test
------------------------------------------------------------  ---------------------------------------------------------------
LayerNorm fwd/bwd, D = VEC .. max, rows 1 .. 9000             test_layernorm[*]
  bwd row walk (> 2048 rows, prefetched next row)             test_layernorm[*-2049|6304|9000], test_layernorm_bwd_dres_accumulate
  MAXP = 4 (16-bit D > 1024, fp32 bwd D > 768)                test_layernorm[bf16|fp16-1032|2048-*], test_layernorm[fp32-772|1024-*]
  large offset / var << eps (eps 1e-12 and 1e-5)              test_layernorm_conditioning[*]
  dres add, accumulate = 1                                    test_layernorm_bwd_dres_accumulate[*]
  deferred partials + sum_grouped, n = 1, 2, 33 (chunk of 32) test_layernorm_deferred_sum_grouped[*]
l2norm fwd/bwd, same D set, zero row, large / tiny fp16 rows  test_l2norm[*], test_l2norm_zero_and_extreme_rows[*]
softmax MAXPL = 4 / 10 / 32, five fwd pairs, ld > cols,       test_softmax_fwd[*]
  scale 100/sqrt(768), -10000 mask with rows_per_mask = 12
softmax bwd, five pairs, ld > cols                            test_softmax_bwd[*]
softmax in-place forward                                      test_softmax_fwd_in_place[*]
host-side refusals (D % VEC, D > max, cols 0 / 2049, align)   test_refusals
js_div rows-per-wave (B > 16), cols-per-lane (B > 64),        test_jsdiv[*]
  probabilities that underflow to exactly 0
  regression: (p + q) / 2 underflowing to 0 gave inf         test_jsdiv_mid_probability_underflow
cross entropy thread loop (B > 256), multi-block bwd, C = 7   test_cross_entropy[*]
Block merge S > 64, all-zero chunk (clamp), z == 0 entries    test_block_merge[*]
SAF gate _ex: B*n > 1024, n > 64, train / eval, w16 / da16    test_saf_gate_ex[*]
  copies vs d2r_cast, accumulate = 1
SAF gate global-batch-exact split (stats, gstats, phase 1/2)  test_saf_gate_global_batch_split
elementwise ops, scalar tail, misaligned operands,            test_elementwise[*]
  grid-stride beyond 2048 blocks
axpby beta = 0 (NaN in y must not leak) and beta != 0         test_axpby[*]
d2r_cast: seven pairs, ties, fp16 overflow, NaN, subnormals   test_cast[*]
dropout: vector and scalar paths keep the same elements       test_dropout_paths_keep_the_same_elements[*]
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_kernels import check, rnd

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}
PAD = 64  # guard elements before and after every buffer (keeps the inner tensor 16-byte aligned for every dtype)

# sentinel bit patterns: a NaN in fp32 / fp16 / fp64, a huge finite value in bf16
_SENT = {torch.float32: (torch.int32, 0x7FB1C2D3), torch.bfloat16: (torch.int16, 0x7DB5), torch.float16: (torch.int16, 0x7DB5),
         torch.float64: (torch.int64, 0x7FF4A5A5A5A5A5A5), torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A)}


def _lib():
    from d2r_amd import _lib as L
    return L


def _st():
    from d2r_amd import functional as F
    return F._stream()


def call(name, *args):
    _lib().call(name, *args)


class Guarded:
    """A [rows, cols] device tensor with row pitch `ld`, `shift` elements past a 16-byte boundary, inside an allocation whose
    every other element (PAD before, PAD after, the ld gap) holds a sentinel bit pattern.  The inner elements start as the
    sentinel too, so an element the kernel forgets to write fails the value comparison."""

    def __init__(self, gpu, dtype, rows, cols=None, ld=None, shift=0, fill=None):
        flat = cols is None
        cols = rows if flat else cols
        rows = 1 if flat else rows
        ld = cols if ld is None else ld
        self.it, self.sent = _SENT[dtype]
        start = PAD + shift
        total = start + rows * ld + PAD
        self.buf = torch.empty(total, dtype=dtype, device=gpu)
        self.buf.view(self.it).fill_(self.sent)
        inner = self.buf[start:start + rows * ld].view(rows, ld)[:, :cols]
        self.t = inner.reshape(-1) if flat else inner
        inside = torch.zeros(total, dtype=torch.bool, device=gpu)
        inside[start:start + rows * ld].view(rows, ld)[:, :cols] = True
        self.outside = ~inside
        if fill is not None:
            self.t.copy_(fill.reshape(self.t.shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self, name):
        bits = self.buf.view(self.it)[self.outside]
        bad = int((bits != self.sent).sum())
        assert bad == 0, f"{name}: {bad} guard element(s) around the tensor were overwritten"


def dev(x, dtype, gpu):
    return x.to(dtype).to(gpu)


def f64(t):
    return t.detach().cpu().double()


# ================================================================================================================================
# 1. Row kernels
# ================================================================================================================================
def ln_ref(x, g, b, eps, dy):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rs
    y = xh * g + b
    gd = dy * g
    dx = rs * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    return y, mu[:, 0], rs[:, 0], dx, (dy * xh).sum(0), dy.sum(0)


def ln_widths(dtype):
    v = VEC[dtype]
    return [v, 64, 768, 772, 1024] if dtype == torch.float32 else [v, 64, 768, 1024, 1032, 2048]


LN_CASES = [(dt, D, rows) for dt in DT for D in ln_widths(dt) for rows in (1, 3, 5, 2047, 2049)]
LN_CASES += [(dt, D, rows) for dt in DT for D in (768, ln_widths(dt)[-1]) for rows in (6304, 9000)]


def ln_params(D, seed=0):
    gamma = 1.0 + 0.2 * rnd(D, seed=seed + 1)
    beta = 0.1 * rnd(D, seed=seed + 2)
    return gamma, beta


def ln_fwd_gpu(gpu, dtype, x, gamma, beta, eps):
    rows, D = x.shape
    Y, mean, rstd = Guarded(gpu, dtype, rows, D), Guarded(gpu, torch.float32, rows), Guarded(gpu, torch.float32, rows)
    call("d2r_layernorm_fwd", CODE[dtype], x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, rows, D, Y.ptr, mean.ptr, rstd.ptr,
         _st())
    return Y, mean, rstd


def ln_ws(rows, D, gpu):
    return torch.empty(_lib().load().d2r_layernorm_bwd_workspace(rows, D), dtype=torch.uint8, device=gpu)


def ln_bwd_gpu(gpu, dtype, dy, x, gamma, mean, rstd, dres=None, dg_init=None, db_init=None, accumulate=0, ws=None):
    rows, D = x.shape
    dX = Guarded(gpu, dtype, rows, D)
    dG = Guarded(gpu, torch.float32, D, fill=dg_init)
    dB = Guarded(gpu, torch.float32, D, fill=db_init)
    ws = ln_ws(rows, D, gpu) if ws is None else ws
    call("d2r_layernorm_bwd_ex", CODE[dtype], dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean, rstd, rows, D, dX.ptr,
         None if dres is None else dres.data_ptr(), dG.ptr, dB.ptr, accumulate, ws.data_ptr(), ws.numel(), _st())
    return dX, dG, dB


def ln_case(gpu, dtype, x32, gamma, beta, eps, dy32, yloosen=1.0):
    """Forward + backward on the GPU against ln_ref in fp64; returns the GPU results."""
    rows, D = x32.shape
    x, dy = dev(x32, dtype, gpu), dev(dy32, dtype, gpu)
    g_d, b_d = gamma.to(gpu), beta.to(gpu)
    Y, mean, rstd = ln_fwd_gpu(gpu, dtype, x, g_d, b_d, eps)
    dX, dG, dB = ln_bwd_gpu(gpu, dtype, dy, x, g_d, mean.ptr, rstd.ptr, dg_init=torch.full((D,), 7.0), db_init=torch.full((D,), -7.0))
    torch.cuda.synchronize()
    y, mu, rs, dx, dg, db = ln_ref(f64(x), gamma.double(), beta.double(), eps, f64(dy))
    tag = f"layernorm[{DT_IDS[dtype]} D={D} rows={rows}]"
    for G, n in ((Y, "y"), (mean, "mean"), (rstd, "rstd"), (dX, "dx"), (dG, "dgamma"), (dB, "dbeta")):
        G.intact(f"{tag}.{n}")
    check(f"{tag}.y", Y.t, y, dtype, loosen=yloosen)
    check(f"{tag}.mean", mean.t, mu, torch.float32, scale=float(mu.abs().max()) + float(rs.reciprocal().max()))
    check(f"{tag}.rstd", rstd.t, rs, torch.float32, loosen=min(yloosen, 50.0))
    check(f"{tag}.dx", dX.t, dx, dtype, loosen=yloosen)
    # the parameter gradients are fp32 sums of exact products: fp32 accuracy whatever the compute dtype
    check(f"{tag}.dgamma", dG.t, dg, torch.float32, loosen=5.0 * yloosen)
    check(f"{tag}.dbeta", dB.t, db, torch.float32, loosen=5.0)
    return x, dy, g_d, Y, mean, rstd, dX, dG, dB


@pytest.mark.parametrize("dtype,D,rows", LN_CASES, ids=[f"{DT_IDS[c[0]]}-{c[1]}-{c[2]}" for c in LN_CASES])
def test_layernorm(gpu, dtype, D, rows):
    gamma, beta = ln_params(D)
    ln_case(gpu, dtype, rnd(rows, D, seed=3), gamma, beta, 1e-12, rnd(rows, D, seed=4))


COND_CASES = [(dt, D, kind, eps) for dt in DT for D in (768, ln_widths(dt)[-1]) for kind in ("offset", "flat") for eps in (1e-12, 1e-5)]


@pytest.mark.parametrize("dtype,D,kind,eps", COND_CASES, ids=[f"{DT_IDS[c[0]]}-{c[1]}-{c[2]}-{c[3]:g}" for c in COND_CASES])
def test_layernorm_conditioning(gpu, dtype, D, kind, eps):
    """Rows with a large common offset (a one-pass E[x^2] - E[x]^2 variance would cancel to garbage) and rows whose variance is far
    below eps: exactly constant rows (var = 0, y = beta) alternating with rows of tiny noise around 0."""
    rows = 2049
    gamma, beta = ln_params(D, seed=5)
    noise, dy, loosen = rnd(rows, D, seed=6), rnd(rows, D, seed=7), 1.0
    if kind == "offset":
        if dtype == torch.float32:
            x = 300.0 + 0.01 * noise
            # an fp32 mean of values near 300 is off by a few ulp(300) / sqrt(D) ~ 3e-5 = 3e-3 of the 0.01 spread; the
            # variance (two-pass) and rstd stay at fp32 accuracy, and a single-pass variance misses by 100 %
            loosen = 500.0
        else:
            x = 64.0 + noise
    else:
        tiny = 2.0 ** -22 if dtype == torch.float16 else 1e-8  # fp16: subnormal multiples of 2^-24, var ~ 6e-14
        x = tiny * noise
        x[0::2] = 3.0
        dy = 1e-3 * dy  # dx ~ rstd * dy = 1e6 * dy at eps = 1e-12: keep it inside fp16's range
    ln_case(gpu, dtype, x, gamma, beta, eps, dy, yloosen=loosen)


DRES_CASES = [(dt, D) for dt in DT for D in (VEC[dt], 768, ln_widths(dt)[-1])]


@pytest.mark.parametrize("dtype,D", DRES_CASES, ids=[f"{DT_IDS[c[0]]}-{c[1]}" for c in DRES_CASES])
def test_layernorm_bwd_dres_accumulate(gpu, dtype, D):
    """9000 rows (every wave walks >= 4 rows): dX += dres, and dgamma / dbeta added into pre-filled sinks."""
    rows = 9000
    gamma, beta = ln_params(D, seed=8)
    x, dy, dres = dev(rnd(rows, D, seed=9), dtype, gpu), dev(rnd(rows, D, seed=10), dtype, gpu), dev(rnd(rows, D, seed=11), dtype, gpu)
    g_d, b_d = gamma.to(gpu), beta.to(gpu)
    _, mean, rstd = ln_fwd_gpu(gpu, dtype, x, g_d, b_d, 1e-12)
    g0, b0 = 0.5 * rnd(D, seed=12), 0.5 * rnd(D, seed=13)
    dX, dG, dB = ln_bwd_gpu(gpu, dtype, dy, x, g_d, mean.ptr, rstd.ptr, dres=dres, dg_init=g0, db_init=b0, accumulate=1)
    torch.cuda.synchronize()
    _, _, _, dx, dg, db = ln_ref(f64(x), gamma.double(), beta.double(), 1e-12, f64(dy))
    tag = f"layernorm_bwd_ex[{DT_IDS[dtype]} D={D}]"
    for G, n in ((dX, "dx"), (dG, "dgamma"), (dB, "dbeta")):
        G.intact(f"{tag}.{n}")
    check(f"{tag}.dx+dres", dX.t, dx + f64(dres), dtype)
    check(f"{tag}.dgamma+=", dG.t, dg + g0.double(), torch.float32, loosen=5.0)
    check(f"{tag}.dbeta+=", dB.t, db + b0.double(), torch.float32, loosen=5.0)


GROUP_CASES = [(dt, D, n) for dt in DT for (D, n) in ((ln_widths(dt)[-1], 1), (ln_widths(dt)[-1], 2), (768, 33))]


@pytest.mark.parametrize("dtype,D,n", GROUP_CASES, ids=[f"{DT_IDS[c[0]]}-{c[1]}-n{c[2]}" for c in GROUP_CASES])
def test_layernorm_deferred_sum_grouped(gpu, dtype, D, n):
    """null dgamma / dbeta defers the second stage; d2r_layernorm_bwd_sum_grouped over n problems (33 crosses the 32-problem
    chunk) equals the undeferred sum bit for bit (overwriting and accumulating) and fp64."""
    rows = 2049
    gamma, beta = ln_params(D, seed=14)
    x = dev(rnd(rows, D, seed=15), dtype, gpu)
    g_d, b_d = gamma.to(gpu), beta.to(gpu)
    _, mean, rstd = ln_fwd_gpu(gpu, dtype, x, g_d, b_d, 1e-12)
    dys = [dev(rnd(rows, D, seed=100 + i), dtype, gpu) for i in range(n)]
    wss, dxs, direct = [], [], []
    for dy in dys:
        ws = ln_ws(rows, D, gpu)
        dX = Guarded(gpu, dtype, rows, D)
        call("d2r_layernorm_bwd_ex", CODE[dtype], dy.data_ptr(), x.data_ptr(), g_d.data_ptr(), mean.ptr, rstd.ptr, rows, D, dX.ptr, None,
             None, None, 0, ws.data_ptr(), ws.numel(), _st())
        wss.append(ws)
        dxs.append(dX)
        direct.append(ln_bwd_gpu(gpu, dtype, dy, x, g_d, mean.ptr, rstd.ptr))
    from d2r_amd.functional import _parr
    pre_g = [0.25 * rnd(D, seed=200 + i) for i in range(n)]
    pre_b = [0.25 * rnd(D, seed=300 + i) for i in range(n)]
    results = {}
    for acc in (0, 1):
        dG = [Guarded(gpu, torch.float32, D, fill=pre_g[i] if acc else torch.full((D,), 9.0)) for i in range(n)]
        dB = [Guarded(gpu, torch.float32, D, fill=pre_b[i] if acc else torch.full((D,), -9.0)) for i in range(n)]
        call("d2r_layernorm_bwd_sum_grouped", _parr(wss), _parr([g.t for g in dG]), _parr([b.t for b in dB]), n, rows, D, acc, _st())
        results[acc] = (dG, dB)
    torch.cuda.synchronize()
    xh_ref = ln_ref(f64(x), gamma.double(), beta.double(), 1e-12, f64(dys[0]))
    mu, rs = xh_ref[1][:, None], xh_ref[2][:, None]
    xh = (f64(x) - mu) * rs
    tag = f"sum_grouped[{DT_IDS[dtype]} D={D} n={n}]"
    for i in range(n):
        ddX, ddG, ddB = direct[i]
        dxs[i].intact(f"{tag}.dx{i}")
        assert torch.equal(dxs[i].t, ddX.t), f"{tag}: deferred dx of problem {i} differs from the undeferred call"
        for acc in (0, 1):
            G, B_ = results[acc][0][i], results[acc][1][i]
            G.intact(f"{tag}.dgamma{i}")
            B_.intact(f"{tag}.dbeta{i}")
            eg = ddG.t + pre_g[i].to(gpu) if acc else ddG.t
            eb = ddB.t + pre_b[i].to(gpu) if acc else ddB.t
            assert torch.equal(G.t, eg), f"{tag}: dgamma of problem {i} (accumulate={acc}) is not bit-identical to the direct sum"
            assert torch.equal(B_.t, eb), f"{tag}: dbeta of problem {i} (accumulate={acc}) is not bit-identical to the direct sum"
        dy = f64(dys[i])
        check(f"{tag}.dgamma{i}", results[0][0][i].t, (dy * xh).sum(0), torch.float32, loosen=5.0)
        check(f"{tag}.dbeta{i}", results[0][1][i].t, dy.sum(0), torch.float32, loosen=5.0)


def l2_ref(x, dy):
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    a = 1.0 / (n + 1e-8)
    dot = (dy * x).sum(-1, keepdim=True)
    b = torch.where(n > 0, dot * a * a / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
    return x * a, n[:, 0], dy * a - x * b


def l2_gpu(gpu, dtype, x, dy):
    rows, D = x.shape
    Y, N, dX = Guarded(gpu, dtype, rows, D), Guarded(gpu, torch.float32, rows), Guarded(gpu, dtype, rows, D)
    call("d2r_l2norm_fwd", CODE[dtype], x.data_ptr(), Y.ptr, N.ptr, rows, D, _st())
    call("d2r_l2norm_bwd", CODE[dtype], dy.data_ptr(), x.data_ptr(), N.ptr, dX.ptr, rows, D, _st())
    torch.cuda.synchronize()
    for G, n in ((Y, "y"), (N, "norm"), (dX, "dx")):
        G.intact(f"l2norm[{DT_IDS[dtype]} D={D}].{n}")
    return Y, N, dX


L2_CASES = [(dt, D) for dt in DT for D in ln_widths(dt)]


@pytest.mark.parametrize("dtype,D", L2_CASES, ids=[f"{DT_IDS[c[0]]}-{c[1]}" for c in L2_CASES])
def test_l2norm(gpu, dtype, D):
    rows = 2049
    x, dy = dev(rnd(rows, D, seed=20), dtype, gpu), dev(rnd(rows, D, seed=21), dtype, gpu)
    Y, N, dX = l2_gpu(gpu, dtype, x, dy)
    y, n, dx = l2_ref(f64(x), f64(dy))
    tag = f"l2norm[{DT_IDS[dtype]} D={D}]"
    check(f"{tag}.y", Y.t, y, dtype)
    check(f"{tag}.norm", N.t, n, torch.float32)
    check(f"{tag}.dx", dX.t, dx, dtype)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_l2norm_zero_and_extreme_rows(gpu, dtype):
    """A zero row gives y = 0 and dx = dy / 1e-8 (the eps outside the root; no norm term); rows of large (fp16: |x| up to
    ~1e4, sum of squares far beyond fp16's range) and tiny (fp16 subnormal) magnitude are normalised in fp32."""
    D, rows = 768, 6
    x = rnd(rows, D, seed=22)
    big, small = (40.0, 2.0 ** -20) if dtype == torch.float16 else (1e15, 1e-15)
    x[0] = 0.0
    x[1] *= big
    x[2] *= small
    x[4] *= big
    dy = rnd(rows, D, seed=23)
    if dtype == torch.float16:  # dx = dy / (norm + 1e-8) must stay inside fp16's range
        dy[0] *= 1e-6
        dy[2] *= 0.1
    xg, dyg = dev(x, dtype, gpu), dev(dy, dtype, gpu)
    Y, N, dX = l2_gpu(gpu, dtype, xg, dyg)
    y, n, dx = l2_ref(f64(xg), f64(dyg))
    tag = f"l2norm extreme[{DT_IDS[dtype]}]"
    assert torch.equal(Y.t[0], torch.zeros_like(Y.t[0])) and float(N.t[0]) == 0.0, f"{tag}: a zero row must give y = 0, norm = 0"
    assert bool(torch.isfinite(dX.t.float()).all()), f"{tag}: non-finite gradient"
    check(f"{tag}.y", Y.t, y, dtype)
    for r in range(rows):
        check(f"{tag}.norm[{r}]", N.t[r], n[r], torch.float32)
        check(f"{tag}.dx[{r}]", dX.t[r], dx[r], dtype)


SM_COLS = [1, 2, 63, 64, 65, 197, 256, 257, 577, 640, 641, 768, 1500, 2048]
SM_FWD_PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.float32, torch.float16),
                (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)]
SM_BWD_PAIRS = [(torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float16, torch.float32),
                (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16)]
# (rows, ld - cols, scale, mask): few rows (a partly filled 4-row block) and a few thousand
SM_CFGS = [(1, 0, 1.0, False), (3, 7, 100 / math.sqrt(768), True), (4, 0, 100 / math.sqrt(768), False), (5, 7, 1.0, True),
           (2500, 7, 100 / math.sqrt(768), True)]


def pair_id(p):
    return f"{DT_IDS[p[0]]}-{DT_IDS[p[1]]}"


def sm_mask(rows, cols, seed):
    nm = (rows + 11) // 12
    m = torch.zeros(nm, cols)
    g = torch.Generator().manual_seed(seed)
    m[torch.rand(nm, cols, generator=g) < 0.3] = -10000.0
    m[:, 0] = 0.0  # a key mask keeps at least one key (a fully masked fp32 row is only defined to ulp(10000))
    return m


@pytest.mark.parametrize("cols", SM_COLS)
@pytest.mark.parametrize("pair", SM_FWD_PAIRS, ids=pair_id)
def test_softmax_fwd(gpu, pair, cols):
    tx, ty = pair
    for rows, gap, scale, use_mask in SM_CFGS:
        ld = cols + gap
        X = Guarded(gpu, tx, rows, cols, ld=ld, fill=rnd(rows, cols, seed=30).to(tx))
        Y = Guarded(gpu, ty, rows, cols, ld=ld)
        mask = sm_mask(rows, cols, 31) if use_mask else None
        md = mask.to(gpu) if use_mask else None
        call("d2r_softmax_fwd", CODE[tx], CODE[ty], X.ptr, Y.ptr, ld, rows, cols, scale, None if md is None else md.data_ptr(), 12, _st())
        torch.cuda.synchronize()
        tag = f"softmax_fwd[{pair_id(pair)} rows={rows} cols={cols} ld={ld} scale={scale:.3f} mask={use_mask}]"
        X.intact(tag + ".x")
        Y.intact(tag + ".y")
        s = scale * f64(X.t)
        if use_mask:
            s = s + mask.double().repeat_interleave(12, 0)[:rows]
        check(tag, Y.t, torch.softmax(s, -1), ty)


@pytest.mark.parametrize("cols", SM_COLS)
@pytest.mark.parametrize("pair", SM_BWD_PAIRS, ids=pair_id)
def test_softmax_bwd(gpu, pair, cols):
    tp, td = pair
    for rows, gap, scale, _ in SM_CFGS:
        ld = cols + gap
        p = torch.softmax(rnd(rows, cols, seed=32), -1)
        P = Guarded(gpu, tp, rows, cols, ld=ld, fill=p.to(tp))
        dP = Guarded(gpu, td, rows, cols, ld=ld, fill=rnd(rows, cols, seed=33).to(td))
        dS = Guarded(gpu, tp, rows, cols, ld=ld)
        call("d2r_softmax_bwd", CODE[tp], CODE[td], P.ptr, dP.ptr, dS.ptr, ld, rows, cols, scale, _st())
        torch.cuda.synchronize()
        tag = f"softmax_bwd[{pair_id(pair)} rows={rows} cols={cols} ld={ld} scale={scale:.3f}]"
        for G, n in ((P, "p"), (dP, "dp"), (dS, "ds")):
            G.intact(f"{tag}.{n}")
        pp, dd = f64(P.t), f64(dP.t)
        check(tag, dS.t, scale * pp * (dd - (dd * pp).sum(-1, keepdim=True)), tp)


@pytest.mark.parametrize("cols", [197, 577, 1500])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_softmax_fwd_in_place(gpu, dtype, cols):
    rows, ld, scale = 2500, cols + 7, 100 / math.sqrt(768)
    X = Guarded(gpu, dtype, rows, cols, ld=ld, fill=rnd(rows, cols, seed=34).to(dtype))
    s = scale * f64(X.t)
    mask = sm_mask(rows, cols, 35)
    md = mask.to(gpu)
    call("d2r_softmax_fwd", CODE[dtype], CODE[dtype], X.ptr, X.ptr, ld, rows, cols, scale, md.data_ptr(), 12, _st())
    torch.cuda.synchronize()
    tag = f"softmax in place[{DT_IDS[dtype]} cols={cols}]"
    X.intact(tag)
    check(tag, X.t, torch.softmax(s + mask.double().repeat_interleave(12, 0)[:rows], -1), dtype)


def test_refusals(gpu):
    """Arguments outside the documented range are refused on the host, before any launch, with a message naming the problem."""
    from d2r_amd._lib import D2RError
    st = _st()
    buf = torch.zeros(4 * 4096 + 64, dtype=torch.float32, device=gpu)
    gb = torch.zeros(4096, dtype=torch.float32, device=gpu)
    stat = torch.zeros(8, dtype=torch.float32, device=gpu)
    p = buf.data_ptr()
    for dtype, D in ((torch.float32, 6), (torch.bfloat16, 12), (torch.float16, 1028)):
        with pytest.raises(D2RError, match=f"D={D} unsupported"):
            call("d2r_layernorm_fwd", CODE[dtype], p, gb.data_ptr(), gb.data_ptr(), 1e-5, 2, D, p, stat.data_ptr(), stat.data_ptr(), st)
        with pytest.raises(D2RError, match=f"D={D} unsupported"):
            call("d2r_l2norm_fwd", CODE[dtype], p, p, stat.data_ptr(), 2, D, st)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    for dtype, D in ((torch.float32, 1028), (torch.bfloat16, 2056), (torch.float16, 4096)):
        with pytest.raises(D2RError, match=f"D={D} unsupported"):
            call("d2r_layernorm_fwd", CODE[dtype], p, gb.data_ptr(), gb.data_ptr(), 1e-5, 1, D, p, stat.data_ptr(), stat.data_ptr(), st)
        with pytest.raises(D2RError, match=f"D={D} unsupported"):
            call("d2r_layernorm_bwd_ex", CODE[dtype], p, p, gb.data_ptr(), stat.data_ptr(), stat.data_ptr(), 1, D, p, None, None, None, 0,
                 ws.data_ptr(), ws.numel(), st)
    for cols in (0, 2049):
        with pytest.raises(D2RError, match=f"cols={cols} outside"):
            call("d2r_softmax_fwd", 0, 0, p, p, 2100, 1, cols, 1.0, None, 1, st)
        with pytest.raises(D2RError, match=f"cols={cols} outside"):
            call("d2r_softmax_bwd", 0, 0, p, p, p, 2100, 1, cols, 1.0, st)
    with pytest.raises(D2RError, match="16-byte aligned"):
        call("d2r_layernorm_fwd", 0, p + 4, gb.data_ptr(), gb.data_ptr(), 1e-5, 1, 768, p + 4096 * 4, stat.data_ptr(), stat.data_ptr(), st)
    with pytest.raises(D2RError, match="16-byte aligned"):
        call("d2r_layernorm_bwd_ex", 0, p, p + 4, gb.data_ptr(), stat.data_ptr(), stat.data_ptr(), 1, 768, p + 4096 * 4, None, None, None,
             0, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and bool((stat == 0).all()), "a refused call wrote to its buffers"


# ================================================================================================================================
# 2. Losses and Block merge
# ================================================================================================================================
def js_ref(P, Q):
    lp, lq = torch.log_softmax(P, -1), torch.log_softmax(Q, -1)
    p, q = lp.exp(), lq.exp()
    lm = torch.log(0.5 * (p + q))
    # KLDivLoss: 0 * log 0 = 0
    kl_p = torch.where(p > 0, p * (lp - lm), torch.zeros_like(p))
    kl_q = torch.where(q > 0, q * (lq - lm), torch.zeros_like(q))
    return 0.5 * (kl_p.sum() + kl_q.sum()) / P.shape[0]


@pytest.mark.parametrize("B", [1, 2, 16, 17, 32, 63, 64, 65, 130])
def test_jsdiv(gpu, B):
    P, Q = 3.0 * rnd(B, B, seed=40), 3.0 * rnd(B, B, seed=41)
    # rows with logit gaps over 110: the other probabilities underflow to exactly 0 in fp32
    for r in range(0, B, 3):
        P[r, (r * 7) % B] = 125.0
    for r in range(1, B, 4):
        Q[r, (r * 5) % B] = -120.0 if B > 1 else 0.0
        Q[r, (r * 3) % B] += 115.0
    Pg, Qg = P.to(gpu), Q.to(gpu)
    out = Guarded(gpu, torch.float32, 1)
    dout = torch.tensor([0.7], device=gpu)
    dP, dQ = Guarded(gpu, torch.float32, B, B), Guarded(gpu, torch.float32, B, B)
    call("d2r_jsdiv_fwd", Pg.data_ptr(), Qg.data_ptr(), B, out.ptr, _st())
    call("d2r_jsdiv_bwd", Pg.data_ptr(), Qg.data_ptr(), B, dout.data_ptr(), dP.ptr, dQ.ptr, _st())
    torch.cuda.synchronize()
    for G, n in ((out, "out"), (dP, "dp"), (dQ, "dq")):
        G.intact(f"jsdiv[B={B}].{n}")
    Pr, Qr = P.double().requires_grad_(True), Q.double().requires_grad_(True)
    js = js_ref(Pr, Qr)
    (0.7 * js).backward()
    check(f"jsdiv[B={B}].out", out.t[0], js.detach(), torch.float32, scale=max(float(js.detach()), 1e-3))
    check(f"jsdiv[B={B}].dp", dP.t, Pr.grad, torch.float32)
    check(f"jsdiv[B={B}].dq", dQ.t, Qr.grad, torch.float32)


def test_jsdiv_mid_probability_underflow(gpu):
    """Regression: a subnormal probability next to one that is exactly 0 made (p + q) / 2 round to 0 in fp32, so
    p * (log p - log m) was inf and the loss and both gradients inf / NaN (seen at B = 65 and 130 with logit gaps over 100)."""
    B = 4
    P = torch.zeros(B, B)
    Q = torch.zeros(B, B)
    P[0] = torch.tensor([0.0, 102.3, 102.3, 102.3])  # p[0, 0] = exp(-102.3 - log 3) = 1.4e-45: the smallest subnormal
    Q[0] = torch.tensor([-120.0, 0.0, 0.0, 0.0])     # q[0, 0] = exp(-120 - log 3) underflows to 0
    Pg, Qg = P.to(gpu), Q.to(gpu)
    out, dP, dQ = Guarded(gpu, torch.float32, 1), Guarded(gpu, torch.float32, B, B), Guarded(gpu, torch.float32, B, B)
    dout = torch.tensor([1.0], device=gpu)
    call("d2r_jsdiv_fwd", Pg.data_ptr(), Qg.data_ptr(), B, out.ptr, _st())
    call("d2r_jsdiv_bwd", Pg.data_ptr(), Qg.data_ptr(), B, dout.data_ptr(), dP.ptr, dQ.ptr, _st())
    torch.cuda.synchronize()
    for G, n in ((out, "out"), (dP, "dp"), (dQ, "dq")):
        G.intact(f"jsdiv underflow.{n}")
    assert bool(torch.isfinite(out.t).all() and torch.isfinite(dP.t).all() and torch.isfinite(dQ.t).all()), "non-finite js_div"
    Pr, Qr = P.double().requires_grad_(True), Q.double().requires_grad_(True)
    js = js_ref(Pr, Qr)
    js.backward()
    check("jsdiv underflow.out", out.t[0], js.detach(), torch.float32, scale=max(float(js.detach()), 1e-3))
    check("jsdiv underflow.dp", dP.t, Pr.grad, torch.float32)
    check("jsdiv underflow.dq", dQ.t, Qr.grad, torch.float32)


CE_CASES = [(B, C) for B in (1, 32, 257, 600) for C in (1, 2, 3, 7, 100)]


@pytest.mark.parametrize("B,C", CE_CASES, ids=[f"B{b}-C{c}" for b, c in CE_CASES])
def test_cross_entropy(gpu, B, C):
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = 80.0 * (2.0 * torch.rand(B, C, generator=g) - 1.0)
    labels = torch.randint(0, C, (B,), generator=g)
    lg, lb = logits.to(gpu), labels.to(gpu)
    loss = Guarded(gpu, torch.float32, 1)
    dl = Guarded(gpu, torch.float32, B, C)
    dloss = torch.tensor([-1.7], device=gpu)
    call("d2r_ce_fwd", lg.data_ptr(), lb.data_ptr(), B, C, loss.ptr, _st())
    call("d2r_ce_bwd", lg.data_ptr(), lb.data_ptr(), B, C, dloss.data_ptr(), dl.ptr, _st())
    torch.cuda.synchronize()
    loss.intact(f"ce[B={B} C={C}].loss")
    dl.intact(f"ce[B={B} C={C}].dlogits")
    lr = logits.double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, labels)
    (-1.7 * ref).backward()
    check(f"ce[B={B} C={C}].loss", loss.t[0], ref.detach(), torch.float32, scale=max(float(ref.abs()), 1.0))
    check(f"ce[B={B} C={C}].dlogits", dl.t, lr.grad, torch.float32, scale=1.7 / B)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_block_merge(gpu, dtype):
    """S = 100 > 64 (each lane loops), chunk (0, 1) identically zero (F.normalize's clamp), entries with z exactly 0."""
    B, C, R, S = 3, 4, 5, 100
    g = torch.Generator().manual_seed(50)
    # |z| >= R / 4 away from the deliberate zeros: the sign of every product is fixed per (b, c, s)
    sgn = torch.where(torch.rand(B, C, 1, S, generator=g) < 0.5, -1.0, 1.0)
    m0 = 0.5 + torch.rand(B, C, R, S, generator=g)
    m1 = sgn * (0.5 + torch.rand(B, C, R, S, generator=g))
    m0[0, 1] = 0.0
    m0[1, 2, :, [3, 70, 99]] = 0.0
    m0, m1 = m0.to(dtype), m1.to(dtype)
    dout = rnd(B, C * S, seed=51).to(dtype)
    g0, g1, gd = m0.to(gpu), m1.to(gpu), dout.to(gpu)
    out, zraw = Guarded(gpu, dtype, B, C * S), Guarded(gpu, torch.float32, B, C * S)
    dm0, dm1 = Guarded(gpu, dtype, B, C * R * S), Guarded(gpu, dtype, B, C * R * S)
    code = CODE[dtype]
    call("d2r_block_merge_fwd", code, g0.data_ptr(), g1.data_ptr(), B, C, R, S, out.ptr, zraw.ptr, _st())
    call("d2r_block_merge_bwd", code, g0.data_ptr(), g1.data_ptr(), zraw.ptr, gd.data_ptr(), B, C, R, S, dm0.ptr, dm1.ptr, _st())
    torch.cuda.synchronize()
    tag = f"block_merge[{DT_IDS[dtype]}]"
    for G, n in ((out, "out"), (zraw, "zraw"), (dm0, "dm0"), (dm1, "dm1")):
        G.intact(f"{tag}.{n}")
    a, b, d = m0.double(), m1.double(), dout.double().view(B, C, S)
    z = (a * b).sum(2)
    y = torch.sign(z) * z.abs().sqrt()
    n2 = y.norm(dim=-1, keepdim=True)
    nrm = n2.clamp_min(1e-12)
    yh = y / nrm
    # F.normalize's gradient; sign(z) sqrt|z| has derivative 0.5 / sqrt|z|, taken as 0 at z = 0
    dy = torch.where(n2 > 1e-12, (d - yh * (yh * d).sum(-1, keepdim=True)) / nrm, d / nrm)
    dz = torch.where(z != 0, dy * 0.5 / z.abs().clamp_min(1e-300).sqrt(), torch.zeros_like(z))
    check(f"{tag}.zraw", zraw.t, z.reshape(B, -1), torch.float32)
    check(f"{tag}.out", out.t, yh.reshape(B, -1), dtype)
    assert bool((out.t.view(B, C, S)[0, 1] == 0).all()), f"{tag}: the all-zero chunk must give 0"
    check(f"{tag}.dm0", dm0.t, (dz[:, :, None, :] * b).reshape(B, -1), dtype, loosen=2.0)
    check(f"{tag}.dm1", dm1.t, (dz[:, :, None, :] * a).reshape(B, -1), dtype, loosen=2.0)
    assert bool((dm0.t.view(B, C, R, S)[1, 2, :, [3, 70, 99]] == 0).all()), f"{tag}: z == 0 entries must get no gradient"


# ================================================================================================================================
# 3. SAF gate
# ================================================================================================================================
def saf_ref(a, bw, bb, train, rm, rv):
    mu, var = (a.mean(), a.var(unbiased=False)) if train else (torch.tensor(rm, dtype=torch.float64), torch.tensor(rv, dtype=torch.float64))
    s = torch.sigmoid((a - mu) / torch.sqrt(var + 1e-5) * bw + bb)
    return s / (s.abs().sum(-1, keepdim=True) + 1e-8)


class Saf:
    def __init__(self, gpu, B, n, seed):
        self.gpu, self.B, self.n = gpu, B, n
        self.a = 2.0 * rnd(B, n, seed=seed) + 0.3
        self.dw = rnd(B, n, seed=seed + 1)
        self.bw, self.bb, self.rm, self.rv = 1.3, -0.2, 0.1, 1.5
        self.bw_d = torch.tensor([self.bw], device=gpu)
        self.bb_d = torch.tensor([self.bb], device=gpu)

    def running(self):
        return torch.tensor([self.rm], device=self.gpu), torch.tensor([self.rv], device=self.gpu)

    def ref(self, train):
        a = self.a.double().requires_grad_(True)
        bw = torch.tensor([self.bw], dtype=torch.float64, requires_grad=True)
        bb = torch.tensor([self.bb], dtype=torch.float64, requires_grad=True)
        w = saf_ref(a, bw, bb, train, self.rm, self.rv)
        (w * self.dw.double()).sum().backward()
        return w.detach(), a.grad, bw.grad, bb.grad


def f16_copy_matches_cast(gpu, src32, copy16, dtype, what):
    """copy16 must be bit-identical to d2r_cast(fp32 -> dtype) of src32."""
    ref = torch.empty(src32.numel(), dtype=dtype, device=gpu)
    src = src32.contiguous().view(-1)
    call("d2r_cast", 0, src.data_ptr(), CODE[dtype], ref.data_ptr(), src.numel(), _st())
    torch.cuda.synchronize()
    assert torch.equal(copy16.reshape(-1).view(torch.int16), ref.view(torch.int16)), f"{what}: 16-bit copy differs from d2r_cast"


SAF_CASES = [(B, n, train, lp) for (B, n) in ((32, 198), (3, 100)) for train in (True, False) for lp in (torch.bfloat16, torch.float16)]


@pytest.mark.parametrize("B,n,train,lowp", SAF_CASES, ids=[f"B{c[0]}-n{c[1]}-{'train' if c[2] else 'eval'}-{DT_IDS[c[3]]}" for c in SAF_CASES])
def test_saf_gate_ex(gpu, B, n, train, lowp):
    s = Saf(gpu, B, n, seed=60 + B)
    a, dw = s.a.to(gpu), s.dw.to(gpu)
    rm, rv = s.running()
    w, saved, w16 = Guarded(gpu, torch.float32, B, n), Guarded(gpu, torch.float32, 2), Guarded(gpu, lowp, B, n)
    call("d2r_saf_gate_fwd_ex", a.data_ptr(), B, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), rm.data_ptr(), rv.data_ptr(), int(train), w.ptr,
         saved.ptr, None, 0.0, w16.ptr, CODE[lowp], _st())
    da, da16 = Guarded(gpu, torch.float32, B, n), Guarded(gpu, lowp, B, n)
    g0w, g0b = 0.375, -1.25
    dbw, dbb = Guarded(gpu, torch.float32, 1, fill=torch.tensor([g0w])), Guarded(gpu, torch.float32, 1, fill=torch.tensor([g0b]))
    call("d2r_saf_gate_bwd_ex", a.data_ptr(), dw.data_ptr(), B, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), saved.ptr, int(train), da.ptr,
         dbw.ptr, dbb.ptr, 0, None, 0.0, da16.ptr, CODE[lowp], 1, _st())
    torch.cuda.synchronize()
    tag = f"saf_gate_ex[B={B} n={n} train={train} {DT_IDS[lowp]}]"
    for G, nm in ((w, "w"), (saved, "saved"), (w16, "w16"), (da, "da"), (da16, "da16"), (dbw, "d_bn_w"), (dbb, "d_bn_b")):
        G.intact(f"{tag}.{nm}")
    rw, ra, rbw, rbb = s.ref(train)
    check(f"{tag}.w", w.t, rw, torch.float32)
    check(f"{tag}.da", da.t, ra, torch.float32, loosen=5.0)
    f16_copy_matches_cast(gpu, w.t, w16.t, lowp, f"{tag}.w16")
    f16_copy_matches_cast(gpu, da.t, da16.t, lowp, f"{tag}.da16")
    # accumulate = 1: added into the pre-filled sinks (the BatchNorm parameter gradients exist in eval mode too)
    check(f"{tag}.d_bn_w", dbw.t, rbw + g0w, torch.float32, scale=max(float(rbw.abs()), 1e-2), loosen=5.0)
    check(f"{tag}.d_bn_b", dbb.t, rbb + g0b, torch.float32, scale=max(float(rbb.abs()), 1e-2), loosen=5.0)
    if train:
        N, a64 = B * n, s.a.double()
        assert abs(float(rm[0]) - (0.9 * s.rm + 0.1 * float(a64.mean()))) < 1e-5
        assert abs(float(rv[0]) - (0.9 * s.rv + 0.1 * float(a64.var(unbiased=False)) * N / (N - 1))) < 1e-5
    else:
        assert float(rm[0]) == pytest.approx(s.rm) and float(rv[0]) == pytest.approx(s.rv), "eval mode must not touch running stats"


def test_saf_gate_global_batch_split(gpu):
    """Two 'ranks' of 13 and 19 samples: stats on each, host sum, forward with gstats; backward phase 1 on each, host sum of gsums,
    phase 2.  Equals phase 0 on the whole batch to fp32 rounding, and the fp64 reference."""
    B, n, cut = 32, 198, 13
    s = Saf(gpu, B, n, seed=70)
    a, dw = s.a.to(gpu), s.dw.to(gpu)
    st = _st()
    # whole batch, phase 0
    rm0, rv0 = s.running()
    w0, sv0, da0 = torch.empty(B, n, device=gpu), torch.empty(2, device=gpu), torch.empty(B, n, device=gpu)
    dbw0, dbb0 = torch.zeros(1, device=gpu), torch.zeros(1, device=gpu)
    call("d2r_saf_gate_fwd_ex", a.data_ptr(), B, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), rm0.data_ptr(), rv0.data_ptr(), 1, w0.data_ptr(),
         sv0.data_ptr(), None, 0.0, None, 0, st)
    call("d2r_saf_gate_bwd_ex", a.data_ptr(), dw.data_ptr(), B, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), sv0.data_ptr(), 1, da0.data_ptr(),
         dbw0.data_ptr(), dbb0.data_ptr(), 0, None, 0.0, None, 0, 0, st)
    ranks = [(0, cut), (cut, B)]
    ntot = float(B * n)
    sums = [Guarded(gpu, torch.float64, 2) for _ in ranks]
    for (r0, r1), sm in zip(ranks, sums):
        call("d2r_saf_gate_stats", a[r0:r1].data_ptr(), r1 - r0, n, sm.ptr, st)
    gstats = sums[0].t + sums[1].t
    outs = []
    for k, (r0, r1) in enumerate(ranks):
        rm, rv = s.running()
        w, sv = Guarded(gpu, torch.float32, r1 - r0, n), Guarded(gpu, torch.float32, 2)
        call("d2r_saf_gate_fwd_ex", a[r0:r1].data_ptr(), r1 - r0, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1,
             w.ptr, sv.ptr, gstats.data_ptr(), ntot, None, 0, st)
        da, gs = Guarded(gpu, torch.float32, r1 - r0, n), Guarded(gpu, torch.float64, 2)
        dbw, dbb = torch.zeros(1, device=gpu), torch.zeros(1, device=gpu)
        call("d2r_saf_gate_bwd_ex", a[r0:r1].data_ptr(), dw[r0:r1].data_ptr(), r1 - r0, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), sv.ptr, 1,
             da.ptr, dbw.data_ptr(), dbb.data_ptr(), 1, gs.ptr, ntot, None, 0, 0, st)
        outs.append((rm, rv, w, sv, da, gs, dbw, dbb))
    gsums = outs[0][5].t + outs[1][5].t
    for k, (r0, r1) in enumerate(ranks):
        o = outs[k]
        call("d2r_saf_gate_bwd_ex", a[r0:r1].data_ptr(), dw[r0:r1].data_ptr(), r1 - r0, n, s.bw_d.data_ptr(), s.bb_d.data_ptr(), o[3].ptr, 1,
             o[4].ptr, None, None, 2, gsums.data_ptr(), ntot, None, 0, 0, st)
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        for G, nm in ((sums[k], "sums"), (o[2], "w"), (o[3], "saved"), (o[4], "da"), (o[5], "gsums")):
            G.intact(f"saf split rank {k}.{nm}")
    a64 = s.a.double()
    assert float((gstats[0] - a64.sum()).abs()) <= 1e-9 * float(a64.abs().sum()), "fp64 sums of the two ranks"
    assert float((gstats[1] - (a64 ** 2).sum()).abs()) <= 1e-9 * float((a64 ** 2).sum())
    w_split = torch.cat([outs[0][2].t, outs[1][2].t])
    da_split = torch.cat([outs[0][4].t, outs[1][4].t])
    rw, ra, rbw, rbb = s.ref(True)
    check("saf split.w vs phase 0", w_split, f64(w0), torch.float32)
    check("saf split.da vs phase 0", da_split, f64(da0), torch.float32, loosen=5.0)
    check("saf split.w", w_split, rw, torch.float32)
    check("saf split.da", da_split, ra, torch.float32, loosen=5.0)
    check("saf split.d_bn_w", outs[0][6] + outs[1][6], rbw, torch.float32, scale=max(float(rbw.abs()), 1e-2), loosen=5.0)
    check("saf split.d_bn_b", outs[0][7] + outs[1][7], rbb, torch.float32, scale=max(float(rbb.abs()), 1e-2), loosen=5.0)
    for k in range(2):  # every rank updates its running statistics with the global ones
        assert abs(float(outs[k][0][0]) - float(rm0[0])) < 1e-6 and abs(float(outs[k][1][0]) - float(rv0[0])) < 1e-5


# ================================================================================================================================
# 4. Elementwise
# ================================================================================================================================
_MANT = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def ulp(x, dtype):
    m, emin = _MANT[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - m)


def within_ulp(name, got, ref, mag, dtype):
    """|got - ref| <= one ulp of the output type at the result, plus the fp32 rounding of the intermediate terms (4 * 2^-24 of
    their magnitude `mag`: it matters only where they cancel, and covers FMA contraction and 1-2 ulp fp32 transcendentals)."""
    g = got.detach().cpu().double()
    rr = ref.to(dtype).double()
    bound = torch.maximum(ulp(ref, dtype), ulp(rr, dtype)) + 4.0 * 2.0 ** -24 * mag
    err = (g - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.nonzero()[0, 0])
        raise AssertionError(f"{name}: {int(bad.sum())} element(s) off by more than one ulp; first at {i}: got {float(g[i])!r}, "
                             f"fp64 {float(ref[i])!r}, bound {float(bound[i]):.3e}")


def _act_ref(code, x):
    return {0: lambda: x, 1: lambda: x.clamp_min(0), 2: lambda: torch.tanh(x), 3: lambda: torch.nn.functional.gelu(x),
            4: lambda: x * torch.sigmoid(1.702 * x), 5: lambda: torch.tanh(x).clamp_min(0), 6: lambda: torch.sigmoid(x)}[code]()


def _act_grad_ref(code, r):
    if code == 1:
        return (r > 0).double()
    if code == 2:
        return 1 - r * r
    if code == 3:
        return 0.5 * (1 + torch.erf(r / math.sqrt(2))) + r * torch.exp(-0.5 * r * r) / math.sqrt(2 * math.pi)
    if code == 4:
        s = torch.sigmoid(1.702 * r)
        return s + 1.702 * r * s * (1 - s)
    if code == 5:
        return torch.where(r > 0, 1 - r * r, torch.zeros_like(r))
    if code == 6:
        return r * (1 - r)
    return torch.ones_like(r)


ACT_NAMES = ["none", "relu", "tanh", "gelu", "quick_gelu", "tanh_relu", "sigmoid"]


def _ew_ops():
    """name -> (entry point, leading int args, #inputs, #outputs, fp64 reference -> [(out, magnitude of its terms)])"""
    ops = {}
    for c, nm in enumerate(ACT_NAMES):
        ops[f"act_fwd_{nm}"] = ("d2r_act_fwd", (c,), 1, 1, lambda x, c=c: [(_act_ref(c, x[0]), x[0].abs() + _act_ref(c, x[0]).abs())])
        ops[f"act_bwd_{nm}"] = ("d2r_act_bwd", (c,), 2, 1,
                                lambda x, c=c: [(x[0] * _act_grad_ref(c, x[1]), x[0].abs() * (1 + 2 * x[1].abs() + x[1] * x[1]))])
    for c in (2, 3):
        ops[f"act_bwd2_{ACT_NAMES[c]}"] = ("d2r_act_bwd2", (c,), 4, 2, lambda x, c=c: [
            (x[0] * _act_grad_ref(c, x[1]), x[0].abs() * (1 + 2 * x[1].abs() + x[1] * x[1])),
            (x[2] * _act_grad_ref(c, x[3]), x[2].abs() * (1 + 2 * x[3].abs() + x[3] * x[3]))])
    ops["sqdiff_fwd"] = ("d2r_sqdiff_fwd", (), 2, 1, lambda x: [((x[0] - x[1]) ** 2, (x[0].abs() + x[1].abs()) ** 2)])
    ops["sqdiff_bwd"] = ("d2r_sqdiff_bwd", (), 3, 2, lambda x: [(2 * (x[0] - x[1]) * x[2], 2 * (x[0].abs() + x[1].abs()) * x[2].abs()),
                                                                (-2 * (x[0] - x[1]) * x[2], 2 * (x[0].abs() + x[1].abs()) * x[2].abs())])
    ops["muladd_fwd"] = ("d2r_muladd_fwd", (), 3, 1, lambda x: [(x[0] * x[1] + x[2], (x[0] * x[1]).abs() + x[2].abs())])
    ops["muladd_bwd"] = ("d2r_muladd_bwd", (), 3, 2, lambda x: [(x[2] * x[1], (x[2] * x[1]).abs()), (x[2] * x[0], (x[2] * x[0]).abs())])
    ops["lerp_fwd"] = ("d2r_lerp_fwd", (), 3, 1, lambda x: [(x[0] * x[1] + (1 - x[0]) * x[2],
                                                             (x[0] * x[1]).abs() + ((1 - x[0]) * x[2]).abs() + x[2].abs())])
    ops["lerp_bwd"] = ("d2r_lerp_bwd", (), 4, 3, lambda x: [(x[3] * (x[1] - x[2]), x[3].abs() * (x[1].abs() + x[2].abs())),
                                                            (x[3] * x[0], (x[3] * x[0]).abs()),
                                                            (x[3] * (1 - x[0]), x[3].abs() * (1 + x[0].abs()))])
    ops["add"] = ("d2r_add", (), 2, 1, lambda x: [(x[0] + x[1], x[0].abs() + x[1].abs())])
    ops["add2"] = ("d2r_add2", (), 4, 2, lambda x: [(x[0] + x[1], x[0].abs() + x[1].abs()), (x[2] + x[3], x[2].abs() + x[3].abs())])
    return ops


EW_OPS = _ew_ops()
# ops with one rounding per output: the vector body and the scalar path (tail, misaligned operand) give the same bits.  The
# others are contracted to FMAs differently in the two loops (e.g. lerp: v_pk_fma_f32 in the body, multiply + add in the tail), so
# there every path is held to the one-ulp criterion instead.
EW_PATH_EXACT = tuple(f"act_fwd_{a}" for a in ACT_NAMES) + ("add", "add2", "muladd_bwd")
EW_BIG = ("add", "lerp_bwd", "act_bwd2_gelu", "act_fwd_gelu")  # also run at ~9e6 elements (grid-stride beyond 2048 blocks)


def _ew_args(name, x_ptrs, o_ptrs, n, dtype):
    ent, lead, nin, nout, _ = EW_OPS[name]
    if ent in ("d2r_add2",):
        return (CODE[dtype], x_ptrs[0], x_ptrs[1], o_ptrs[0], x_ptrs[2], x_ptrs[3], o_ptrs[1], n, _st())
    if ent == "d2r_act_bwd2":
        return (CODE[dtype], *lead, x_ptrs[0], x_ptrs[1], o_ptrs[0], x_ptrs[2], x_ptrs[3], o_ptrs[1], n, _st())
    return (CODE[dtype], *lead, *x_ptrs, *o_ptrs, n, _st())


def _ew_inputs(name, n, dtype, gpu):
    g = torch.Generator(device=gpu).manual_seed(n % 100003 + len(name))
    nin = EW_OPS[name][2]
    xs = [torch.randn(n, generator=g, device=gpu) * 2.0 for _ in range(nin)]
    if name.startswith("lerp"):
        xs[0] = torch.rand(n, generator=g, device=gpu)  # the gate lies in [0, 1]
    if name.startswith("act_bwd"):
        c = ACT_NAMES.index(name.split("_", 2)[2])
        for k in range(1, nin, 2):  # ref = the activation output for the output-referenced codes
            if c in (1, 2, 5, 6):
                xs[k] = _act_ref(c, xs[k])
    return [x.to(dtype) for x in xs]


@pytest.mark.parametrize("name", list(EW_OPS))
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_elementwise(gpu, dtype, name):
    """Sizes 1, VEC - 1, VEC + 1 (scalar tail), 1000003 (and ~9e6 for some ops: grid-stride past 2048 blocks); each input and each
    output moved one element off 16 bytes in turn (everything on the scalar path).  Every run is within one ulp of fp64; the
    single-rounding ops (EW_PATH_EXACT) must also give the aligned run's bits."""
    ent, _, nin, nout, ref = EW_OPS[name]
    v = VEC[dtype]
    sizes = [1, v - 1, v + 1, 1000003] + ([9000011] if name in EW_BIG else [])
    for n in sizes:
        xs = _ew_inputs(name, n, dtype, gpu)
        runs = []
        for mis in range(-1, nin + nout):  # -1: everything aligned
            X = [Guarded(gpu, dtype, n, shift=int(mis == k), fill=xs[k]) for k in range(nin)]
            O = [Guarded(gpu, dtype, n, shift=int(mis == nin + k)) for k in range(nout)]
            call(ent, *_ew_args(name, [x.ptr for x in X], [o.ptr for o in O], n, dtype))
            torch.cuda.synchronize()
            for k, G in enumerate(X + O):
                G.intact(f"{name}[{DT_IDS[dtype]} n={n} misaligned={mis}] operand {k}")
            runs.append([o.t.clone() for o in O])
            del X, O
        x64 = [f64(x) for x in xs]
        for k, (r, mag) in enumerate(ref(x64)):
            within_ulp(f"{name}[{DT_IDS[dtype]} n={n}].out{k}", runs[0][k], r, mag, dtype)
            for mis in range(nin + nout):
                within_ulp(f"{name}[{DT_IDS[dtype]} n={n} operand {mis} misaligned].out{k}", runs[mis + 1][k], r, mag, dtype)
                if name not in EW_PATH_EXACT:
                    continue
                assert torch.equal(runs[mis + 1][k].view(_SENT[dtype][0]), runs[0][k].view(_SENT[dtype][0])), \
                    f"{name}[{DT_IDS[dtype]} n={n}].out{k}: operand {mis} misaligned gives different bits"


@pytest.mark.parametrize("beta", [0.0, -0.75])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_axpby(gpu, dtype, beta):
    """y = alpha x + beta y; with beta = 0 a NaN already in y must not leak into the result."""
    alpha = 1.5
    for n in (1, VEC[dtype] - 1, VEC[dtype] + 1, 1000003, 9000011):
        g = torch.Generator(device=gpu).manual_seed(n % 9973)
        x = torch.randn(n, generator=g, device=gpu).to(dtype)
        y0 = torch.full((n,), float("nan"), device=gpu).to(dtype) if beta == 0.0 else torch.randn(n, generator=g, device=gpu).to(dtype)
        runs = []
        for mis in (-1, 0, 1):
            X = Guarded(gpu, dtype, n, shift=int(mis == 0), fill=x)
            Y = Guarded(gpu, dtype, n, shift=int(mis == 1), fill=y0)
            call("d2r_axpby", CODE[dtype], alpha, X.ptr, beta, Y.ptr, n, _st())
            torch.cuda.synchronize()
            X.intact(f"axpby[{DT_IDS[dtype]} n={n}].x")
            Y.intact(f"axpby[{DT_IDS[dtype]} n={n}].y")
            runs.append(Y.t.clone())
        x64, y64 = f64(x), f64(y0)
        r = alpha * x64 + (beta * y64 if beta != 0.0 else 0.0)
        mag = alpha * x64.abs() + (abs(beta) * y64.abs() if beta != 0.0 else 0.0)
        within_ulp(f"axpby[{DT_IDS[dtype]} beta={beta} n={n}]", runs[0], r, mag, dtype)
        for k in (1, 2):
            assert torch.equal(runs[k].view(_SENT[dtype][0]), runs[0].view(_SENT[dtype][0])), f"axpby n={n}: misaligned run differs"


CAST_PAIRS = [(torch.float32, torch.bfloat16), (torch.float32, torch.float16), (torch.bfloat16, torch.float32),
              (torch.float16, torch.float32), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
              (torch.float16, torch.float16)]


def _cast_source(src):
    """Random values plus ties (halfway between two 16-bit neighbours), values beyond fp16's range, NaN, infinities, signed
    zeros and subnormals of every type."""
    v = [rnd(1000, seed=80).double() * 3.0]
    # ties: x = k + 0.5 ulp for bf16 / fp16 at several binades (even and odd k)
    for e in (-3, 0, 5, 12):
        for m, bits in ((7, 0), (10, 0)):
            base = torch.arange(1, 9, dtype=torch.float64) * 2.0 ** (e - m) + 2.0 ** e
            v.append(base + 2.0 ** (e - m - 1))
            v.append(-(base + 2.0 ** (e - m - 1)))
    v.append(torch.tensor([65504.0, 65519.0, 65520.0, 65536.0, 1e5, 3e38, -65520.0, -1e6, float("inf"), float("-inf"),
                           float("nan"), 0.0, -0.0]))
    v.append(torch.tensor([1e-40, -1e-40, 1.4e-45, 2.0 ** -126, 2.0 ** -127, 6e-8, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 3, 1e-6, -3e-7,
                           2.0 ** -14, 2.0 ** -15, 1e-38]))
    x = torch.cat(v).float()
    return x.to(src)


@pytest.mark.parametrize("pair", CAST_PAIRS, ids=pair_id)
def test_cast(gpu, pair):
    src, dst = pair
    base = _cast_source(src)
    for n in (base.numel(), base.numel() - 1, base.numel() - 2, 3, 1):  # n % 4 covers 0..3
        xs = base[:n]
        S = Guarded(gpu, src, n, fill=xs)
        D = Guarded(gpu, dst, n)
        call("d2r_cast", CODE[src], S.ptr, CODE[dst], D.ptr, n, _st())
        torch.cuda.synchronize()
        S.intact(f"cast[{pair_id(pair)} n={n}].src")
        D.intact(f"cast[{pair_id(pair)} n={n}].dst")
        got, ref = D.t.cpu(), xs.to(dst)
        it = _SENT[dst][0]
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(got), nan), f"cast[{pair_id(pair)}]: NaN positions differ"
        same = got.view(it)[~nan] == ref.view(it)[~nan]
        if not bool(same.all()):
            i = int((~same).nonzero()[0, 0])
            raise AssertionError(f"cast[{pair_id(pair)} n={n}]: {int((~same).sum())} element(s) differ from torch.Tensor.to; first: "
                                 f"{float(xs[~nan][i])!r} -> {float(got[~nan][i])!r}, expected {float(ref[~nan][i])!r}")


def _keep_ref(n, p, seed):
    """The counter-based mask of d2r_dropout (splitmix64 finaliser of seed + (i + 1) * golden ratio), in numpy uint64."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return torch.from_numpy((z >> np.uint64(40)) >= np.uint64(int(float(np.float32(p)) * 16777216.0)))


@pytest.mark.parametrize("n", [1003, 77777])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS.get)
def test_dropout_paths_keep_the_same_elements(gpu, dtype, n):
    """With one seed, the vector path (all aligned) and the scalar path (x, add or y one element off 16 bytes) keep exactly the same
    elements - the backward regenerates the mask from (seed, index) - and the kept set is the counter-based generator's."""
    p, seed = 0.1, 0x1234567890ABCDEF
    g = torch.Generator(device=gpu).manual_seed(n)
    x = (1.0 + torch.rand(n, generator=g, device=gpu)).to(dtype)  # never 0: y != 0 <=> kept
    add = torch.randn(n, generator=g, device=gpu).to(dtype)
    it = _SENT[dtype][0]
    keep = _keep_ref(n, p, seed)
    for with_add in (False, True):
        runs = []
        for mis in (-1, 0, 1, 2):  # x, add, y misaligned in turn
            X = Guarded(gpu, dtype, n, shift=int(mis == 0), fill=x)
            A = Guarded(gpu, dtype, n, shift=int(mis == 1), fill=add)
            Y = Guarded(gpu, dtype, n, shift=int(mis == 2))
            call("d2r_dropout", CODE[dtype], X.ptr, A.ptr if with_add else None, Y.ptr, n, p, seed, _st())
            torch.cuda.synchronize()
            for G, nm in ((X, "x"), (A, "add"), (Y, "y")):
                G.intact(f"dropout[{DT_IDS[dtype]} n={n} add={with_add} misaligned={mis}].{nm}")
            runs.append(Y.t.clone())
        for k in range(1, 4):
            assert torch.equal(runs[k].view(it), runs[0].view(it)), f"dropout n={n} add={with_add}: misaligned operand {k - 1} differs"
        x64, a64 = f64(x), f64(add)
        r = torch.where(keep, x64 / (1 - p), torch.zeros_like(x64)) + (a64 if with_add else 0.0)
        within_ulp(f"dropout[{DT_IDS[dtype]} n={n} add={with_add}]", runs[0], r, x64.abs() / (1 - p) + a64.abs(), dtype)
        if not with_add:
            assert torch.equal(runs[0].cpu() != 0, keep), "kept elements differ from the counter-based generator"
