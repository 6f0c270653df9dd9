"""Every dispatch path of d2r_gemm (d2r_amd/csrc/gemm.hip, gemm_glds.hip, gemm8.hip) against fp64, through the raw descriptor.

Each case names the kernel variant it must reach (the launch timer's family // 100, include/d2r_hip_probes.h) so that a change of a
dispatch rule cannot quietly move a case to another kernel.  Operands are made in their 16-bit (or fp32) type first; the reference is
an fp64 expression of exactly those values.  Per element the result must satisfy

    |got - ref| <= u_out |ref| + slope |act'(G)| (u_v |v| + gamma alpha (|A| |B|)_mn) + (fp32 epilogue arithmetic) + tiny

with u_out half an ulp of the output type (the stored result), u_v the same (the 16-bit epilogues round v = alpha acc + bias to the
output type before the activation), gamma = 2 K 2^-24 (fp32 accumulation) and slope the activation's largest derivative.  A dropped or
repeated K-tile, a bias of the wrong column or batch row, a row of another tile or a mis-scaled split-K slab miss this by orders of
magnitude.  Everything outside the output rectangle (two extra rows, ldc padding narrower than 16 bytes, batch gaps) is a NaN pattern that
must come back bit-identical; with beta = 0 the output itself starts as NaN (a kernel that read C would show 0 * NaN).  Every case runs
twice and must be bit-identical to itself (split-K reductions are deterministic)."""
import ctypes as C
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, H, F = torch.bfloat16, torch.float16, torch.float32
LOWP = [BF, H]
LOWP_IDS = ["bf16", "fp16"]
U = {F: 2.0 ** -24, BF: 2.0 ** -8, H: 2.0 ** -11}  # half an ulp, relative
NONE, RELU, TANH, GELU, QGELU, TRELU, SIGM = range(7)
SLOPE = {NONE: 1.0, RELU: 1.0, TANH: 1.0, GELU: 1.13, QGELU: 1.1, TRELU: 1.0, SIGM: 0.25}  # max |act'|
NT, NN, TN = 0, 1, 2
TINY = 2.0 ** -22
EPS32 = 2.0 ** -24
# d2r_gemm_tuning codes that put every switch back to its default (gemm.hip: g_gemm8, g_group, g_splitk, g_wgrad_glds,
# g_gemm8_wgrad, g_gemm8_min = 150, g_dbg = 0), then (nbuf 1, vectorised epilogue on, automatic tile)
DEFAULT_SWITCHES = (111, 121, 131, 101, 103, 1150, 2000)


def _L():
    from d2r_amd import _lib
    return _lib.load()


def _restore_tuning():
    lib = _L()
    for code in DEFAULT_SWITCHES:
        lib.d2r_gemm_tuning(1, 1, code)
    lib.d2r_gemm_tuning(1, 1, -1)


@pytest.fixture(autouse=True)
def default_tuning(gpu):
    """d2r_gemm_tuning state is process-global: every test starts and ends on the defaults."""
    _restore_tuning()
    yield
    _restore_tuning()


def _code(dt):
    from d2r_amd._lib import BF16, F16, F32
    return {F: F32, BF: BF16, H: F16}[dt]


def _act(act, v):
    if act == RELU:
        return v.clamp_min(0.0)
    if act == TANH:
        return torch.tanh(v)
    if act == GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == QGELU:
        return v * torch.sigmoid(1.702 * v)
    if act == TRELU:
        return torch.tanh(v).clamp_min(0.0)
    if act == SIGM:
        return torch.sigmoid(v)
    return v


def _act_grad(act, r):
    """d act / dx given r = the activation output (relu, tanh, tanh_relu, sigmoid) or the pre-activation (gelu, quick_gelu)."""
    if act == RELU:
        return (r > 0).double()
    if act == TANH:
        return 1.0 - r * r
    if act == GELU:
        return 0.5 * (1.0 + torch.erf(r / math.sqrt(2.0))) + r * torch.exp(-0.5 * r * r) / math.sqrt(2.0 * math.pi)
    if act == QGELU:
        s = torch.sigmoid(1.702 * r)
        return s + 1.702 * r * s * (1.0 - s)
    if act == TRELU:
        return torch.where(r > 0, 1.0 - r * r, torch.zeros_like(r))
    if act == SIGM:
        return r * (1.0 - r)
    return torch.ones_like(r)


def _nan_like(n, dt, device):
    """n elements of dt whose bytes are all 0xFF: a NaN in fp32, bf16 and fp16."""
    es = torch.tensor([], dtype=dt).element_size()
    return torch.full((n * es,), 255, dtype=torch.uint8, device=device).view(dt)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _timer_families():
    lib = _L()
    cap = 64
    fam, fl, by, ms = (C.c_int * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_float * cap)()
    n = lib.d2r_gemm_timer_read(fam, fl, by, ms, cap)
    return [fam[i] for i in range(n)]


def _strides(rows, ld, nb, nh, bcast_h=False):
    """(batch stride, head stride) of a stack of [rows, ld] matrices with gaps between them (distinct for b and h)."""
    if nb * nh == 1:
        return 0, 0
    size = rows * ld
    sh = 0 if bcast_h else size + 8
    sb = (size if bcast_h else nh * sh) + 24
    return sb, sh


def _flat_len(off, sb, sh, nb, nh, rows, ld):
    return off + (nb - 1) * sb + (nh - 1) * sh + rows * ld + 8


def _view64(flat64, off, rows, cols, ld):
    return torch.as_strided(flat64, (rows, cols), (ld, 1), off)


SPEC = dict(dt=BF, cdt=None, layout=NT, M=64, N=64, K=64, nb=1, nh=1, a_off=0, b_off=0, lda=None, ldb=None, ldc=None, ldr=None,
            bias=False, sbias=False, act=NONE, alpha=1.0, beta=0.0, res=False, pre=False, gact=NONE, ws=0, dbias=False, bcast=None,
            tune=(), expect=None, scale=1.0)


def case(expect, **kw):
    s = dict(SPEC, **kw)
    s["expect"] = expect
    return s


def _id(s):
    parts = [{F: "f32", BF: "bf16", H: "fp16"}[s["dt"]], ("NT", "NN", "TN")[s["layout"]], f"{s['M']}x{s['N']}x{s['K']}"]
    if s["cdt"] not in (None, s["dt"]):
        parts.append("c" + {F: "f32", BF: "bf16", H: "fp16"}[s["cdt"]])
    for k in ("nb", "nh"):
        if s[k] != 1:
            parts.append(f"{k}{s[k]}")
    for k in ("a_off", "b_off", "lda", "ldb", "ldc", "ldr", "ws"):
        if s[k]:
            parts.append(f"{k}{s[k]}")
    for k in ("bias", "sbias", "res", "pre", "dbias"):
        if s[k]:
            parts.append(k)
    if s["act"]:
        parts.append(f"act{s['act']}")
    if s["gact"]:
        parts.append(f"gact{s['gact']}")
    if s["alpha"] != 1.0:
        parts.append(f"alpha{s['alpha']}")
    if s["beta"]:
        parts.append(f"beta{s['beta']}")
    if s["bcast"]:
        parts.append("bcast" + s["bcast"])
    if s["tune"]:
        parts.append("tune" + "-".join(map(str, s["tune"])))
    parts.append(f"v{s['expect']}")
    return "-".join(parts)


def run_case(gpu, s):
    """Launches the case twice and checks the path, the values against fp64, the untouched surroundings and determinism."""
    from d2r_amd import _lib
    from d2r_amd.functional import _stream
    lib = _L()
    dt, cdt, layout = s["dt"], s["cdt"] or s["dt"], s["layout"]
    M, N, K, nb, nh = s["M"], s["N"], s["K"], s["nb"], s["nh"]
    Z = nb * nh
    gen = torch.Generator().manual_seed(zlib.crc32(repr(sorted((k, str(v)) for k, v in s.items())).encode()))

    def rnd(n, dtype, scale=1.0):
        return (torch.randn(n, generator=gen, dtype=torch.float64) * scale).to(dtype)

    # ---- operands: A [M,K] stored [M,lda] (NT / NN) or [K,lda] (TN); B [K,N] stored [N,ldb] (NT) or [K,ldb] ------------------
    a_rows, a_cols = (M, K) if layout != TN else (K, M)
    b_rows, b_cols = (N, K) if layout == NT else (K, N)
    lda = s["lda"] if s["lda"] is not None else (a_cols or 8)
    ldb = s["ldb"] if s["ldb"] is not None else (b_cols or 8)
    sAb, sAh = _strides(a_rows, lda, nb, nh, s["bcast"] == "A")
    sBb, sBh = _strides(b_rows, ldb, nb, nh, s["bcast"] == "B")
    a_flat = rnd(_flat_len(s["a_off"], sAb, sAh, nb, nh, a_rows, lda), dt, s["scale"])
    b_flat = rnd(_flat_len(s["b_off"], sBb, sBh, nb, nh, b_rows, ldb), dt, s["scale"])
    a64, b64 = a_flat.double(), b_flat.double()

    # ---- output, pre-activation, residual, activation-gradient reference, bias, bias gradient ---------------------------------------
    ces = torch.tensor([], dtype=cdt).element_size()
    align = 16 // ces
    ldc = s["ldc"] if s["ldc"] is not None else ((N + 1 + align - 1) // align) * align  # padding of 1..8 columns (< 16 bytes)
    ldr = s["ldr"] if s["ldr"] is not None else ldc + align
    crow = M + 2  # two rows past the output
    sCb, sCh = _strides(crow, ldc, nb, nh)
    c_len = _flat_len(0, sCb, sCh, nb, nh, crow, ldc)
    inside = torch.zeros(c_len, dtype=torch.bool)
    for z in range(Z):
        zb, zh = divmod(z, nh)
        _view64(inside, zb * sCb + zh * sCh, M, N, ldc).fill_(True)
    c_init = _nan_like(c_len, cdt, "cpu")
    if s["beta"] != 0.0:
        c_init[inside] = rnd(int(inside.sum()), cdt)
    sRb, sRh = _strides(M, ldr, nb, nh)
    r_flat = rnd(_flat_len(0, sRb, sRh, nb, nh, M, ldr), cdt) if s["res"] else None
    g_flat = rnd(c_len, cdt) if s["gact"] else None
    s_bias_b = N + 8 if s["sbias"] else 0
    bias = rnd(N + (nb - 1) * s_bias_b, F) if s["bias"] else None
    db_init = None
    if s["dbias"]:
        db_init = torch.cat([rnd(M, F), _nan_like(4, F, "cpu")])

    dev = gpu
    Ag, Bg = a_flat.to(dev), b_flat.to(dev)
    Cg = c_init.to(dev)
    Pg = _nan_like(c_len, cdt, dev) if s["pre"] else None
    Rg = r_flat.to(dev) if r_flat is not None else None
    Gg = g_flat.to(dev) if g_flat is not None else None
    biasg = bias.to(dev) if bias is not None else None
    dbg = db_init.to(dev) if db_init is not None else None
    wsg = torch.zeros(s["ws"], dtype=torch.uint8, device=dev) if s["ws"] else None

    es = a_flat.element_size()
    d = _lib.GemmDesc(dtype=_code(dt), c_dtype=_code(cdt), layout=layout, act=s["act"], M=M, N=N, K=K, nb=nb, nh=nh,
                      alpha=s["alpha"], beta=s["beta"],
                      A=Ag.data_ptr() + s["a_off"] * es, lda=lda, sAb=sAb, sAh=sAh,
                      B=Bg.data_ptr() + s["b_off"] * es, ldb=ldb, sBb=sBb, sBh=sBh,
                      C=Cg.data_ptr(), ldc=ldc, sCb=sCb, sCh=sCh,
                      bias=None if biasg is None else biasg.data_ptr(),
                      residual=None if Rg is None else Rg.data_ptr(), ldr=ldr if Rg is not None else 0, sRb=sRb, sRh=sRh,
                      preact=None if Pg is None else Pg.data_ptr())
    d.s_bias_b = s_bias_b
    d.dbias = None if dbg is None else dbg.data_ptr()
    if Gg is not None:
        d.grad_ref, d.grad_act = Gg.data_ptr(), s["gact"]
    if wsg is not None:
        d.workspace, d.workspace_bytes = wsg.data_ptr(), wsg.numel()

    # overrides for paths the automatic rule does not take: tile codes, "nbuf2" (double-buffered generic kernel), "vepi0" (element-wise
    # epilogue); the default_tuning fixture puts everything back
    nbuf, vepi = (2 if "nbuf2" in s["tune"] else 1), (0 if "vepi0" in s["tune"] else 1)
    for code in [c for c in s["tune"] if not isinstance(c, str)] or [-1]:
        lib.d2r_gemm_tuning(nbuf, vepi, code)

    runs = []
    for _ in range(2):
        Cg.copy_(c_init.to(dev))
        if Pg is not None:
            Pg.copy_(_nan_like(c_len, cdt, dev))
        if dbg is not None:
            dbg.copy_(db_init.to(dev))
        lib.d2r_gemm_timer(1)
        try:
            _lib.call("d2r_gemm", C.byref(d), _stream())
        finally:
            fams = _timer_families()
            lib.d2r_gemm_timer(0)
        torch.cuda.synchronize()
        if M == 0 or N == 0:
            assert fams == [], f"an empty product launched {fams}"
        else:
            assert len(fams) == 1 and fams[0] // 100 == s["expect"], f"expected kernel variant {s['expect']}, the launch timer says {fams}"
        runs.append([t.clone() for t in (Cg, Pg, dbg) if t is not None])
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y)), "two launches of the same case differ"

    got_c = Cg.cpu()
    assert torch.equal(_bits(got_c[~inside]), _bits(c_init[~inside])), "the kernel wrote outside the output (rows, padding or gaps)"
    if Pg is not None:
        got_p = Pg.cpu()
        assert torch.equal(_bits(got_p[~inside]), _bits(_nan_like(c_len, cdt, "cpu")[~inside])), "preact written outside the output"
    if M == 0 or N == 0:
        if dbg is not None:
            assert torch.equal(_bits(dbg.cpu()), _bits(db_init))
        return

    c_old64 = c_init.double()
    u_out = U[cdt]
    slope = SLOPE[s["act"]]
    gamma = 2.0 * K * EPS32
    for z in range(Z):
        zb, zh = divmod(z, nh)
        if layout == TN:
            A = _view64(a64, s["a_off"] + zb * sAb + zh * sAh, K, M, lda).t()
        else:
            A = _view64(a64, s["a_off"] + zb * sAb + zh * sAh, M, K, lda)
        if layout == NT:
            B = _view64(b64, s["b_off"] + zb * sBb + zh * sBh, N, K, ldb).t()
        else:
            B = _view64(b64, s["b_off"] + zb * sBb + zh * sBh, K, N, ldb)
        acc = A @ B
        absacc = A.abs() @ B.abs()
        bv = bias.double()[zb * s_bias_b: zb * s_bias_b + N] if bias is not None else torch.zeros(N, dtype=torch.float64)
        v = s["alpha"] * acc + bv
        av = _act(s["act"], v)
        gf = _act_grad(s["gact"], _view64(g_flat.double(), zb * sCb + zh * sCh, M, N, ldc)) if s["gact"] else torch.ones_like(v)
        ref = av * gf
        extra = torch.zeros_like(v)
        if r_flat is not None:
            r = _view64(r_flat.double(), zb * sRb + zh * sRh, M, N, ldr)
            ref, extra = ref + r, extra + r.abs()
        if s["beta"] != 0.0:
            cold = _view64(c_old64, zb * sCb + zh * sCh, M, N, ldc)
            ref, extra = ref + s["beta"] * cold, extra + abs(s["beta"]) * cold.abs()
        e_v = u_out * v.abs() + gamma * abs(s["alpha"]) * absacc + 4 * EPS32 * (abs(s["alpha"]) * acc.abs() + bv.abs())
        bound = (u_out * ref.abs() + slope * gf.abs() * e_v + 8 * EPS32 * ((av.abs() + v.abs()) * gf.abs() + extra) + TINY)
        got = _view64(got_c.double(), zb * sCb + zh * sCh, M, N, ldc)
        err = (got - ref).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            m, n = divmod(i, N)
            raise AssertionError(f"batch {z}: {int(bad.sum())} of {M * N} elements outside the bound; first at [{m},{n}]: got "
                                 f"{float(got[m, n])!r}, ref {float(ref[m, n])!r}, bound {float(bound[m, n]):.3e}")
        if Pg is not None:
            p = _view64(got_p.double(), zb * sCb + zh * sCh, M, N, ldc)
            assert bool(((p - v).abs() <= e_v + TINY).all()), f"batch {z}: preact differs from alpha A B + bias"
    if dbg is not None:
        A = _view64(a64, s["a_off"], K, M, lda)
        ref_db = db_init.double()[:M] + A.sum(0)
        bound_db = gamma * A.abs().sum(0) + 4 * EPS32 * (db_init.double()[:M].abs() + A.sum(0).abs()) + TINY
        got_db = dbg.cpu()
        assert bool(((got_db[:M].double() - ref_db).abs() <= bound_db).all()), "dbias is not the prior value plus the column sums"
        assert torch.equal(_bits(got_db[M:]), _bits(db_init[M:])), "dbias written past M"


# ---------------------------------------------------------------------------------------------------------------------------------
# the case matrix: (kernel variant, descriptor); 16-bit cases run in both 16-bit types
# ---------------------------------------------------------------------------------------------------------------------------------
EPI_16 = [  # epilogue operands on a 16-bit output
    dict(bias=True),
    dict(bias=True, act=RELU, alpha=0.5),
    dict(bias=True, act=TANH, beta=1.0),
    dict(bias=True, act=GELU, pre=True),
    dict(bias=True, act=QGELU, pre=True, beta=-0.75),
    dict(bias=True, act=TRELU, alpha=-1.5),
    dict(bias=True, act=SIGM, beta=1.0, alpha=2.0),
    dict(bias=True, res=True, alpha=0.25),
]
GRAD = [dict(gact=a) for a in (RELU, TANH, GELU, QGELU, TRELU, SIGM)]

LOWP_CASES = []


def _lp(expect, **kw):
    LOWP_CASES.append((expect, kw))


# ---- generic register-staged tiles (0) ----
_lp(0, layout=NT, M=64, N=64, K=64)                    # (below the LDS-DMA kernel's 128 rows)
_lp(0, layout=NT, M=65, N=63, K=72)                    # ragged everything, K not a multiple of the 64-deep tile
_lp(0, layout=NN, M=63, N=65, K=130)
_lp(0, layout=TN, M=96, N=80, K=100)
_lp(0, layout=TN, M=33, N=129, K=64, dbias=True)
_lp(0, layout=NT, M=127, N=256, K=128)                 # one row short of the LDS-DMA kernel
_lp(0, layout=NT, M=256, N=256, K=200)                 # K % 64 != 0: not LDS-DMA
_lp(0, layout=NN, M=256, N=96, K=136)
_lp(0, layout=NT, M=256, N=256, K=64)                  # K below 128
_lp(0, layout=NN, M=256, N=100, K=128)                 # NN with N % 8 != 0
_lp(0, layout=NT, M=256, N=256, K=128, a_off=1)        # unaligned A pointer
_lp(0, layout=NT, M=256, N=256, K=128, b_off=1)        # unaligned B pointer
_lp(0, layout=NN, M=130, N=136, K=128, a_off=1, b_off=1)
_lp(0, layout=TN, M=136, N=136, K=128, b_off=1)
_lp(0, layout=NT, M=200, N=136, K=128, lda=131)        # ld not a multiple of 8
_lp(0, layout=NN, M=200, N=136, K=128, ldb=139)
_lp(0, layout=TN, M=72, N=72, K=130, lda=75, ldb=77)
_lp(0, layout=NT, M=100, N=100, K=100, ldc=101, bias=True, act=GELU, pre=True)  # unaligned ldc: element-wise epilogue
_lp(0, layout=NT, M=100, N=70, K=96, ldr=73, res=True, beta=1.0)                  # unaligned residual rows
for _e in EPI_16:
    _lp(0, layout=NT, M=96, N=70, K=136, **_e)
for _e in GRAD:
    _lp(0, layout=NN, M=72, N=99, K=200, bias=True, **_e)
for _t in (0, 1, 2, 3):                                # every generic tile, forced
    _lp(0, layout=NT, M=131, N=135, K=136, bias=True, act=GELU, pre=True, tune=(_t,))
    _lp(0, layout=NN, M=131, N=136, K=136, res=True, beta=-0.75, tune=(_t,))
    _lp(0, layout=TN, M=136, N=131, K=150, dbias=True, tune=(_t,))
_lp(0, layout=NT, M=131, N=135, K=200, bias=True, act=QGELU, tune=("nbuf2",))  # double-buffered LDS
_lp(0, layout=TN, M=131, N=136, K=200, dbias=True, tune=("nbuf2",))
_lp(0, layout=NT, M=96, N=70, K=136, bias=True, act=TANH, beta=1.0, pre=True, tune=("vepi0",))  # element-wise epilogue
# generic split-K (workspace, batch 1): slabs + the reduce launch
_lp(0, layout=TN, M=768, N=768, K=4096, ws=64 << 20)
_lp(0, layout=TN, M=768, N=768, K=1000, ws=64 << 20, dbias=True, beta=1.0)
_lp(0, layout=TN, M=768, N=768, K=4096, ws=3 * 768 * 768 * 4 + 4096, dbias=True)  # a workspace for three slabs only
_lp(0, layout=TN, M=768, N=768, K=512)                  # no workspace: one pass
_lp(0, layout=NT, M=40, N=768, K=3072, ws=64 << 20, bias=True, act=GELU, pre=True)
_lp(0, layout=NN, M=64, N=200, K=2000, ws=64 << 20, res=True, beta=1.0, alpha=0.5)
_lp(0, layout=NN, M=48, N=136, K=1024, ws=64 << 20, gact=GELU)
_lp(0, layout=NT, M=256, N=256, K=6144, ws=64 << 20, a_off=1)  # unaligned: the generic split-K instead of the in-launch one
_lp(0, layout=NT, M=20, N=768, K=1024, ws=64 << 20, a_off=1, bias=True, act=RELU)  # unaligned skinny shape: 32 x 64 tiles, split
# batched (nb x nh) with distinct strides, broadcast operands and per-batch bias rows
_lp(0, layout=NT, M=40, N=72, K=96, nb=3, nh=4, bias=True, sbias=True, act=RELU, res=True)
_lp(0, layout=NN, M=40, N=72, K=96, nb=3, nh=4, bcast="B", bias=True, sbias=True, beta=1.0)
_lp(0, layout=TN, M=40, N=72, K=96, nb=3, nh=4, bcast="A", pre=True, bias=True, sbias=True, act=GELU)
_lp(0, layout=NT, M=129, N=130, K=128, nb=2, nh=2, bias=True)   # batched: never LDS-DMA
# ---- K = 0: the epilogue of a zero product ----
_lp(0, layout=NT, M=64, N=72, K=0, bias=True, act=GELU, pre=True)
_lp(0, layout=NN, M=300, N=256, K=0, bias=True, res=True, beta=-0.75)
_lp(0, layout=TN, M=80, N=64, K=0, dbias=True, beta=1.0)
_lp(0, layout=TN, M=768, N=768, K=0, ws=64 << 20, alpha=2.0)
# ---- LDS-DMA 128 x 64 (1) and 128 x 128 on eight waves (3), automatic ----
for _m, _n, _k in ((128, 64, 128), (129, 72, 192), (255, 100, 128), (257, 127, 320), (129, 65, 128)):
    _lp(1, layout=NT, M=_m, N=_n, K=_k, bias=True)
for _m, _n, _k in ((129, 72, 128), (255, 120, 192)):
    _lp(1, layout=NN, M=_m, N=_n, K=_k, bias=True)
for _m, _n, _k in ((128, 128, 128), (129, 129, 192), (255, 255, 128), (257, 136, 320), (129, 250, 128)):
    _lp(3, layout=NT, M=_m, N=_n, K=_k, bias=True)
for _m, _n, _k in ((129, 136, 128), (257, 248, 192)):
    _lp(3, layout=NN, M=_m, N=_n, K=_k, bias=True)
for _e in EPI_16:
    _lp(1, layout=NT, M=129, N=100, K=192, **_e)
    _lp(3, layout=NN, M=200, N=136, K=192, **_e)
for _e in GRAD:
    _lp(1, layout=NN, M=136, N=72, K=128, bias=True, **_e)
    _lp(3, layout=NT, M=136, N=131, K=128, **_e)
_lp(3, layout=NT, M=129, N=131, K=128, ldc=136, ldr=144, res=True)  # residual rows narrower / wider than C's
_lp(3, layout=NT, M=129, N=131, K=128, ldc=131, bias=True, act=TANH)  # unaligned ldc: element-wise epilogue
_lp(1, layout=NN, M=129, N=72, K=192, tune=("vepi0",), bias=True, act=GELU, pre=True, beta=1.0)
# in-launch split-K of the eight-wave kernel (K >= 6144 over few tiles, workspace given)
_lp(3, layout=NT, M=256, N=256, K=6144, ws=64 << 20)
_lp(3, layout=NN, M=136, N=200, K=6400, ws=64 << 20, bias=True, act=GELU, pre=True, beta=1.0)
# ---- LDS-DMA variants reachable only by tile code: 4 -> 2, 5 -> 1, 6 -> 3, 7 -> 12, 8 -> 11, 9 -> 13 ----
for _tile, _var in ((4, 2), (5, 1), (6, 3), (7, 12), (8, 11), (9, 13)):
    _wide = _var in (2, 3, 12, 13)
    _lp(_var, layout=NT, M=129, N=131 if _wide else 72, K=192, bias=True, act=GELU, pre=True, tune=(_tile,))
    _lp(_var, layout=NN, M=257, N=136 if _wide else 120, K=128, res=True, beta=1.0, tune=(_tile,))
    _lp(_var, layout=TN, M=136, N=136 if _wide else 72, K=320, bias=True, alpha=0.5, tune=(_tile,))
    _lp(_var, layout=NT, M=136, N=136 if _wide else 72, K=128, bias=True, **GRAD[2], tune=(_tile,))
    _lp(0, layout=TN, M=136, N=136, K=192, dbias=True, tune=(_tile,))  # dbias keeps the generic kernel
# ---- 256 x 256 deep-pipelined kernel (8), forced at small sizes (the automatic rule needs >= 150 such tiles) ----
_lp(8, layout=NT, M=300, N=264, K=192, bias=True, act=GELU, pre=True, tune=(11,))
_lp(8, layout=NN, M=257, N=520, K=128, res=True, beta=-0.75, tune=(11,))
_lp(8, layout=NT, M=256, N=256, K=128, bias=True, **GRAD[0], tune=(11,))
_lp(0, layout=NT, M=300, N=264, K=192, a_off=1, bias=True, tune=(11,))  # not eligible (unaligned A): the generic kernel
# ---- 16-bit skinny (31): M <= 32 ----
for _m, _n, _k in ((1, 16, 64), (16, 17, 96), (17, 100, 64), (32, 1, 128), (32, 768, 1088)):
    _lp(31, layout=NT, M=_m, N=_n, K=_k, bias=True)
for _m, _n, _k in ((1, 16, 64), (17, 48, 96), (32, 768, 2080)):
    _lp(31, layout=NN, M=_m, N=_n, K=_k, bias=True)
for _e in EPI_16:
    _lp(31, layout=NT, M=20, N=70, K=160, **_e)
for _e in GRAD:
    _lp(31, layout=NN, M=24, N=64, K=96, bias=True, **_e)
_lp(0, layout=NN, M=20, N=72, K=96)                      # NN with N % 16 != 0: tiled kernel
_lp(0, layout=NT, M=20, N=72, K=80)                      # K % 32 != 0
_lp(0, layout=NT, M=20, N=72, K=96, a_off=1)             # unaligned A
_lp(0, layout=NT, M=20, N=72, K=96, nb=3)                # batched
# ---- 16-bit matrix-vector (34): N = 1 ----
_lp(34, layout=NT, M=64, N=1, K=8, bias=True)
_lp(34, layout=NT, M=257, N=1, K=72, bias=True, act=SIGM, alpha=0.5)
_lp(34, layout=NT, M=4100, N=1, K=776, ldc=3, act=TANH)
_lp(34, layout=NT, M=66, N=1, K=0, bias=True, act=GELU)
_lp(0, layout=NT, M=257, N=1, K=72, beta=1.0)            # accumulation: tiled kernel
_lp(0, layout=NT, M=257, N=1, K=76)                      # K % 8 != 0


@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
@pytest.mark.parametrize("expect,kw", LOWP_CASES, ids=[_id(case(e, **k)) for e, k in LOWP_CASES])
def test_gemm_16bit(gpu, dt, expect, kw):
    run_case(gpu, case(expect, dt=dt, **kw))


# fp32 output of 16-bit inputs, on every path that takes it
C32_CASES = [
    (0, dict(layout=NT, M=96, N=70, K=136, bias=True, act=GELU, pre=True, beta=1.0)),
    (0, dict(layout=TN, M=768, N=768, K=2048, ws=64 << 20, beta=1.0, dbias=True)),
    (1, dict(layout=NT, M=129, N=100, K=192, bias=True, act=RELU, res=True)),
    (3, dict(layout=NN, M=200, N=136, K=128, bias=True, act=QGELU, beta=-0.75, pre=True)),
    (31, dict(layout=NT, M=20, N=70, K=160, bias=True, act=TANH, beta=1.0)),
    (31, dict(layout=NN, M=7, N=32, K=64, res=True)),
    (34, dict(layout=NT, M=300, N=1, K=64, bias=True, act=TRELU)),
    (2, dict(layout=TN, M=136, N=136, K=128, tune=(4,))),
    (0, dict(layout=NT, M=64, N=64, K=0, bias=True, beta=1.0)),
]


@pytest.mark.parametrize("dt", LOWP, ids=LOWP_IDS)
@pytest.mark.parametrize("expect,kw", C32_CASES, ids=[_id(case(e, **k)) for e, k in C32_CASES])
def test_gemm_16bit_inputs_fp32_output(gpu, dt, expect, kw):
    run_case(gpu, case(expect, dt=dt, cdt=F, **kw))


F32_CASES = [
    # skinny fp32 (30): M <= 32, K % 16 == 0, K >= 64
    (30, dict(layout=NT, M=1, N=1, K=64)),
    (30, dict(layout=NT, M=16, N=17, K=80, bias=True, act=TRELU)),
    (30, dict(layout=NT, M=17, N=100, K=1200, bias=True, act=GELU, pre=True)),
    (30, dict(layout=NN, M=32, N=33, K=208, res=True, beta=-0.75)),
    (30, dict(layout=NN, M=5, N=768, K=768, bias=True, act=SIGM, alpha=0.5)),
    (30, dict(layout=NT, M=9, N=40, K=96, nb=3, nh=4, bias=True, sbias=True, act=RELU)),
    (30, dict(layout=NN, M=9, N=40, K=96, nb=3, nh=4, bcast="B", bias=True, sbias=True, res=True, beta=1.0)),
    (0, dict(layout=NT, M=16, N=40, K=72)),                 # K % 16 != 0
    (0, dict(layout=NT, M=16, N=40, K=48)),                 # K < 64
    (0, dict(layout=NT, M=16, N=40, K=96, a_off=1)),        # unaligned A
    (0, dict(layout=NT, M=16, N=40, K=96, lda=98)),         # unaligned rows
    (0, dict(layout=NT, M=16, N=40, K=96, gact=TANH, cdt=BF)),  # 16-bit (bf16) output with an activation-gradient reference
    # rank-K TN (32): K <= 64, plain products with M N >= 4096
    (32, dict(layout=TN, M=64, N=64, K=1)),
    (32, dict(layout=TN, M=100, N=77, K=17, beta=1.0, alpha=-1.5)),
    (32, dict(layout=TN, M=129, N=200, K=64, dbias=True, beta=1.0)),
    (32, dict(layout=TN, M=65, N=70, K=33, ldc=73)),
    (32, dict(layout=TN, M=48, N=96, K=40, nb=3, nh=4, bcast="A", beta=1.0)),
    (0, dict(layout=TN, M=100, N=77, K=17, bias=True)),    # an epilogue operand: tiled kernel
    (0, dict(layout=TN, M=40, N=40, K=17)),                 # M N < 4096
    # generic fp32 tiles
    (0, dict(layout=NT, M=33, N=65, K=33, bias=True, act=GELU, pre=True)),
    (0, dict(layout=NN, M=100, N=129, K=200, res=True, beta=1.0, alpha=0.5)),
    (0, dict(layout=TN, M=96, N=80, K=100, dbias=True)),
    (0, dict(layout=TN, M=768, N=768, K=1000, ws=64 << 20, dbias=True, beta=1.0)),  # generic split-K
    (0, dict(layout=NT, M=40, N=768, K=768, ws=64 << 20, bias=True, act=TANH)),
    (0, dict(layout=NT, M=40, N=72, K=96, nb=3, nh=4, bias=True, sbias=True, act=RELU, res=True)),
    (0, dict(layout=TN, M=40, N=72, K=96, nb=3, nh=4, bcast="B", bias=True, sbias=True, beta=-0.75)),
    (0, dict(layout=NT, M=64, N=64, K=64, tune=(3,), bias=True, act=QGELU)),
    (0, dict(layout=NN, M=64, N=64, K=64, tune=("nbuf2",), res=True)),
    (0, dict(layout=NT, M=64, N=72, K=0, bias=True, act=SIGM, pre=True)),
    (0, dict(layout=TN, M=100, N=77, K=0, dbias=True, beta=1.0)),
    (0, dict(layout=NT, M=64, N=72, K=96, cdt=H, bias=True, act=GELU, pre=True)),  # fp16 output of fp32 inputs
]


@pytest.mark.parametrize("expect,kw", F32_CASES, ids=[_id(case(e, dt=F, **k)) for e, k in F32_CASES])
def test_gemm_fp32(gpu, expect, kw):
    run_case(gpu, case(expect, dt=F, **kw))


@pytest.mark.parametrize("dt", [F, BF, H], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("mn", [(0, 64), (64, 0), (0, 0)], ids=["M0", "N0", "M0N0"])
def test_empty_products_write_nothing(gpu, dt, layout, mn):
    M, N = mn
    run_case(gpu, case(None, dt=dt, layout=layout, M=M, N=N, K=96, bias=True, act=GELU, pre=True, beta=1.0, res=True))


def test_every_reachable_gemm_variant_is_exercised(gpu):
    """One small representative per path the automatic rule reaches.  If a rule change makes a path unreachable (or moves the cases
    above to other kernels, so that their assertions fail), this says which."""
    reps = [
        case(0, dt=BF, layout=TN, M=128, N=128, K=64),
        case(1, dt=BF, layout=NT, M=256, N=96, K=128),
        case(3, dt=H, layout=NT, M=256, N=256, K=128),
        case(8, dt=BF, layout=NT, M=4096, N=3072, K=128, bias=True),  # 192 tiles of 256 x 256 (g_gemm8_min = 150, >= 70 % of a round)
        case(30, dt=F, layout=NT, M=8, N=64, K=64),
        case(31, dt=BF, layout=NN, M=8, N=64, K=64),
        case(32, dt=F, layout=TN, M=128, N=128, K=16),
        case(34, dt=H, layout=NT, M=256, N=1, K=64),
    ]
    seen = set()
    for s in reps:
        run_case(gpu, s)
        seen.add(s["expect"])
    assert seen == {0, 1, 3, 8, 30, 31, 32, 34}


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: every host-side check of gemm_desc_to_args and the grad_ref rule, with C untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def _refusal_desc(gpu, **over):
    from d2r_amd import _lib
    M, N, K = 64, 64, 64
    bufs = dict(A=torch.randn(M, K, device=gpu).bfloat16(), B=torch.randn(N, K, device=gpu).bfloat16(),
                C=_nan_like(M * N, BF, gpu).view(M, N), R=torch.randn(M, N, device=gpu).bfloat16(),
                W=torch.zeros(1 << 20, dtype=torch.uint8, device=gpu), D=torch.zeros(M, device=gpu), C32=_nan_like(M * N, F, gpu))
    d = _lib.GemmDesc(dtype=_lib.BF16, c_dtype=_lib.BF16, layout=_lib.GEMM_NT, act=0, M=M, N=N, K=K, nb=1, nh=1, alpha=1.0, beta=0.0,
                      A=bufs["A"].data_ptr(), lda=K, B=bufs["B"].data_ptr(), ldb=K, C=bufs["C"].data_ptr(), ldc=N)
    for k, v in over.items():
        setattr(d, k, v(bufs) if callable(v) else v)
    return d, bufs


REFUSALS = [
    ("null descriptor", None, "null descriptor"),
    ("null operand", dict(A=None), "null operand"),
    ("negative size", dict(K=-1), "negative size"),
    ("bad dtype", dict(dtype=7), "bad dtype"),
    ("bad c_dtype", dict(c_dtype=7), "bad c_dtype"),
    ("16-bit output of the other type", dict(c_dtype=2), "inputs' type"),
    ("batch 0", dict(nb=0), "batch must be"),
    ("batch beyond grid.z", dict(nb=256, nh=256), "exceeds grid.z"),
    ("bad layout", dict(layout=3), "bad layout"),
    ("lda too small", dict(lda=63), "lda"),
    ("ldb too small", dict(ldb=63), "ldb"),
    ("ldb too small for NN", dict(layout=1, ldb=63), "ldb"),
    ("lda too small for TN", dict(layout=2, lda=63, ldb=64), "lda"),
    ("ldc too small", dict(ldc=63), "ldc"),
    ("ldr too small", dict(residual=lambda b: b["R"].data_ptr(), ldr=63), "ldr"),
    ("misaligned workspace", dict(workspace=lambda b: b["W"].data_ptr() + 4, workspace_bytes=1 << 19), "workspace"),
    ("dbias with a batch", dict(layout=2, ldb=64, lda=64, nb=2, dbias=lambda b: b["D"].data_ptr()), "dbias"),
    ("dbias on NT", dict(dbias=lambda b: b["D"].data_ptr()), "dbias"),
    ("dbias on NN", dict(layout=1, ldb=64, dbias=lambda b: b["D"].data_ptr()), "dbias"),
    ("grad_ref with a batch", dict(nb=2, grad_ref=lambda b: b["R"].data_ptr(), grad_act=1), "grad_ref"),
    ("grad_ref with an fp32 output", dict(c_dtype=0, C=lambda b: b["C32"].data_ptr(), grad_ref=lambda b: b["R"].data_ptr(), grad_act=1),
     "grad_ref"),
]


@pytest.mark.parametrize("name,over,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_invalid_descriptors_are_refused(gpu, name, over, msg):
    from d2r_amd import D2RError, _lib
    from d2r_amd.functional import _stream
    d, bufs = _refusal_desc(gpu, **(over or {}))
    c0, c32 = bufs["C"].clone(), bufs["C32"].clone()
    torch.cuda.synchronize()
    with pytest.raises(D2RError) as ei:
        _lib.call("d2r_gemm", None if over is None else C.byref(d), _stream())
    assert "status -1" in str(ei.value), str(ei.value)
    text = _L().d2r_last_error().decode()
    assert msg in text, f"d2r_last_error: {text!r}"
    torch.cuda.synchronize()
    assert torch.equal(_bits(bufs["C"]), _bits(c0)) and torch.equal(_bits(bufs["C32"]), _bits(c32)), "a refused call wrote C"


# ---------------------------------------------------------------------------------------------------------------------------------
# weight-shared linears: one parameter at two call sites in one backward pass (deferred, grouped weight gradients)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, BF, H], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("tokens", [(300, 517), (300, 300)], ids=["different_counts", "same_count"])
def test_weight_shared_linear_accumulates_both_weight_gradients(gpu, dt, tokens):
    """A 768 x 768 Linear whose fp32 master weight and bias have flat gradient sinks (as ParamStore gives them), applied to two inputs
    on one stream: both products must land in the sinks, on top of what they held.  With different token counts the two deferred
    products have different shape keys; they must still not meet in one grouped launch (which refuses two problems with one output)."""
    from d2r_amd import functional as F_
    E = 768
    gen = torch.Generator().manual_seed(7 + tokens[1])
    w0 = torch.randn(E, E, generator=gen) * 0.03
    b0 = torch.randn(E, generator=gen) * 0.1
    xs = [torch.randn(t, E, generator=gen).to(dt) for t in tokens]
    gys = [torch.randn(t, E, generator=gen).to(dt) for t in tokens]
    gw0 = torch.randn(E, E, generator=gen)  # the sinks already hold gradient: they must be accumulated into
    gb0 = torch.randn(E, generator=gen)
    w = w0.to(gpu).requires_grad_(True)
    b = b0.to(gpu).requires_grad_(True)
    w._d2r_grad = gw0.to(gpu)
    b._d2r_grad = gb0.to(gpu)
    wc = w.detach().to(dt) if dt != F else None
    ys = [F_.linear(x.to(gpu), w, b, wc) for x in xs]
    torch.autograd.backward(ys, [g.to(gpu) for g in gys])
    F_.flush_wgrads()
    torch.cuda.synchronize()
    x64, g64 = [x.double() for x in xs], [g.double() for g in gys]
    ref_w = gw0.double() + sum(g.t() @ x for g, x in zip(g64, x64))
    ref_b = gb0.double() + sum(g.sum(0) for g in g64)
    abs_w = sum(g.abs().t() @ x.abs() for g, x in zip(g64, x64))
    abs_b = sum(g.abs().sum(0) for g in g64)
    T = sum(tokens)
    bw = 2.0 * T * EPS32 * abs_w + 4 * EPS32 * (gw0.double().abs() + ref_w.abs()) + TINY
    bb = 2.0 * T * EPS32 * abs_b + 4 * EPS32 * (gb0.double().abs() + ref_b.abs()) + TINY
    got_w, got_b = w._d2r_grad.double().cpu(), b._d2r_grad.double().cpu()
    assert bool(((got_w - ref_w).abs() <= bw).all()), f"weight sink: max err {float((got_w - ref_w).abs().max()):.3e}"
    assert bool(((got_b - ref_b).abs() <= bb).all()), f"bias sink: max err {float((got_b - ref_b).abs().max()):.3e}"
