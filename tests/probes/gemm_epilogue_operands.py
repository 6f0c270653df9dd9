"""What a second epilogue operand costs a 16-bit GEMM launch: one shape on one kernel, timed with events in one process

  plain                  C = A B
  bias                   C = A B + bias
  R                      C = A B + R                    (residual)
  G relu                 C = (A B) * relu'(G)           (gradient reference; relu' costs no arithmetic: what is left is the fetch)

  python tests/probes/gemm_epilogue_operands.py [--dtype fp16] LAYOUT:M:N:K:TILE ...

TILE is a d2r_gemm_tuning tile code (6: 128 x 128 on eight waves, 5: 128 x 64, 11: 256 x 256, -1: the automatic rule); the kernel
variant that served the launch is printed with every row.  Without arguments: the four shapes of profiles/gemm_epilogue_fetch.log.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from d2r_amd import _lib  # noqa: E402
from d2r_amd.functional import _stream  # noqa: E402

DEFAULT = ["NN:4096:3072:768:11", "NN:6304:3072:768:6", "NT:4096:768:768:6", "NT:6304:768:3072:6"]
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="fp16")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("shapes", nargs="*", default=DEFAULT)
a = ap.parse_args()
dev = torch.device("cuda", 0)
dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
code = {"bf16": _lib.BF16, "fp16": _lib.F16}[a.dtype]
lib = _lib.load()
RELU = 1


def variant_of(desc):
    cap = 8
    fam, fl, by, ms = (C.c_int * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_float * cap)()
    lib.d2r_gemm_timer(1)
    _lib.call("d2r_gemm", C.byref(desc), _stream())
    n = lib.d2r_gemm_timer_read(fam, fl, by, ms, cap)
    lib.d2r_gemm_timer(0)
    return [fam[i] // 100 for i in range(n)]


def time_us(desc):
    for _ in range(10):
        _lib.call("d2r_gemm", C.byref(desc), _stream())
    best = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            _lib.call("d2r_gemm", C.byref(desc), _stream())
        e1.record()
        e1.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    best.sort()
    return best[len(best) // 2], best[0], best[-1]


print("%-24s %-8s %7s %9s %9s %9s %8s" % ("shape", "operand", "variant", "median us", "min us", "max us", "TFLOP/s"))
for spec in a.shapes:
    lay_s, M, N, K, tile = spec.split(":")
    M, N, K, tile = int(M), int(N), int(K), int(tile)
    lay = {"NT": _lib.GEMM_NT, "NN": _lib.GEMM_NN}[lay_s]
    A = (torch.randn(M, K, device=dev) * 0.05).to(dt)
    B = (torch.randn((N, K) if lay == _lib.GEMM_NT else (K, N), device=dev) * 0.05).to(dt)
    Cc = torch.empty(M, N, device=dev, dtype=dt)
    R = torch.randn(M, N, device=dev).to(dt)
    G = torch.randn(M, N, device=dev).to(dt)
    bias = torch.randn(N, device=dev)
    lib.d2r_gemm_tuning(1, 1, tile)
    base = None
    for name in ("plain", "bias", "R", "G relu"):
        d = _lib.GemmDesc(dtype=code, c_dtype=code, layout=lay, act=0, M=M, N=N, K=K, nb=1, nh=1, alpha=1.0, beta=0.0,
                          A=A.data_ptr(), lda=A.shape[1], B=B.data_ptr(), ldb=B.shape[1], C=Cc.data_ptr(), ldc=N)
        if name == "bias":
            d.bias = bias.data_ptr()
        if name == "R":
            d.residual, d.ldr = R.data_ptr(), N
        if name == "G relu":
            d.grad_ref, d.grad_act = G.data_ptr(), RELU
        var = variant_of(d)
        med, lo, hi = time_us(d)
        base = med if base is None else base
        print("%-24s %-8s %7s %9.2f %9.2f %9.2f %8.0f   %+6.2f us" % ("%s %dx%dx%d" % (lay_s, M, N, K), name, ",".join(map(str, var)), med, lo, hi,
                                                                    2.0 * M * N * K / med / 1e6, med - base), flush=True)
    lib.d2r_gemm_tuning(1, 1, -1)
