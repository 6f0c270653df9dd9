"""CPU: the host side of the weight EMA (FusedAdamW(ema_decay=...)) - the --ema_decay flag, the decay schedule against its closed
form (and against torch_ema where that package is installed), and the argument checks of d2r_adamw_step_ema,
d2r_adamw_step_dev_ema and d2r_swap_f32, all of which refuse before anything is enqueued."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_ema_decay_flag():
    from d2r_amd.run import build_parser
    p = build_parser()
    assert p.parse_args([]).ema_decay == 0.0
    assert p.parse_args(["--ema_decay", "0.999"]).ema_decay == 0.999
    assert p.parse_args(["--ema_decay", "0"]).ema_decay == 0.0
    for bad in ("1", "1.0", "1.5", "-0.1", "-1e-9", "nan", "inf"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ema_decay", bad])
    assert "(1 + t) / (10 + t)" in " ".join(p.format_help().split())  # the warm-up is documented where the flag is


def test_decay_schedule_matches_the_closed_form():
    from d2r_amd.params import ema_one_minus_decay
    for D in (0.5, 0.9, 0.99, 0.999, 0.9999):
        for t in list(range(1, 200)) + [1000, 8990, 8991, 8992, 10 ** 6]:
            d_t = min(D, (1 + t) / (10 + t))
            got = ema_one_minus_decay(D, t)
            assert got == 1.0 - d_t, (D, t, got)
            assert 0.0 < np.float32(got) <= 1.0  # what the entry point accepts
    # the warm-up rules while (1 + t) / (10 + t) < D: t < (10 D - 1) / (1 - D); 0.999 takes over at step 8990
    assert ema_one_minus_decay(0.999, 1) == 1.0 - 2.0 / 11.0
    assert ema_one_minus_decay(0.999, 8989) > 1.0 - 0.999 and ema_one_minus_decay(0.999, 8991) == 1.0 - 0.999
    assert ema_one_minus_decay(0.5, 8) == 0.5 and ema_one_minus_decay(0.5, 7) > 0.5  # (1 + 8) / (10 + 8) = 0.5


def test_decay_schedule_matches_torch_ema():
    torch_ema = pytest.importorskip("torch_ema")
    import torch
    from d2r_amd.params import ema_one_minus_decay
    D = 0.9
    p = torch.nn.Parameter(torch.tensor([1.0], dtype=torch.float64))
    ema = torch_ema.ExponentialMovingAverage([p], decay=D, use_num_updates=True)
    e = 1.0
    for t in range(1, 40):
        with torch.no_grad():
            p.add_(0.37 * t)
        ema.update()
        e = e + ema_one_minus_decay(D, t) * (float(p) - e)
        assert abs(float(ema.shadow_params[0]) - e) <= 1e-12 * abs(e), (t, float(ema.shadow_params[0]), e)


def test_optimizer_refuses_a_decay_outside_the_range():
    from d2r_amd.params import FusedAdamW
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(None, lr=1e-3, ema_decay=bad)


def _f(x):
    return ctypes.c_float(x)


def test_ema_entry_points_check_their_arguments():
    from d2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 96)()
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16  # w, g, m, v (never dereferenced: every call below is refused)
    e = a + 128                                                  # a separate, 16-byte aligned EMA range
    hyper = (0.9, 0.999, 1e-8, 0.0)

    def eager(ema, omd, w=a):
        return lib.d2r_adamw_step_ema(w, a, a, a, None, 1, 8, _f(1e-3), *map(_f, hyper), 1, _f(1.0), None, None, ema, _f(omd), None)

    def dev(ema, d_omd, w=a):
        return lib.d2r_adamw_step_dev_ema(w, a, a, a, None, 1, 8, a, *map(_f, hyper), None, None, ema, d_omd, None)

    assert eager(None, 0.1) == -1 and b"d2r_adamw_step_ema" in lib.d2r_last_error()       # null ema
    assert eager(e + 4, 0.1) == -1 and b"aligned" in lib.d2r_last_error()                  # misaligned ema
    assert eager(a, 0.1) == -1                                                             # ema == w
    assert eager(e, 1.5) == -1 and b"[0, 1]" in lib.d2r_last_error()                       # factor outside [0, 1]
    assert eager(e, -0.25) == -1 and eager(e, float("nan")) == -1
    assert eager(e, 0.1, w=None) == -1
    assert dev(None, a) == -1 and b"d2r_adamw_step_dev_ema" in lib.d2r_last_error()
    assert dev(e + 4, a) == -1 and b"aligned" in lib.d2r_last_error()
    assert dev(a, a) == -1
    assert dev(e, None) == -1 and b"d_ema_one_minus_decay" in lib.d2r_last_error()         # null device factor
    # an empty range passes every check and launches nothing
    assert lib.d2r_adamw_step_ema(a, a, a, a, None, 1, 0, _f(1e-3), *map(_f, hyper), 1, _f(1.0), None, None, e, _f(0.1), None) == 0
    assert lib.d2r_adamw_step_dev_ema(a, a, a, a, None, 1, 0, a, *map(_f, hyper), None, None, e, a, None) == 0


def test_swap_checks_its_arguments():
    from d2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 96)()
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    assert lib.d2r_swap_f32(None, a, 8, None) == -1 and b"d2r_swap_f32" in lib.d2r_last_error()
    assert lib.d2r_swap_f32(a, None, 8, None) == -1
    assert lib.d2r_swap_f32(a, a + 64, -1, None) == -1
    for off in (0, 4, 28, -28):  # the same range, and ranges of 8 floats that share 7, 1 and 1 elements
        assert lib.d2r_swap_f32(a + 64, a + 64 + off, 8, None) == -1 and b"overlap" in lib.d2r_last_error(), off
    assert lib.d2r_swap_f32(a, a + 32, 0, None) == 0  # nothing to do, nothing launched
    assert lib.d2r_swap_f32(a, a, 0, None) == 0
