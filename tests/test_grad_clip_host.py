"""CPU: the host side of gradient clipping by global norm (FusedAdamW(max_grad_norm=...)) - the --max_grad_norm flag, the
argument checks of the norm entry points, and the range accounting of the sharded optimiser: every element of every parameter
group is added into the norm by exactly one rank."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_max_grad_norm_flag():
    from d2r_amd.run import build_parser
    p = build_parser()
    assert p.parse_args([]).max_grad_norm == 0.0
    assert p.parse_args(["--max_grad_norm", "1.5"]).max_grad_norm == 1.5
    assert p.parse_args(["--max_grad_norm", "0"]).max_grad_norm == 0.0
    for bad in ("-1", "-1e-9", "nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["--max_grad_norm", bad])


def test_intersect_ranges_merges_adjacent_parts():
    from d2r_amd.params import intersect_ranges
    groups = [(0, 16), (16, 40), (40, 64)]
    assert intersect_ranges(groups) == [(0, 64)]
    assert intersect_ranges(groups, [(8, 24), (48, 52)]) == [(8, 24), (48, 52)]
    assert intersect_ranges(groups, [(60, 100)]) == [(60, 64)]
    assert intersect_ranges([(0, 0)], None) == []


def _group_ranges(rng, n_groups):
    """A partition of [0, n) into ALIGN-aligned contiguous group ranges, as ParamStore lays them out."""
    from d2r_amd.params import ALIGN
    sizes = [int(rng.integers(1, 400)) * ALIGN for _ in range(n_groups)]
    out, a = [], 0
    for s in sizes:
        out.append((a, a + s))
        a += s
    return out, a


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_sharded_norm_ranges_count_every_element_once(world):
    from d2r_amd.dp import bucket_bounds, norm_element_ranges, stripe_bounds
    from d2r_amd.params import intersect_ranges
    rng = np.random.default_rng(world)
    for trial in range(12):
        groups, n = _group_ranges(rng, int(rng.integers(1, 5)))
        # bucket sizes that are multiples of 4 * world and ones that are not (rounded by bucket_bounds), down to the minimum
        for bucket in (1, 4 * world, 4 * world + 3, 37, 1000, int(rng.integers(1, n + 1)), n, 2 * n):
            bounds = bucket_bounds(n, bucket, world, True)
            assert bounds[0][0] == 0 and bounds[-1][1] == n
            assert all(b - a == bounds[0][1] - bounds[0][0] for a, b in bounds[:-1])
            count = np.zeros(n, dtype=np.int64)
            for rank in range(world):
                stripes = [stripe_bounds(a, b, rank, world) for a, b in bounds]
                updated = [r for own, _, tail in stripes for r in (own, tail) if r[1] > r[0]]  # DataParallel's element_ranges
                counted = intersect_ranges(groups, norm_element_ranges(stripes, rank))
                for lo, hi in counted:
                    assert lo % 4 == 0, (world, bucket, rank, lo)  # d2r_grad_sumsq takes 16-byte aligned range starts
                    assert any(a <= lo and hi <= b for a, b in intersect_ranges(updated)), "counts an element it does not update"
                    count[lo:hi] += 1
            want = np.zeros(n, dtype=np.int64)
            for a, b in groups:
                want[a:b] = 1
            assert np.array_equal(count, want), (world, bucket, n, np.flatnonzero(count != want)[:8])


def test_norm_entry_points_check_their_arguments():
    from d2r_amd import _lib
    lib = _lib.load()
    slab = (ctypes.c_double * _lib.GRAD_NORM_PARTS)()
    g = (ctypes.c_float * 64)()
    g_al = ctypes.addressof(g) + (-ctypes.addressof(g)) % 16
    rg = (ctypes.c_int64 * 2)(0, 8)
    # a slab too small for one call's partials
    assert lib.d2r_grad_sumsq(g_al, rg, 1, slab, _lib.GRAD_NORM_PARTS - 1, None) == -1
    assert b"slab" in lib.d2r_last_error()
    # a misaligned gradient, a misaligned range start, a reversed range, too many ranges, null pointers
    assert lib.d2r_grad_sumsq(g_al + 4, rg, 1, slab, _lib.GRAD_NORM_PARTS, None) == -1
    assert lib.d2r_grad_sumsq(g_al, (ctypes.c_int64 * 2)(2, 8), 1, slab, _lib.GRAD_NORM_PARTS, None) == -1
    assert lib.d2r_grad_sumsq(g_al, (ctypes.c_int64 * 2)(8, 4), 1, slab, _lib.GRAD_NORM_PARTS, None) == -1
    assert lib.d2r_grad_sumsq(g_al, rg, _lib.GRAD_NORM_MAX_RANGES + 1, slab, _lib.GRAD_NORM_PARTS, None) == -1
    assert lib.d2r_grad_sumsq(None, rg, 1, slab, _lib.GRAD_NORM_PARTS, None) == -1
    assert lib.d2r_grad_sumsq(g_al, None, 1, slab, _lib.GRAD_NORM_PARTS, None) == -1
    out = (ctypes.c_float * 2)()
    assert lib.d2r_grad_norm_finish(slab, 0, 1.0, None, 1.0, out, None, None) == -1  # no partials
    assert lib.d2r_grad_norm_finish(slab, 16, 1.0, None, 0.0, out, None, None) == -1  # clipping to 0 is "off", not a norm
    assert lib.d2r_grad_norm_finish(None, 16, 1.0, None, 1.0, out, None, None) == -1
    # the clip-aware AdamW entries need the coefficient
    assert lib.d2r_adamw_step_clip(g_al, g_al, g_al, g_al, None, 1, 8, ctypes.c_float(1e-3), ctypes.c_float(0.9),
                                   ctypes.c_float(0.999), ctypes.c_float(1e-8), ctypes.c_float(0.0), 1, ctypes.c_float(1.0), None,
                                   None, None) == -1
    assert lib.d2r_adamw_step_dev_clip(g_al, g_al, g_al, g_al, None, 1, 8, g_al, ctypes.c_float(0.9), ctypes.c_float(0.999),
                                       ctypes.c_float(1e-8), ctypes.c_float(0.0), None, None, None) == -1
    assert b"d2r_adamw_step_dev_clip" in lib.d2r_last_error()
