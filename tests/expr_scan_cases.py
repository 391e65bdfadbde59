"""The inputs of the exact tests of the running-integral kernels (csrc/runtime/expr_scan.cpp),
in one place: test_expr_scan_gpu.py launches them (ExprScan), test_expr_scan_cpu.py asserts
on any box that each keeps its exactness budget and the tile structure the GPU tests lean on.

The family is expr_exact_cases.py's: polynomials in x with integer coefficients on grids of
step 2**-k from a dyadic lower limit. exact_riemann.expr_budget_bits bounds every partial sum
of a case's samples in any order, so every prefix sum, under any association (the thread's
serial scan, the wave and workgroup scans, the tile prefix, the rank carries), is exact in
fp64: each written value must have the bits of the integer prefix sum.

The reference is torch.cumsum over exact_riemann.exact_poly_samples in int64, computed once
per (case, rule) over the case's span and shared (read-only) by every test.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import expr_exact_cases as ec
from cuda_v_mpi_amd.utils import exact_riemann as xr

TILE = 4096                    # samples of a scan tile: 256 threads x 16 (EXPR_SCAN_TILE)
PREFIX_THREADS = 1024          # threads of the one tile-prefix workgroup

CUBIC, QUADRATIC, FULL_LANES = ec.CUBIC, ec.QUADRATIC, ec.FULL_LANES
# more tiles than the prefix workgroup has threads: a thread walks two tiles there
LONG = ec.PolyExpr("long", "5.0-7.0*x", (5, -7), ec.Coords(12, ec.a_num_of(12), 4096 * 1027 + 5))
# more tiles than the sums pass has workgroups (2048): a workgroup walks a run of two tiles,
# 1027 runs, the last of one ragged tile
WIDE = ec.PolyExpr("wide", "7.0*x+5.0", (5, 7), ec.Coords(12, ec.a_num_of(12), 4096 * 2052 + 7))
POLY_CASES = (CUBIC, QUADRATIC, FULL_LANES, LONG, WIDE)
# samples 2^33 + 1 .. of the 2^40-sample rule of step 1 on [0, 2^40]: one tile and 1025
PAST_2_32 = ec.PolyExpr("past-2^32", "7.0*x-5.0", (-5, 7),
                        ec.Coords(0, 0, 2**40, 2**33 + 1, 4096 + 1025))
ALL_CASES = POLY_CASES + (PAST_2_32,)

# (whole tiles, samples past them) of each case's span
TILE_CENSUS = {"cubic": (0, 2085), "quadratic": (8, 37), "full-lanes": (512, 3),
               "long": (1027, 5), "wide": (2052, 7), "past-2^32": (1, 1025)}
# expr_scan_shape of each span: (tiles, tiles per run, runs). Up to 2048 tiles a run is one
# tile; past 1024 runs a prefix thread walks two of them (long, wide)
SHAPES = {"cubic": (1, 1, 1), "quadratic": (9, 1, 9), "full-lanes": (513, 1, 513),
          "long": (1028, 1, 1028), "wide": (2053, 2, 1027), "past-2^32": (2, 1, 2)}
MAX_RUNS = 2048
# expr_budget_bits of each case as first computed (one decimal); past-2^32 was estimated at 49
BUDGETS = {"cubic": 46.6, "quadratic": 47.9, "full-lanes": 45.8, "long": 47.8, "wide": 49.8,
           "past-2^32": 49.1}

EDGE_BEGIN = ec.EDGE_BEGIN     # 5: an odd first sample
# either side of a thread's 16 samples, of 4 and 16 threads' worth, of one tile and of two:
# every one but 4096 and 8192 ends in a ragged tile
EDGE_COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)


def every_values(count: int) -> tuple:
    return (2, 3, 16, 37, 4096, 4097, 10000, count, count + 1)


@functools.lru_cache(maxsize=None)
def _prefix_ints(name: str, rule: str) -> np.ndarray:
    """int64 inclusive prefix sums of the case's samples over its span, in units of
    2**-poly_unit_bits (read-only)."""
    c = {k.name: k for k in ALL_CASES}[name]
    b, m = c.at.span
    s = xr.exact_poly_samples(c.coef, c.at.a_num, c.at.k, ec.OFF2[rule], b, m)
    p = torch.cumsum(s, dim=0).numpy()
    p.setflags(write=False)
    return p


def selected(begin: int, count: int, every: int) -> np.ndarray:
    """Global indices i of [begin, begin + count) with (i + 1) % every == 0, in order."""
    first = (begin // every + 1) * every - 1
    return np.arange(first, begin + count, every, dtype=np.int64)


def running_ref(c, rule: str, begin: int, count: int, every: int = 1, scale: float = 1.0,
                start: int | None = None) -> np.ndarray:
    """The fp64 values a scan of samples [begin, begin + count) must write, bit for bit: for
    each selected sample i, scale * h * sum of f(x_j) over start <= j <= i (start: where the
    sum begins; `begin` unless lower ranks' slices are carried in)."""
    b0, _ = c.at.span
    start = begin if start is None else start
    p = _prefix_ints(c.name, rule)
    i = selected(begin, count, every)
    before = int(p[start - b0 - 1]) if start > b0 else 0
    return xr.values_f64(p[i - b0] - before, xr.poly_unit_bits(c.coef, c.at.k)) \
        * 2.0 ** -c.at.k * scale


def total_ref(c, rule: str, begin: int, count: int, scale: float = 1.0) -> float:
    return ec.poly_value(c.coef, c.at, rule, begin, count, scale)


def same_bits(got, want) -> bool:
    g = np.ascontiguousarray(np.asarray(got, dtype=np.float64)).reshape(-1)
    w = np.ascontiguousarray(np.asarray(want, dtype=np.float64)).reshape(-1)
    return g.shape == w.shape and bool(np.array_equal(g.view(np.uint64), w.view(np.uint64)))
