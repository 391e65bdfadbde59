"""The inputs of the exact train-scan tests, in one place: test_scan_exact_gpu.py and
test_trainscan_exact_gpu.py run them on the device, test_exact_scan_cpu.py asserts on any
box that every one of them keeps the exactness budget (exact_scan.budget_bits < 53).

A case is (table name, d, k, i0, n, window, carries): dt = d / 2**k, window in global sample
indices or None, carries = (C1, C2) as the fp64 values the kernels get (multiples of 2**-k).
"""
from __future__ import annotations

import functools
import itertools

from cuda_v_mpi_amd.utils import exact_scan as xs

TILE = 4096
BLOCK = 256 * TILE  # samples per block of 256 tiles (trainscan.hip kB * kTile)


@functools.lru_cache(maxsize=None)
def table(name: str):
    """'jag7': 2048 entries in [-7, 7]; 'jag1': 2048 entries in {-1, 0, 1} (class-level runs)."""
    return {"jag7": lambda: xs.jagged_table(2048, 7, seed=20240),
            "jag1": lambda: xs.jagged_table(2048, 1, seed=1801)}[name]()


# dt as (d, k): 1/64 spans 64 segments per tile (table read unstaged from global memory);
# 1/128 and 1/1024 stage LDS windows of 34 and 6 entries; 1 puts every sample on a knot and
# the slice past the table's end after 2047 samples; 3/1024 and 5/64 are not 1/sps (3-kernel
# path, tiles that start mid-segment).
DTS = {"1/64": (1, 6), "1/128": (1, 7), "1/1024": (1, 10), "1": (1, 0), "3/1024": (3, 10),
       "5/64": (5, 6)}
CLOSED = ("1/64", "1/128", "1/1024", "1")  # dt = 1/sps: closed-form tile sums, fold applies
NS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, BLOCK + TILE + 1)
I0S = (0, 37)
ALGOS = ("fused", "fold", "onepass", "lookback")  # lookback: interp_scan, then inclusive_scan


def algo_dts():
    """(algo, dt name) pairs of 4a: the fold only where dt = 1/sps."""
    return [(a, dt) for a in ALGOS for dt in DTS if a != "fold" or dt in CLOSED]


def sampling_cases(dt: str):
    d, k = DTS[dt]
    return [("jag7", d, k, i0, n, None, (0.0, 0.0)) for n, i0 in itertools.product(NS, I0S)]


# 4b: most of the slice is the flat tail past the table's end; four blocks of tiles
FLAT_TAIL = ("jag7", 1, 6, 0, 3 * 2**20 + TILE + 1, None, (0.0, 0.0))

# 4c: fill windows on a slice of three full tiles and a partial one, starting at i0 = 5000
WIN_I0, WIN_N = 5000, 3 * TILE + 100
WINDOWS = {
    "inside_one_tile": (WIN_I0 + TILE + 100, WIN_I0 + TILE + 900),
    "cuts_both_ends": (WIN_I0 + 1000, WIN_I0 + 2 * TILE + 2000),  # tile 1 alone is wholly inside
    "whole_tiles": (WIN_I0 + TILE, WIN_I0 + 3 * TILE),            # edges on tile boundaries
    "empty": (WIN_I0 + 500, WIN_I0 + 500),
    "before_slice": (100, WIN_I0),
    "after_slice": (WIN_I0 + WIN_N, WIN_I0 + WIN_N + 5000),
}
WINDOW_DTS = ("1/64", "1/1024", "3/1024")


def window_cases(dt: str):
    d, k = DTS[dt]
    return {w: ("jag7", d, k, WIN_I0, WIN_N, win, (0.0, 0.0)) for w, win in WINDOWS.items()}


# 4d: rank carries (multiples of 1/4: exact in units of 2**-k for k >= 2)
CARRIES = (12345.5, -987654.25)
CARRY_DTS = ("1/64", "1/1024", "3/1024")


def carry_cases(dt: str):
    d, k = DTS[dt]
    return [("jag7", d, k, 37, n, None, CARRIES) for n in (2 * TILE + 1, BLOCK + TILE + 1)]


# 4f: more than 256 blocks of tiles; the samples that are not zero sit in 2**13 in the middle
BIG_N = 2**28 + 3 * TILE + 17
BIG = ("jag7", 1, 6, 0, BIG_N, (BIG_N // 2, BIG_N // 2 + 2**13), (0.0, 0.0))

# 5: TrainScanConfig(table = jag1, steps_per_sec, seconds): 375 tiles, two blocks
CLASS_SPS, CLASS_K, CLASS_SECONDS = 1024, 10, 1500
CLASS_TOTAL = CLASS_SPS * CLASS_SECONDS
# every rank's slice and every parity fill window holds a subset of these samples, and the
# rank carries are partial sums of them: this one budget bounds every world
CLASS = ("jag1", 1, CLASS_K, 0, CLASS_TOTAL, None, (0.0, 0.0))


def int_carries(case) -> tuple[int, int]:
    """The case's carries in units of 2**-k (they must be whole numbers of them)."""
    k = case[2]
    c = tuple(v * 2.0**k for v in case[6])
    assert all(v == int(v) for v in c), f"carries {case[6]} are no multiples of 2**-{k}"
    return int(c[0]), int(c[1])


def budget(case) -> float:
    name, d, k, i0, n, window, _ = case
    return xs.budget_bits(table(name), d, k, i0, n, window, int_carries(case))


def every_gpu_case():
    """(label, case) for every input the GPU tests launch."""
    for dt in DTS:
        for c in sampling_cases(dt):
            yield f"sampling dt={dt} n={c[4]} i0={c[3]}", c
    yield "flat tail", FLAT_TAIL
    for dt in WINDOW_DTS:
        for w, c in window_cases(dt).items():
            yield f"window {w} dt={dt}", c
    for dt in CARRY_DTS:
        for c in carry_cases(dt):
            yield f"carries dt={dt} n={c[4]}", c
    yield "more than 256 blocks", BIG
    yield "class level", CLASS
