"""The inputs of the exact Riemann and 2-D field tests, in one place: test_riemann_exact_gpu.py
launches them on the device, test_exact_riemann_cpu.py asserts on any box that every one of
them keeps its exactness budget (exact_riemann.*_budget_bits), that the table cases reach all
three tile paths, and runs the host engine on them.

1-D coordinates: h = 2**-k, a = A0 - 5 h with A0 = -2.625 (so no tile boundary falls on a
knot: a is no multiple of 64 h for any k here), b = a + n h, n = (entries + 4) 2**k + tail
with a tail that is no multiple of 64. The domain runs from 2.6 below the table's first
entry to 2.4 past its last one; a polynomial's from -R to about R.
"""
from __future__ import annotations

import functools
import itertools
from typing import NamedTuple

from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.parallel.decomposition import rank_slice
from cuda_v_mpi_amd.utils import exact_riemann as xr

OFF2 = {"left": 0, "mid": 1, "right": 2}
RULES = ("left", "mid", "right")
KS = (3, 5, 6, 7, 8)
GRIDS = (1, 3, 7, 130)
WORLD = 7           # rank slices: rank_slice(n, r, 7)


@functools.lru_cache(maxsize=None)
def table(name: str):
    """'t200' / 't2048': 200 / 2048 (kMaxTable) integer entries in [-7, 7], equal and not
    zero at the end so samples past the table still count."""
    return {"t200": lambda: xr.jagged_table(200, 7, seed=355),
            "t2048": lambda: xr.jagged_table(2048, 7, seed=950)}[name]()


def a_num_of(k: int) -> int:
    """a = -2.625 - 5 h in units of 2**-(k+1) (k >= 3: 2.625 = 21 / 8)."""
    return -(21 << (k - 2)) - 10


class TableCase(NamedTuple):
    tab: str
    k: int
    rule: str
    dtype: str
    div: str
    grid: int
    fused: bool
    tail: int = 37
    rank: int | None = None    # rank_slice(n, rank, WORLD), or the whole rule

    @property
    def id(self) -> str:
        s = f"{self.tab}-k{self.k}-{self.rule}-{self.dtype}-{self.div}-g{self.grid}"
        s += "-fused" if self.fused else "-2k"
        return s + (f"-r{self.rank}of{WORLD}" if self.rank is not None else "")


def n_of(c) -> int:
    return ((len(table(c.tab)) + 4) << c.k) + c.tail


def span(c) -> tuple[int, int]:
    """(i_begin, n_local) of the launch."""
    return (0, n_of(c)) if c.rank is None else rank_slice(n_of(c), c.rank, WORLD)


def table_spec(c) -> integrands.IntegrandSpec:
    a = a_num_of(c.k) * 2.0 ** -(c.k + 1)
    return integrands.table([float(v) for v in table(c.tab)], a=a, b=a + n_of(c) * 2.0 ** -c.k)


def table_ref(c) -> float:
    """h * sum, exactly: the fp64 every launch of the case must return."""
    i0, m = span(c)
    tot = xr.exact_table_sum(table(c.tab), a_num_of(c.k), c.k, OFF2[c.rule], i0, m)
    return xr.value_f64(tot, c.k + 1) * 2.0 ** -c.k


def table_budget(c) -> dict:
    i0, m = span(c)
    return xr.table_budget_bits(table(c.tab), a_num_of(c.k), c.k, OFF2[c.rule], i0, m, 0, n_of(c))


def table_census(c) -> dict:
    i0, m = span(c)
    return xr.table_tile_census(table(c.tab), a_num_of(c.k), c.k, OFF2[c.rule], i0, m)


def _table_cases() -> list:
    out = []
    cyc = itertools.cycle(GRIDS)
    # every step x rule x dtype on the series (segment-line) tiles; the grids and the
    # fused / two-kernel forms take turns
    for j, (k, rule, dtype) in enumerate(itertools.product(KS, RULES, ("fp64", "fp32"))):
        out.append(TableCase("t200", k, rule, dtype, "series", next(cyc), j % 3 != 0))
    # the per-sample (ieee) tiles
    for j, (k, dtype) in enumerate(itertools.product((3, 6, 8), ("fp64", "fp32"))):
        out.append(TableCase("t200", k, RULES[j % 3], dtype, "ieee", next(cyc), j % 2 == 0))
    # the largest table the kernels stage (kMaxTable entries)
    for j, (k, dtype) in enumerate(itertools.product((5, 8), ("fp64", "fp32"))):
        out.append(TableCase("t2048", k, RULES[(j + 1) % 3], dtype, "series", (130, 7)[j % 2],
                             j % 2 == 0))
    out.append(TableCase("t2048", 6, "mid", "fp64", "ieee", 130, True))
    out.append(TableCase("t2048", 6, "right", "fp32", "ieee", 3, False))
    # rank slices, each against the reference of its own samples (tails chosen so that some
    # slices begin on odd samples: asserted in test_exact_riemann_cpu.py)
    for r in range(WORLD):
        out.append(TableCase("t200", 7, RULES[r % 3], "fp32", "series", GRIDS[r % 4], r % 2 == 0,
                             tail=33, rank=r))
    # (ranks chosen with care: from k = 6 up every kinked tile of a launch has its knot at the
    # same place, the kinks' slope changes telescope, and a slice that begins and ends on equal
    # slopes — rank 6 does — is blind to a wrong kink weight: exact_riemann.table_kink_slope_sums,
    # asserted not zero for every case in test_exact_riemann_cpu.py)
    for r in (1, 3, 5):
        out.append(TableCase("t2048", 7, RULES[r % 3], "fp64", "series", GRIDS[r % 4], r % 4 == 1,
                             tail=33, rank=r))
    return out


TABLE_CASES = _table_cases()
FP32_SERIES = [c for c in TABLE_CASES if c.dtype == "fp32" and c.div == "series"]
FP32_SLICES = [c for c in FP32_SERIES if c.rank is not None]
FP32_WHOLE = [c for c in FP32_SERIES if c.rank is None]

# plans (chained batch, multi-step launch with its closing kernel, one-step batches) and
# loopback ranks: one table case per dtype, kink-bearing (k = 7: half the tiles straddle a
# knot). A plan never launches more workgroups than ceil(tiles / block): 4105 tiles keep the
# 5 workgroups asked for at 1024 threads too (12 rounds and a remainder at 64).
PLAN_CASES = {dt: TableCase("t2048", 7, "mid", dt, "series", 5, True, tail=33)
              for dt in ("fp64", "fp32")}
PLAN_BLOCKS = (64, 256, 1024)
PLAN_STEPS = 8
LOOPBACK_CASE = TableCase("t200", 8, "left", "fp64", "series", 0, True, tail=33)
LOOPBACK_WORLDS = (2, 3)


# ------------------------------------------------------------------------------ polynomial
class PolyCase(NamedTuple):
    coef: tuple          # integer coefficients, |c| <= 7 (zeros appended: a wider bucket)
    k: int
    R: int               # the domain is [-R - 5 h - 1/8, about R]
    rule: str
    dtype: str
    div: str
    grid: int
    rank: int | None = None

    @property
    def id(self) -> str:
        s = f"nc{len(self.coef)}-k{self.k}-{self.rule}-{self.dtype}-{self.div}-g{self.grid}"
        return s + (f"-r{self.rank}of{WORLD}" if self.rank is not None else "")


def poly_a_num(c) -> int:
    """a = -R - 1/8 - 5 h in units of 2**-(k+1)."""
    return -(c.R << (c.k + 1)) - (1 << (c.k - 2)) - 10


def poly_n(c) -> int:
    return ((2 * c.R) << c.k) + 37


def poly_span(c) -> tuple[int, int]:
    return (0, poly_n(c)) if c.rank is None else rank_slice(poly_n(c), c.rank, WORLD)


def poly_spec(c) -> integrands.IntegrandSpec:
    a = poly_a_num(c) * 2.0 ** -(c.k + 1)
    return integrands.poly([float(v) for v in c.coef], a=a, b=a + poly_n(c) * 2.0 ** -c.k)


def poly_ref(c) -> float:
    i0, m = poly_span(c)
    tot = xr.exact_poly_sum(c.coef, poly_a_num(c), c.k, OFF2[c.rule], i0, m)
    return xr.value_f64(tot, xr.poly_unit_bits(c.coef, c.k)) * 2.0 ** -c.k


def poly_budget(c) -> dict:
    i0, m = poly_span(c)
    return xr.poly_budget_bits(c.coef, poly_a_num(c), c.k, OFF2[c.rule], i0, m, 0, poly_n(c))


DEG2 = (3, -5, 7)           # k = 10 on [-16, 16]: 32 805 samples, two tile rounds at 256 lanes
DEG3 = (-6, 7, -3, 5)       # k = 7 on [-8, 8]: 2 085 samples
DEG1 = (5, -7)              # fp32: k = 6 on [-64, 64]
POLY_GRIDS = (1, 3)


def _pad(coef: tuple, nc: int) -> tuple:
    return tuple(coef) + (0,) * (nc - len(coef))


def _poly_cases() -> list:
    out = []
    shapes = [(DEG2, 10, 16), (DEG3, 7, 8)]
    # both polynomials as they are: series and ieee, three rules, two grids, one slice
    for (coef, k, R), div in itertools.product(shapes, ("series", "ieee")):
        for j, rule in enumerate(RULES):
            out.append(PolyCase(coef, k, R, rule, "fp64", div, POLY_GRIDS[j % 2]))
        out.append(PolyCase(coef, k, R, "mid", "fp64", div, POLY_GRIDS[1], rank=3))
    # every coefficient bucket: series 4, 6, 7, 8 wide, Horner 4, 8, 16 wide (9 coefficients)
    for nc, (coef, k, R) in itertools.product((4, 6, 7, 8, 9), shapes):
        if nc == len(coef):
            continue
        for j, div in enumerate(("series", "ieee")):
            out.append(PolyCase(_pad(coef, nc), k, R, RULES[(nc + j) % 3], "fp64", div,
                                POLY_GRIDS[(nc + j) % 2]))
    for div in ("series", "ieee"):
        for j, rule in enumerate(RULES):
            out.append(PolyCase(DEG1, 6, 64, rule, "fp32", div, POLY_GRIDS[j % 2]))
        out.append(PolyCase(DEG1, 6, 64, "left", "fp32", div, POLY_GRIDS[0], rank=5))
    return out


POLY_CASES = _poly_cases()
# the in-launch close of a multi-step batch (the table's plans keep the closing kernel)
POLY_PLAN_CASE = PolyCase(DEG2, 10, 16, "mid", "fp64", "series", 5)


# ------------------------------------------------------------------------------ 2-D field
@functools.lru_cache(maxsize=None)
def field(name: str):
    """Integer ny x nx tables in [-7, 7]. 'f37x53' and 'f200x300' are the issue's; 3 divides
    neither 52 nor 199 nor 299, so the rates with a 3 in them (3/8, 3/2) can only run along y
    of 'f37x53' there; 'f40x55' (39 x 54 cells) takes them on both axes."""
    import numpy as np

    ny, nx, seed = {"f37x53": (37, 53, 11), "f200x300": (200, 300, 12),
                    "f40x55": (40, 55, 13)}[name]
    return np.random.default_rng(seed).integers(-7, 8, size=(ny, nx), dtype=np.int64)


class FieldCase(NamedTuple):
    tab: str
    rx: tuple            # (d, k): d / 2**k table cells per sample along x
    ry: tuple
    path: str            # the kernel the whole field must run: "stream" | "tile"

    @property
    def id(self) -> str:
        return f"{self.tab}-x{self.rx[0]}_{1 << self.rx[1]}-y{self.ry[0]}_{1 << self.ry[1]}-{self.path}"


def field_grid(c) -> tuple[int, int]:
    ny, nx = field(c.tab).shape
    return xr.table2d_grid_of(nx, c.rx), xr.table2d_grid_of(ny, c.ry)


def field_ref(c, row0: int = 0, row1: int | None = None) -> float:
    gx, gy = field_grid(c)
    tot = xr.exact_table2d_sum(field(c.tab), c.rx, c.ry, gx, gy, row0, gy if row1 is None else row1)
    (dx, kx), (dy, ky) = c.rx, c.ry
    # unit 2**-(kx+ky+2), times sx sy = dx dy 2**-(kx+ky)
    return xr.value_f64(tot * dx * dy, kx + ky + 2) * 2.0 ** -(kx + ky)


def field_budget(c) -> float:
    gx, gy = field_grid(c)
    return xr.table2d_budget_bits(field(c.tab), c.rx, c.ry, gx, gy)


Q, E8, T8 = (1, 2), (1, 3), (3, 3)                  # 1/4, 1/8, 3/8: the row stream
HALF, ONE, T2, FOUR = (1, 1), (1, 0), (3, 1), (4, 0)  # 1/2, 1, 3/2, 4: the tile kernel
FIELD_CASES = [
    # gx = 208, 416, 432: partial 256-column workgroups; gy = 144, 96, 312, 104: partial
    # row blocks
    FieldCase("f37x53", Q, Q, "stream"),
    FieldCase("f37x53", E8, T8, "stream"),
    FieldCase("f40x55", T8, E8, "stream"),
    FieldCase("f40x55", E8, T8, "stream"),
    FieldCase("f200x300", Q, E8, "stream"),
    FieldCase("f200x300", E8, Q, "stream"),
    FieldCase("f37x53", HALF, T2, "tile"),
    FieldCase("f37x53", FOUR, ONE, "tile"),
    FieldCase("f40x55", T2, HALF, "tile"),
    FieldCase("f40x55", ONE, T2, "tile"),
    FieldCase("f200x300", HALF, ONE, "tile"),
    FieldCase("f200x300", ONE, HALF, "tile"),
]
FIELD_PHASES = (1, 3, 16)
FIELD_STEPS = 20     # steps of a multi-step launch: 3 phases run 7, 7, 6 of them, 16 run 2 or 1


def field_cuts(gy: int) -> list:
    """Odd row cuts: [0, c1), [c1, c2), [c2, gy)."""
    c1, c2 = (gy // 3) | 1, (2 * gy // 3) | 1
    return [(0, c1), (c1, c2), (c2, gy)]
