"""The cases of the bit-exact tests of the adaptive integrators (test_expr_adaptive_exact_cpu.py
and _gpu.py), each with its expression for hipRTC, the same function in numpy, and its
reference run (cuda_v_mpi_amd/utils/adaptive_exact.py), computed once per process.

Every integrand is bit-identical on any IEEE machine: each operation is exact or one correctly
rounded +, -, fabs or compare/select, and no product feeds an addition (the generated miint_f is
compiled with contraction on). The sweep's p1 is a power of two, so its product is exact. Eight
expressions in all (each costs a hipRTC compile): X, ZIG, BOX and BOX's unbounded twin source;
the sweep's KINK; and SUM, STEP_X, STEP_Y in two dimensions.
"""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass, field

import numpy as np

from cuda_v_mpi_amd.utils import adaptive_exact as ax

INF = float("inf")

# ------------------------------------------------------------------ the integrands
X = "x"
BOX = "(fabs(x-0.3)<0.5)?1.0:0.0"   # 1 on (-0.2, 0.8): two steps, a finite integral on any range
FOLDS = [0.51 / 2 ** k for k in range(10)]  # 0.51, 0.255, ...: 1023 kinks on [0, 1]


# The zigzag runs between 0 and 0.51 / 2^9 = 0.000996; lowered by ZIG_OFFSET it changes sign
# between the kinks, so R is not K again, and the sums cancel enough to show their order.
ZIG_OFFSET = 0.0003


def _zig_expr() -> str:
    e = "x"
    for c in FOLDS:
        e = f"fabs({e}-{c!r})"
    return f"{e}-{ZIG_OFFSET!r}"


ZIG = _zig_expr()
KINK = "p1*fabs(x-p0)"
SUM = "fabs(x-0.3)+fabs(y-0.3)"
STEP_X = "(x<0.3)?1.0:0.0"
STEP_Y = "(y<0.3)?1.0:0.0"


def _zig(x):
    for c in FOLDS:
        x = np.abs(x - c)
    return x - ZIG_OFFSET


F = {
    X: lambda x: x + 0.0,
    BOX: lambda x: np.where(np.abs(x - 0.3) < 0.5, 1.0, 0.0),
    ZIG: _zig,
    KINK: lambda x, p0, p1: p1 * np.abs(x - p0),
    SUM: lambda x, y: np.abs(x - 0.3) + np.abs(y - 0.3),
    STEP_X: lambda x, y: np.where(x < 0.3, 1.0, 0.0) + 0.0 * y,
    STEP_Y: lambda x, y: np.where(y < 0.3, 1.0, 0.0) + 0.0 * x,
}


# ------------------------------------------------------------------ one dimension
@dataclass(frozen=True)
class Case:
    name: str
    expr: str
    a: float
    b: float
    pins: str                                   # the path the case is there for
    opts: dict = field(default_factory=dict, compare=False, hash=False)
    buffer: bool = True                         # take the partition (and, capped, the canary)

    def __repr__(self):
        return self.name


BIG = 65537                    # nb = 257 workgroups, per = 2 in miint_adapt_prefix
BIG_B = 1.01901  # the last panel [b - b / 65537, b] holds ZIG's last kink, 0.51 (2 - 2^-9)
BIG_OPTS = dict(panels=BIG, rtol=1e-7, max_intervals=1 << 18)

CASES_1D = [
    Case("zig-1", ZIG, 0.0, 1.0, "one lane; lists grow to several mixed workgroups",
         dict(panels=1, rtol=1e-7, max_intervals=1 << 14)),
    Case("zig-3", ZIG, 0.0, 1.0, "init edges a + (w i) / 3", dict(panels=3, rtol=1e-7,
                                                                  max_intervals=1 << 14)),
    Case("zig-256", ZIG, 0.0, 1.0, "one full workgroup", dict(panels=256, rtol=1e-7,
                                                              max_intervals=1 << 14)),
    Case("zig-257", ZIG, 0.0, 1.0, "one lane alone in a second workgroup",
         dict(panels=257, rtol=1e-7, max_intervals=1 << 14)),
    Case("zig-1000", ZIG, 0.0, 1.0, "many kinks: splits and acceptances interleave in every "
         "workgroup of a round", dict(panels=1000, rtol=1e-9, max_intervals=1 << 15)),
    Case("zig-per2", ZIG, 0.0, BIG_B, "per = 2: the prefix kernel's runs, blk_off across a run",
         BIG_OPTS),
    Case("zig-per2-capped", ZIG, 0.0, BIG_B, "the capped branch at per = 2: pending K and err "
         "added, nothing split, the whole list to done[base + i]",
         dict(BIG_OPTS, max_intervals=BIG + 64)),
    Case("x-floor", X, 0.0, 1.0, "floor: a tiny rtol on x", dict(panels=64, rtol=1e-30)),
    Case("zig-floor", ZIG, 0.0, 0.02, "rtol below rounding: the floor ends thousands of branches "
         "in lists of more than ten thousand, until the cap; 49 or 51 for 50 changes the counts",
         dict(panels=20, rtol=1e-30, max_intervals=1 << 15)),
    Case("zig-depth3", ZIG, 0.0, 1.0, "forced by max_depth", dict(panels=16, max_depth=3)),
    Case("zig-depth0", ZIG, 0.0, 1.0, "max_depth = 0: one round", dict(panels=256, max_depth=0)),
    Case("box-midpoint", BOX, -1.0, 1.0, "forced by c == lo at full depth",
         dict(panels=1, max_depth=200, max_intervals=1 << 12)),
    Case("zig-reversed", ZIG, 1.0, 0.0, "a > b: negated, the partition from a down to b",
         dict(panels=3, rtol=1e-7, max_intervals=1 << 14)),
    Case("zig-atol", ZIG, 0.0, 1.0, "tol = atol (atol > rtol |S|)",
         dict(panels=16, rtol=1e-12, atol=1e-6)),
    Case("zig-rtol", ZIG, 0.0, 1.0, "tol = rtol |S| (atol below it)",
         dict(panels=16, rtol=1e-6, atol=1e-12)),
] + [
    Case(f"box-{kind}-{panels}", BOX, a, b, f"the {kind} map's eval twin from {panels} panel(s)",
         dict(panels=panels, unbounded=True, max_intervals=1 << 12))
    for kind, a, b in (("upper", -1.0, INF), ("lower", -INF, 1.0), ("both", -INF, INF))
    for panels in (1, 16)
]
BY_NAME = {c.name: c for c in CASES_1D}
WALL = {}  # name -> seconds the reference took


@functools.lru_cache(maxsize=None)
def _ref_1d(name: str) -> dict:
    c = BY_NAME[name]
    t0 = time.perf_counter()
    r = ax.adaptive_exact(F[c.expr], c.a, c.b, **c.opts)
    WALL[name] = time.perf_counter() - t0
    return r


def reference(case) -> dict:
    """The reference run of a case (of any family); shared, so leave it unchanged."""
    return {Case: _ref_1d, Case2D: _ref_2d, SweepCase: _ref_sweep}[type(case)](case.name)


# ------------------------------------------------------------------ the sweep
@dataclass(frozen=True)
class SweepCase:
    name: str
    expr: str
    a: float
    b: float
    pins: str
    params: tuple = field(compare=False, hash=False, default=())
    opts: dict = field(default_factory=dict, compare=False, hash=False)

    def __repr__(self):
        return self.name


# kinks at (2 k + 1) / 1000 that take 21 rounds and at most 170 intervals from 150 panels at
# rtol = 1e-10 (p1 is a power of two, so it scales K, err and tol alike and changes no decision)
_EASY_K = (0, 6, 13, 19, 25, 31, 38, 44, 50, 56, 63, 69, 75, 81, 88, 94, 100, 106, 113, 119,
           125, 136, 148, 161, 173, 186, 198, 211, 223, 236, 248, 261, 273, 286, 298, 311, 323,
           336, 348, 361, 373, 379, 385, 391, 398, 404, 410, 416, 423, 429, 435, 441, 448, 454,
           460, 466, 473, 479, 485, 491)
HARD_ROW, HARD_P0 = 37, 0.301  # 22 rounds and 171 intervals: the one row a cap of 170 stops


def _sweep_rows():
    """72 rows, so 18 workgroups of four waves: p1 cycles through +-1, +-2, +-0.5; every sixth
    row has its kink outside [0, 1] (linear: done in round 1), the others a kink of _EASY_K,
    row 37 the harder HARD_P0; row 40 repeats row 10."""
    scales = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)
    rows, easy = [], iter(_EASY_K)
    for k in range(72):
        p0 = 1.5 + k if k % 6 == 0 else HARD_P0 if k == HARD_ROW else (2 * next(easy) + 1) / 1000.0
        rows.append((p0, scales[(k + k // 6) % 6]))
    rows[40] = rows[10]
    return tuple(rows)


SWEEP_PANELS = 150  # chunks of 64, 64 and 22: a ragged tail in every row's chain
SWEEP = SweepCase("kink-72", KINK, 0.0, 1.0, "one wave per row over 18 workgroups; ragged "
                  "chains; rows leaving after round 1 beside rows of more than 20 rounds; a "
                  "repeated row", _sweep_rows(),
                  dict(panels=SWEEP_PANELS, rtol=1e-10, max_intervals=1 << 10))
SWEEP_CAPPED = SweepCase("kink-72-capped", KINK, 1.0, 0.0, "row 37 caps alone, the others do "
                         "not notice; a > b negates every row", SWEEP.params,
                         dict(SWEEP.opts, max_intervals=170))
SWEEP_CASES = [SWEEP, SWEEP_CAPPED]
BY_NAME_SWEEP = {c.name: c for c in SWEEP_CASES}


@functools.lru_cache(maxsize=None)
def _ref_sweep(name: str) -> dict:
    c = BY_NAME_SWEEP[name]
    t0 = time.perf_counter()
    r = ax.adaptive_sweep_exact(F[c.expr], np.array(c.params), c.a, c.b, **c.opts)
    WALL[name] = time.perf_counter() - t0
    return r


# ------------------------------------------------------------------ two dimensions
@dataclass(frozen=True)
class Case2D:
    name: str
    expr: str
    box: tuple                                  # ax, bx, ay, by
    pins: str
    opts: dict = field(default_factory=dict, compare=False, hash=False)

    def __repr__(self):
        return self.name


_O2 = dict(rtol=1e-6, max_intervals=1 << 13)
CASES_2D = [
    Case2D("sum-1x1", SUM, (0.0, 1.0, 0.0, 1.0), "a square cell on the diagonal of a square "
           "box: ex == ey ties, the rule picks x", dict(_O2, panels=(1, 1))),
    Case2D("sum-3x5", SUM, (0.0, 1.0, 0.0, 1.0), "init i = iy * 3 + ix, edges (w k) / 3 and "
           "/ 5", dict(_O2, panels=(3, 5))),
    Case2D("sum-17x16", SUM, (0.0, 1.0, 0.0, 1.0), "272 rectangles: two workgroups",
           dict(_O2, panels=(17, 16))),
    Case2D("ridge-x", SUM, (0.0, 1.0, 0.4, 1.0), "only the ridge x = 0.3 crosses the box: "
           "splits along x", dict(_O2, panels=(3, 5))),
    Case2D("ridge-y", SUM, (0.4, 1.0, 0.0, 1.0), "only the ridge y = 0.3 crosses the box: "
           "splits along y", dict(_O2, panels=(3, 5))),
    Case2D("sum-wide-box", SUM, (0.0, 2.0, 0.0, 1.0), "square cells in a 2 x 1 box: a tie "
           "goes to y (wx Wy < wy Wx)", dict(_O2, panels=(2, 1))),
    Case2D("step-x-depth", STEP_X, (0.0, 1.0, 0.0, 1.0), "the x depth (low half) reaches "
           "max_depth", dict(rtol=1e-6, max_intervals=1 << 13, panels=(3, 5), max_depth=4)),
    Case2D("step-y-depth", STEP_Y, (0.0, 1.0, 0.0, 1.0), "the y depth (high half) reaches "
           "max_depth", dict(rtol=1e-6, max_intervals=1 << 13, panels=(5, 3), max_depth=4)),
    Case2D("sum-capped", SUM, (0.0, 1.0, 0.0, 1.0), "the cap, with two workgroups' pending "
           "sums", dict(rtol=1e-6, panels=(17, 16), max_intervals=300)),
    Case2D("sum-flipped", SUM, (1.0, 0.0, 0.0, 1.0), "ax > bx: negated",
           dict(_O2, panels=(3, 5))),
]
BY_NAME_2D = {c.name: c for c in CASES_2D}


@functools.lru_cache(maxsize=None)
def _ref_2d(name: str) -> dict:
    c = BY_NAME_2D[name]
    t0 = time.perf_counter()
    r = ax.adaptive2d_exact(F[c.expr], *c.box, **c.opts)
    WALL[name] = time.perf_counter() - t0
    return r
