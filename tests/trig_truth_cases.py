"""The inputs of the truth-referenced sin / train-velocity tests, in one place:
test_trig_truth_gpu.py launches them on the device, test_trig_truth_cpu.py asserts on any box
what makes each of them meaningful (representable coordinates where a case claims them, the
fp32 tiles' sensitivity, the closed form against a brute-force sum, which division runs).

Exact coordinates: a an integer (or a small dyadic), h = 2**-k and b = a + n h, so that
(b - a) / n is h again and every sample and tile midpoint is a double (multiples of h / 2
below 2**53 h / 2: trig_truth.coords_exact). The train's exact cases take ts = 2**-j too, so
that t * (1 / ts) is exact and theta = t 2**j reaches any range on [0, 1800]. Their bound
carries no coordinate term and stays a few ulp(1) at any distance.
"""
from __future__ import annotations

import dataclasses
import functools
import math

from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.utils import trig_truth as tt

WINDOW = 4096          # samples of a per-point window
VS = integrands.TRAIN_VS
TS = integrands.TRAIN_TS
RULES = ("left", "mid", "right")


def sin_spec(a: float, h: float, n: int) -> integrands.IntegrandSpec:
    """sin on [a, a + n h] (h < 0: a reversed interval)."""
    return integrands.IntegrandSpec("sin", float(a), float(a) + n * h)


def train_spec(ts: float, vs: float = VS, a: float = 0.0, b: float = 1800.0):
    return integrands.IntegrandSpec("train", float(a), float(b), p0=float(ts), p1=float(vs))


@dataclasses.dataclass(frozen=True)
class Domain:
    """One family: an integrand on a domain at a step. `exact`: coordinates (and the train's
    angle) are formed without rounding. Whether a launch is far (an end angle beyond
    TRIG_SERIES_MAX_N quadrants) is decided per launch, from its own samples: runs_series."""
    id: str
    spec: integrands.IntegrandSpec
    n: int
    exact: bool
    coarse: bool = False       # delta large enough for the packed-fp32 tiles' sensitivity

    @property
    def h(self) -> float:
        return (self.spec.b - self.spec.a) / self.n

    @property
    def name(self) -> str:
        return self.spec.name


def _sin_exact(id_, a, k, n, coarse=False):
    return Domain(id_, sin_spec(a, 2.0 ** -k, n), n, True, coarse)


def _sin_reversed(id_, a, k, n, coarse=False):
    return Domain(id_, sin_spec(a, -(2.0 ** -k), n), n, True, coarse)


N1800 = lambda k: 1800 << k   # noqa: E731  (h = 2**-k on [0, 1800])

DOMAINS = {d.id: d for d in [
    # ---- sin, exact coordinates, one family per angle range
    _sin_exact("sin-near0", -2.0, 10, 1 << 13),
    _sin_exact("sin-pm40", -40.0, 7, 80 << 7),
    _sin_exact("sin-1e5", 102912.0, 7, 1 << 14),       # straddles kFastTrigMaxN (102943.7)
    _sin_exact("sin-1e7", 1.0e7, 9, 1 << 14),
    _sin_exact("sin-3.0e9", 3.0e9, 10, 1 << 14),
    _sin_exact("sin-3.373e9", 3.373e9, 10, 1 << 14),   # the last 1.6e5 rad under the limit
    _sin_exact("sin-3.4e9", 3.4e9, 10, 1 << 14),
    _sin_exact("sin-m3.4e9", -3.4e9 - 16.0, 10, 1 << 14),
    _sin_exact("sin-1e12", 1.0e12, 10, 1 << 14),
    # coarse steps (delta = 2**-6): the packed-fp32 tiles, and structural slips
    _sin_exact("sin-near0-coarse", -2.0, 6, 1 << 10, True),
    _sin_exact("sin-1e5-coarse", 102912.0, 6, 1 << 12, True),
    _sin_exact("sin-3.0e9-coarse", 3.0e9, 6, 1 << 10, True),
    _sin_exact("sin-3.4e9-coarse", 3.4e9, 6, 1 << 10, True),
    # reversed intervals (b < a, h < 0)
    _sin_reversed("sin-rev-pm40", 40.0, 7, 80 << 7),
    _sin_reversed("sin-rev-coarse", 40.0, 6, 80 << 6, True),
    _sin_reversed("sin-rev-3.4e9", 3.4e9 + 16.0, 10, 1 << 14),
    # ---- sin, the workload's own domains and steps (coordinates round)
    Domain("sin-0pi-1e9", integrands.sin(), 10 ** 9, False),
    Domain("sin-0pi-1e10", integrands.sin(), 10 ** 10, False),
    Domain("sin-0pi-200", integrands.sin(), 200, False, True),
    Domain("sin-pi0-1e9", integrands.IntegrandSpec("sin", math.pi, 0.0), 10 ** 9, False),
    Domain("sin-pm40-1e8", integrands.IntegrandSpec("sin", -40.0, 40.0), 10 ** 8, False),
    # ---- train on [0, 1800], exact: ts = 2**-j, h = 2**-k (theta = t 2**j, delta = 2**(j-k))
    Domain("train-near0", train_spec(2.0 ** 9), N1800(10), True),          # theta <= 3.5
    Domain("train-56", train_spec(2.0 ** 5), N1800(12), True),             # theta <= 56
    Domain("train-neg-ts", train_spec(-(2.0 ** 5)), N1800(12), True),      # theta >= -56
    Domain("train-1e5", train_spec(2.0 ** -6), N1800(14), True),           # <= 1.15e5, straddles
    Domain("train-1e7", train_spec(2.0 ** -13), N1800(22), True),          # <= 1.5e7
    Domain("train-3.8e9", train_spec(2.0 ** -21), N1800(30), True),        # <= 3.77e9: far
    Domain("train-1e12", train_spec(2.0 ** -30), N1800(39), True),         # <= 1.9e12: far
    Domain("train-56-coarse", train_spec(2.0 ** 5), N1800(0), True, True),     # delta = 2**-5
    Domain("train-3.8e9-coarse", train_spec(2.0 ** -21), N1800(26), True, True),
    Domain("train-rev-56", train_spec(2.0 ** 5, a=1800.0, b=0.0), N1800(12), True),
    Domain("train-rev-coarse", train_spec(2.0 ** 5, a=1800.0, b=0.0), N1800(0), True, True),
    # ---- train, the reference's ts and vs (coordinates and the angle round)
    Domain("train-ref-1e9", integrands.train(), 10 ** 9, False),
    Domain("train-ref-1e10", integrands.train(), 10 ** 10, False),
    Domain("train-ref-600", integrands.train(), 600, False, True),
    Domain("train-ref-rev-1e9", train_spec(TS, a=1800.0, b=0.0), 10 ** 9, False),
    # a small inexact ts that reaches far angles on the default domain (the issue's example)
    Domain("train-small-ts", train_spec(3.0e-7), 10 ** 9, False),
]}


def tile_of(d: Domain, div: str) -> int:
    return tt.SERIES_TILE[d.name] if div == "series" else tt.IEEE_TILE


def index_of_angle(d: Domain, theta: float) -> int:
    """The sample index whose angle is nearest `theta` (left rule)."""
    x = theta * (d.spec.p0 if d.name == "train" else 1.0)
    return max(0, min(d.n - 1, round((x - d.spec.a) / d.h)))


def window_starts(d: Domain, count: int) -> tuple:
    """Where the windows and tiles of a family start: the first samples, an odd index a third
    in, the quadrant boundary and the zero of sin / cos nearest the middle of the domain (the
    window centred on it), and the last `count` samples."""
    mid_theta = float(tt.geometry(d.spec, d.n, "left", d.n // 2, 1).theta(0))
    k = round(mid_theta / (math.pi / 2))
    starts = {0, d.n // 3 | 1, d.n - count}
    for th in (k * math.pi / 2, (k + 0.5) * math.pi / 2, (k + 1) * math.pi / 2):
        starts.add(max(0, min(d.n - count, index_of_angle(d, th) - count // 2)))
    return tuple(sorted(s for s in starts if 0 <= s <= d.n - count))


# ---------------------------------------------------------------------------- per point
@dataclasses.dataclass(frozen=True)
class PointCase:
    dom: str
    rule: str
    i_begin: int
    count: int = WINDOW

    @property
    def id(self) -> str:
        return f"{self.dom}-{self.rule}-i{self.i_begin}"


def _point_cases() -> list:
    out = []
    for j, d in enumerate(DOMAINS.values()):
        if d.coarse and d.n < WINDOW:
            out.append(PointCase(d.id, RULES[j % 3], 0, d.n))
            continue
        starts = window_starts(d, WINDOW)
        # every family: its first window, the one on the middle zero / boundary, the last
        picks = dict.fromkeys((starts[0], starts[len(starts) // 2], starts[-1]))
        for i, s in enumerate(picks):
            out.append(PointCase(d.id, RULES[(i + j) % 3], s))
    out.append(PointCase("sin-0pi-1e10", "mid", (1 << 32) + 12345))       # i_begin > 2**32
    out.append(PointCase("train-1e12", "left", (1 << 40) + 7))
    return out


POINT_CASES = _point_cases()


# ---------------------------------------------------------------------------- single tiles
@dataclasses.dataclass(frozen=True)
class TileCase:
    dom: str
    rule: str
    i_begin: int
    dtype: str
    div: str

    @property
    def id(self) -> str:
        return f"{self.dom}-{self.rule}-i{self.i_begin}-{self.dtype}-{self.div}"


def _tile_cases() -> list:
    out = []
    for j, d in enumerate(DOMAINS.values()):
        for div in ("series", "ieee"):
            T = tile_of(d, div)
            if d.n < T:
                continue
            # every start window_starts names: the first tile, an odd one a third in, the
            # tiles holding the zero of sin / cos and the quadrant boundary (an odd multiple
            # of pi / 4) nearest the middle, and the last full tile (asserted per family and
            # path in test_trig_truth_cpu.py)
            for i, s in enumerate(window_starts(d, T)):
                out.append(TileCase(d.id, RULES[(i + j) % 3], s, "fp64", div))
                # packed fp32: the coarse families only (the sensitivity condition,
                # asserted in test_trig_truth_cpu.py); fp32 per-sample tiles round the angle
                # to fp32 and mean something only while ulp32(theta) is small
                near = tt.geometry(d.spec, d.n, "left", 0, d.n).theta_abs_max <= 64.0
                if d.coarse and (div == "series" or near):
                    out.append(TileCase(d.id, RULES[(i + j) % 3], s, "fp32", div))
    return out


TILE_CASES = _tile_cases()


# ---------------------------------------------------------------------------- slices, ranges
@dataclasses.dataclass(frozen=True)
class SliceCase:
    dom: str
    rule: str
    i_begin: int
    count: int
    dtype: str
    div: str
    grid: int          # 0: the default grid

    @property
    def id(self) -> str:
        return (f"{self.dom}-{self.rule}-i{self.i_begin}-m{self.count}-{self.dtype}-{self.div}"
                f"-g{self.grid}")


def _slice_cases() -> list:
    out = []
    grids = (1, 3, 0)
    # multi-tile slices T k + r, r in {0, 1, T - 1}, odd i_begin, the three rules
    doms = ("sin-pm40", "sin-3.0e9", "sin-3.4e9", "sin-rev-pm40", "sin-0pi-1e9", "sin-pi0-1e9",
            "train-56", "train-neg-ts", "train-1e7", "train-3.8e9", "train-rev-56",
            "train-ref-1e9", "train-ref-rev-1e9")
    j = 0
    for dom in doms:
        d = DOMAINS[dom]
        for div in ("series", "ieee"):
            T = tile_of(d, div)
            for r in (0, 1, T - 1):
                count = T * 37 + r
                i0 = (d.n // 3) | 1
                dtype = "fp32" if (j % 4 == 3 and div == "series") else "fp64"
                # a packed-fp32 launch sums its < T remainder samples by sinf / cosf of the
                # fp32 angle: far out (ulp32(theta) / 2 = 128 rad at 3e9) those samples are
                # arbitrary and their bound could hide a dropped one, so the far fp32 slices
                # are whole tiles
                if dtype == "fp32" and tt.geometry(d.spec, d.n, "left", i0, count).theta_abs_max > 64.0:
                    count = T * 36
                out.append(SliceCase(dom, RULES[j % 3], i0, count, dtype, div, grids[j % 3]))
                j += 1
    # whole ranges: the workload's own launches (what bench.py runs for sin and train), the
    # reversed ones, a far whole range, and a slice beyond 2**32
    for dom in ("sin-0pi-1e9", "train-ref-1e9", "sin-pi0-1e9", "train-ref-rev-1e9"):
        for dtype in ("fp64", "fp32"):
            out.append(SliceCase(dom, "left", 0, DOMAINS[dom].n, dtype, "series", 0))
    out.append(SliceCase("sin-0pi-1e9", "mid", 0, 10 ** 9, "fp64", "ieee", 0))
    out.append(SliceCase("train-small-ts", "left", 0, 10 ** 9, "fp64", "series", 0))
    out.append(SliceCase("train-3.8e9", "mid", 0, 1 << 26, "fp64", "series", 0))
    out.append(SliceCase("train-3.8e9", "mid", N1800(30) - (1 << 20) - 5, 1 << 20, "fp64",
                         "series", 0))
    out.append(SliceCase("train-3.8e9", "mid", N1800(30) - (1 << 20) - 5, 1 << 20, "fp32",
                         "series", 0))
    # an explicit per-sample request in fp32 beyond the limit: the fp64 per-sample tiles
    out.append(SliceCase("sin-3.4e9", "left", 5461, 7104, "fp32", "ieee", 1))
    out.append(SliceCase("train-1e12", "mid", (1 << 41) + 1, 4737, "fp32", "ieee", 3))
    out.append(SliceCase("sin-0pi-1e10", "left", (1 << 32) + 1, 10 ** 8 + 1, "fp64", "series", 0))
    out.append(SliceCase("sin-0pi-1e10", "left", (1 << 32) + 1, 10 ** 8 + 1, "fp32", "series", 0))
    out.append(SliceCase("train-ref-1e10", "right", (1 << 33) + 3, 10 ** 8 + 127, "fp64",
                         "series", 0))
    return out


SLICE_CASES = _slice_cases()


# ---------------------------------------------------------------------------- plans
@dataclasses.dataclass(frozen=True)
class PlanCase:
    dom: str
    dtype: str
    block: int
    multistep: bool
    n: int | None = None     # the plan's own n over the family's domain (default: its n)

    @property
    def id(self) -> str:
        return f"{self.dom}-{self.dtype}-b{self.block}-{'ms' if self.multistep else 'chained'}"


PLAN_CASES = [
    PlanCase("sin-0pi-1e9", "fp64", 256, True),
    PlanCase("sin-0pi-1e9", "fp32", 1024, False),
    PlanCase("train-ref-1e9", "fp64", 64, True, n=10 ** 8),
    PlanCase("train-ref-1e9", "fp32", 256, True),
    PlanCase("sin-pi0-1e9", "fp64", 1024, True),
    PlanCase("sin-3.4e9", "fp64", 256, True, n=1 << 24),      # far: the per-sample fallback
    PlanCase("train-small-ts", "fp32", 256, True, n=10 ** 8),  # far, fp32 request
]


# ---------------------------------------------------------------------------- shared truth
@functools.lru_cache(maxsize=None)
def truth_values(dom: str, rule: str, i_begin: int, count: int):
    d = DOMAINS[dom]
    return tt.true_values(d.spec, d.n, rule, i_begin, count)


@functools.lru_cache(maxsize=None)
def truth_sum(dom: str, rule: str, i_begin: int, count: int):
    d = DOMAINS[dom]
    return tt.true_sum(d.spec, d.n, rule, i_begin, count)


def geom(dom: str, rule: str, i_begin: int, count: int) -> tt.Geometry:
    d = DOMAINS[dom]
    return tt.geometry(d.spec, d.n, rule, i_begin, count)


def runs_series(g: tt.Geometry, div: str) -> bool:
    """What the dispatcher decides from the launch's end angles (kernels.hpp,
    trig_series_in_range); asserted against the extension in the CPU tests."""
    return div == "series" and g.quadrants <= tt.TRIG_SERIES_MAX_N


@functools.lru_cache(maxsize=None)
def truth_trig(dom: str, rule: str, i_begin: int, count: int):
    d = DOMAINS[dom]
    return tt.true_trig(d.spec, d.n, rule, i_begin, count)


def effective_path(g: tt.Geometry, dtype: str, div: str) -> tuple:
    """(div, fp32) of the tiles a launch runs: beyond the limit the per-sample fp64 tiles,
    whatever was asked (kernels.hpp)."""
    far = g.quadrants > tt.TRIG_SERIES_MAX_N
    return ("ieee" if far else div), (dtype == "fp32" and not far)


def tile_bound(c: TileCase) -> float:
    """The derived bound of partials[0] of a single-tile launch against truth_sum: the tile
    bound of the path that runs, with sum |.| taken from the truth; a series request beyond
    the limit runs T / 32 per-sample tiles on as many lanes, whose sums meet in the wave's 6
    DPP additions."""
    import numpy as np

    d = DOMAINS[c.dom]
    T = tile_of(d, c.div)
    g = geom(c.dom, c.rule, c.i_begin, T)
    vals, _ = truth_values(c.dom, c.rule, c.i_begin, T)
    trig, _ = truth_trig(c.dom, c.rule, c.i_begin, T)
    div, fp32 = effective_path(g, c.dtype, c.div)
    if div == "series":
        return tt.series_tile_bound(g, fp32, abs_sum=float(np.abs(trig).sum()))
    tot = 0.0
    for s in range(0, T, tt.IEEE_TILE):
        sub = dataclasses.replace(g, i_begin=g.i_begin + s, count=tt.IEEE_TILE)
        # (the angle terms read the sub-tile's own far end: no smaller than needed)
        A = np.abs(vals[s:s + 32]).sum() if fp32 else np.abs(trig[s:s + 32]).sum()
        tot += tt.ieee_tile_bound(sub, fp32, abs_sum=float(A))
    if T > tt.IEEE_TILE:
        tot += 6 * tt.U64 * float(np.abs(vals).sum())
    return tot


def tile_sensitivity(c: TileCase) -> float:
    """max_i |d f / d i| over the tile: what one sample misplaced by one step moves the sum."""
    import numpy as np

    T = tile_of(DOMAINS[c.dom], c.div)
    return float(np.abs(truth_trig(c.dom, c.rule, c.i_begin, T)[1]).max())
