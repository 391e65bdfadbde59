"""The inputs of the truth-referenced 4/(1+x^2) tests, in one place: test_pi4_truth_gpu.py
launches them on the device, test_pi4_truth_cpu.py asserts on any box what makes each of them
meaningful (which path the dispatcher runs, exact coordinates where a case claims them, the
tile across zero really across zero, the definitions within their bounds of the truth, the
bounds not vacuous).

Shapes are the smallest at which a path can still go wrong: single tiles, windows of 4096
points, slices of at most 261 tiles taken with i_begin / n_local out of a large n, and the
listed whole ranges. Every domain is run at the largest h each path admits (N = 96 000 001
for the 384-sample tiles on [0, 1], 48 000 001 for the fp32 tiles, 8 000 000 for
series_direct) unless its name says otherwise.
"""
from __future__ import annotations

import dataclasses
import functools

from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.utils import pi4_truth as pt

WINDOW = 4096
RULES = ("left", "mid", "right")
MIRROR = {"left": "right", "mid": "mid", "right": "left"}
REQUEST = {  # path -> (dtype, div) that asks for it
    "fp64-series_exact": ("fp64", "series_exact"), "fp64-series": ("fp64", "series"),
    "fp64-series_direct": ("fp64", "series_direct"), "fp64-ieee": ("fp64", "ieee"),
    "fp32-series": ("fp32", "series"), "fp32-ieee": ("fp32", "ieee"),
    "fp32acc-series": ("fp32acc", "series"), "fp32acc-ieee": ("fp32acc", "ieee"),
}
PATHS = tuple(REQUEST)


def spec(a: float, b: float) -> integrands.IntegrandSpec:
    return integrands.IntegrandSpec("pi4", float(a), float(b))


@dataclasses.dataclass(frozen=True)
class Domain:
    id: str
    spec: integrands.IntegrandSpec
    n: int
    exact: bool = False     # every fp64 coordinate is formed without rounding
    reverse_of: str | None = None

    @property
    def h(self) -> float:
        return (self.spec.b - self.spec.a) / self.n


N384, N192, N32 = 96_000_001, 48_000_001, 8_000_000      # largest h on a unit interval
_FWD = [
    Domain("unit-96M", spec(0, 1), N384), Domain("unit-48M", spec(0, 1), N192),
    Domain("unit-8M", spec(0, 1), N32),
    Domain("unit-1e9", spec(0, 1), 10 ** 9), Domain("unit-5e9", spec(0, 1), 5 * 10 ** 9),
    Domain("unit-1e10", spec(0, 1), 10 ** 10),
    # [-1, 1/2]: one tile holds x = 0 (the slope A = -2 x h s changes sign there)
    Domain("cross-96M", spec(-1, 0.5), 144_000_002), Domain("cross-48M", spec(-1, 0.5), 72_000_001),
    Domain("cross-8M", spec(-1, 0.5), 12_000_000),
    # off the unit interval: s < 1/2 (1 - s rounds), then h below ulp(x)
    Domain("8to9-96M", spec(8, 9), N384), Domain("8to9-48M", spec(8, 9), N192),
    Domain("8to9-8M", spec(8, 9), N32),
    Domain("1e6", spec(1e6, 1e6 + 1), N384),
    Domain("1e12", spec(1e12, 1e12 + 1024), 10 ** 11),
    # exact coordinates: a dyadic, h = 2**-27; every 192-sample tile midpoint under the mid
    # rule is an fp32 number on [0, 4)
    Domain("exact-0to4", spec(0, 4), 1 << 29, exact=True),
]
_REV = [Domain("rev-" + d.id, spec(d.spec.b, d.spec.a), d.n, d.exact, d.id)
        for d in _FWD if d.id in ("unit-96M", "unit-48M", "unit-8M", "cross-96M", "cross-48M",
                                  "cross-8M", "8to9-96M", "8to9-48M", "8to9-8M", "1e6", "1e12",
                                  "exact-0to4")]
# far from the origin: slices of a huge n (h = 2**-26 over 2**32), and degenerate intervals
_FAR = [
    Domain("far-2p61", spec(2.0 ** 61, 2.0 ** 61 + 2.0 ** 32), 1 << 58),      # fp32 series still runs
    Domain("far-1.2e19", spec(1.2e19, 1.2e19 + 2.0 ** 32), 1 << 58),           # 2**63 < x < 1.84e19
    Domain("far-2e19", spec(2e19, 2e19 + 2.0 ** 32), 1 << 58),                 # fp32 d_m overflows
    Domain("point-1", spec(1.0, 1.0), 1000), Domain("point-1e200", spec(1e200, 1e200), 1000),
    Domain("wide-1e150", spec(1e150, 2e150), 1_000_003), Domain("wide-1e160", spec(1e160, 2e160), 4097),
]
DOMAINS = {d.id: d for d in _FWD + _REV + _FAR}

# the domain of each size class a path runs at its largest h
SIZE = {"fp64-series_exact": "96M", "fp64-series": "96M", "fp64-series_direct": "8M",
        "fp64-ieee": "96M", "fp32-series": "48M", "fp32-ieee": "48M", "fp32acc-series": "48M",
        "fp32acc-ieee": "48M"}


def dom_for(path: str, family: str) -> str:
    """unit / cross / 8to9 (and their rev- forms) at the path's largest h; other families as
    they are."""
    base = family[4:] if family.startswith("rev-") else family
    if base in ("unit", "cross", "8to9"):
        return f"{family}-{SIZE[path]}"
    return family


def geom(dom: str, rule: str, i_begin: int = 0, count: int | None = None) -> pt.Geometry:
    d = DOMAINS[dom]
    return pt.geometry(d.spec, d.n, rule, i_begin, count)


# ---------------------------------------------------------------------------- the dispatcher
def expected_path(dtype: str, div: str, g: pt.Geometry) -> str:
    """kernels.hpp effective_div(params, div, dtype) for pi4, in Python: the h test of each
    series tile, then the end-coordinate test of the series tiles."""
    h = abs(g.h)
    ok = lambda half: half * h <= pt.HALF_SPAN_H  # noqa: E731
    x0 = abs(pt.fma64(pt.base_index(g), g.h, g.a))
    x1 = abs(pt.fma64(pt.base_index(g) + float(g.count - 1), g.h, g.a))
    if dtype != "fp64":
        lim = pt.PI4_F32_SERIES_MAX_X
        eff = "series" if (div != "ieee" and ok(96)) else "ieee"
    else:
        lim = pt.PI4_SERIES_MAX_X
        if div == "ieee":
            eff = "ieee"
        elif div in ("series", "series_exact") and ok(192):
            eff = div
        else:
            eff = "series_direct" if ok(16) else "ieee"
    if eff != "ieee" and not (x0 < lim and x1 < lim):
        eff = "ieee"
    return f"{dtype}-{eff}"


def expected_narrow(dtype: str, g: pt.Geometry) -> bool:
    """riemann.hip pi4_narrow: both end coordinates below 2**249 (fp64) or 2**49 (fp32)."""
    lim = pt.PI4_NARROW_MAX_X if dtype == "fp64" else pt.PI4_F32_NARROW_MAX_X
    x0 = abs(pt.fma64(pt.base_index(g), g.h, g.a))
    x1 = abs(pt.fma64(pt.base_index(g) + float(g.count - 1), g.h, g.a))
    return x0 < lim and x1 < lim


# ---------------------------------------------------------------------------- truth, cached
@functools.lru_cache(maxsize=None)
def truth_sum(dom: str, rule: str, i_begin: int, count: int):
    return pt.true_sum(geom(dom, rule, i_begin, count))


@functools.lru_cache(maxsize=None)
def truth_values(dom: str, rule: str, i_begin: int, count: int):
    return pt.true_values(geom(dom, rule, i_begin, count))


@functools.lru_cache(maxsize=None)
def defined_sum(path: str, dom: str, rule: str, i_begin: int):
    return pt.defined_tile_sum(path, geom(dom, rule, i_begin, pt.tile_len(path)))


@functools.lru_cache(maxsize=None)
def model_parts(path: str, dom: str, rule: str, i_begin: int, count: int, grid: int) -> tuple:
    return tuple(pt.model_partials(path, geom(dom, rule, i_begin, count), grid))


# ---------------------------------------------------------------------------- single tiles
@dataclasses.dataclass(frozen=True)
class TileCase:
    path: str
    dom: str
    rule: str
    i_begin: int
    tag: str

    @property
    def id(self) -> str:
        return f"{self.path}-{self.dom}-{self.rule}-{self.tag}"


def zero_tile_start(dom: str, T: int) -> int:
    """First sample of a T-sample tile of [-1, 1/2] (or its reverse) that holds x = 0 about a
    third of the way in (a launch's tiles start at its i_begin)."""
    d = DOMAINS[dom]
    i = round((0.0 - d.spec.a) / d.h)
    return i - T // 3 - 1


def _tile_cases():
    out = []
    for path in PATHS:
        T = pt.tile_len(path)
        for fam in ("unit", "rev-unit", "8to9", "rev-8to9"):
            dom = dom_for(path, fam)
            n = DOMAINS[dom].n
            tiles = n // T
            for tag, t, rule in (("first", 0, "left"), ("middle", tiles // 2 + 1, "mid"),
                                 ("last", tiles - 1, "right")):
                if fam.startswith("rev-") and tag != "middle":
                    continue
                out.append(TileCase(path, dom, rule, t * T, tag))
        for fam in ("cross", "rev-cross"):
            dom = dom_for(path, fam)
            out.append(TileCase(path, dom, "mid", zero_tile_start(dom, T), "zero"))
        for dom in ("unit-1e9", "unit-1e10", "1e6", "rev-1e6", "1e12", "rev-1e12"):
            tiles = DOMAINS[dom].n // T
            out.append(TileCase(path, dom, "mid", (tiles // 3) * T, "third"))
        # exact coordinates (mid rule: the fp32 tiles' midpoints are fp32 numbers)
        for dom in ("exact-0to4", "rev-exact-0to4"):
            tiles = DOMAINS[dom].n // T
            for tag, t in (("first", 0), ("x1", tiles // 4), ("last", tiles - 1)):
                out.append(TileCase(path, dom, "mid", t * T, tag))
    return out


TILE_CASES = _tile_cases()


# ---------------------------------------------------------------------------- remainders
@dataclasses.dataclass(frozen=True)
class RemCase:
    path: str
    dom: str
    rule: str
    i_begin: int
    count: int

    @property
    def id(self) -> str:
        return f"{self.path}-{self.dom}-{self.rule}-i{self.i_begin}-n{self.count}"


def _rem_cases():
    out = []
    for path in PATHS:
        T = pt.tile_len(path)
        for fam, rule in (("unit", "left"), ("rev-8to9", "mid")):
            dom = dom_for(path, fam)
            i0 = (DOMAINS[dom].n // 3) | 1
            for count in dict.fromkeys((1, 31, T - 1, T + 100)):
                out.append(RemCase(path, dom, rule, i0, count))
    return out


REM_CASES = _rem_cases()


# ---------------------------------------------------------------------------- windows
@dataclasses.dataclass(frozen=True)
class WindowCase:
    div: str
    dom: str
    rule: str
    i_begin: int

    @property
    def path(self) -> str:
        return "fp64-" + self.div

    @property
    def id(self) -> str:
        return f"{self.div}-{self.dom}-{self.rule}-i{self.i_begin}"


def _window_cases():
    out = []
    for div in ("series_exact", "series", "series_direct", "ieee"):
        path = "fp64-" + div
        for fam in ("unit", "cross", "8to9", "rev-unit", "1e6", "1e12", "exact-0to4",
                    "rev-exact-0to4"):
            dom = dom_for(path, fam)
            n = DOMAINS[dom].n
            # an odd start that is no multiple of any tile: the window's last tile is partial
            starts = {"unit": (0, (n // 2) | 1, n - WINDOW), "cross": (zero_tile_start(dom, 384) - 1000,)}
            for i0 in starts.get(fam, ((n // 3) | 1,)):
                out.append(WindowCase(div, dom, "mid" if fam != "unit" else "left", i0))
    return out


WINDOW_CASES = _window_cases()

# fp32 samples, one launch each (n_local = 1 runs Pi4F32::point): 64 of them per family
POINT32_FAMILIES = ("unit", "rev-8to9", "1e6", "exact-0to4")
POINT32_COUNT = 64


# ---------------------------------------------------------------------------- slices, ranges
@dataclasses.dataclass(frozen=True)
class SliceCase:
    path: str
    dom: str
    rule: str
    i_begin: int
    count: int
    grid: int          # 0: the default grid

    @property
    def id(self) -> str:
        return f"{self.path}-{self.dom}-{self.rule}-i{self.i_begin}-n{self.count}-g{self.grid}"


def _slice_cases():
    """69 tiles (a full round and an exec-masked extra round), + 100 samples (the per-point
    remainder), 261 tiles (every lane a round, five lanes another), at grids 1 and 2: the
    shapes of test_exec_masked_extra_round, for every path. The reversed and off-unit
    families take the middle shape."""
    out = []
    for path in PATHS:
        T = pt.tile_len(path)
        dom = dom_for(path, "unit")
        i0 = T * (DOMAINS[dom].n // T // 2)
        for grid in (1, 2):
            for count in (T * 69, T * 69 + 100, T * 261):
                out.append(SliceCase(path, dom, "left", i0, count, grid))
        for fam in ("rev-unit", "cross", "rev-cross", "8to9", "rev-8to9", "1e6", "rev-1e6", "1e12",
                    "rev-1e12", "exact-0to4", "rev-exact-0to4"):
            dom = dom_for(path, fam)
            i0 = zero_tile_start(dom, T) - 30 * T if "cross" in fam else (DOMAINS[dom].n // 3) | 1
            out.append(SliceCase(path, dom, "mid", i0, T * 69 + 100, 2))
    return out


SLICE_CASES = _slice_cases()


def _range_cases():
    out = []
    for path in PATHS:
        for dom, rules in (("unit-1e9", ("left", "mid")), ("unit-5e9", ("left",)),
                           ("unit-1e10", ("left",)), ("unit-96M", ("left",)),
                           ("rev-unit-96M", ("right",))):
            for rule in rules:
                out.append(SliceCase(path, dom, rule, 0, DOMAINS[dom].n, 0))
    return out


RANGE_CASES = _range_cases()


# ---------------------------------------------------------------------------- far, degenerate
@dataclasses.dataclass(frozen=True)
class FarCase:
    dtype: str
    div: str
    dom: str
    i_begin: int
    count: int
    raises: bool = False     # fp32acc beyond 2**49 under ieee: the dispatcher refuses

    @property
    def id(self) -> str:
        return f"{self.dtype}-{self.div}-{self.dom}-i{self.i_begin}-n{self.count}"


def _far_cases():
    out = []
    # the fp32 series slice the dispatcher used to admit on h alone
    for dom in ("far-2p61", "far-1.2e19", "far-2e19"):
        beyond = dom != "far-2p61"
        for count in (192, 192 * 3 + 7):
            out.append(FarCase("fp32", "series", dom, 192 * 5, count))
            out.append(FarCase("fp32acc", "series", dom, 192 * 5, count, raises=beyond))
        out.append(FarCase("fp32", "ieee", dom, 192 * 5, 64))
        out.append(FarCase("fp64", "series_exact", dom, 192 * 5, 384 + 7))
        out.append(FarCase("fp64", "ieee", dom, 192 * 5, 64))
    # a == b: h = 0, every sample at a; the value is 0.0 on every path
    for dom in ("point-1", "point-1e200"):
        for path, (dtype, div) in REQUEST.items():
            T = pt.tile_len(path)
            out.append(FarCase(dtype, div, dom, 0, T + 100,
                               raises=(dtype == "fp32acc" and dom == "point-1e200")))
    # the existing wide-domain cases: a value, and the zero where 1 + x^2 overflows
    out.append(FarCase("fp64", "ieee", "wide-1e150", 0, 1_000_003))
    out.append(FarCase("fp64", "ieee", "wide-1e160", 0, 4097))
    out.append(FarCase("fp64", "series_exact", "wide-1e150", 0, 4097))    # h too large: ieee
    return out


FAR_CASES = _far_cases()


@dataclasses.dataclass(frozen=True)
class SwitchCase:
    """A 64-sample ieee launch around a narrow / wide switch point X: both ends below, both
    beyond, one on each side (in either order)."""
    dtype: str
    a: float
    b: float
    tag: str

    @property
    def id(self) -> str:
        return f"{self.dtype}-{self.tag}"

    @property
    def spec(self):
        return spec(self.a, self.b)


def _switch_cases():
    out = []
    for dtype, X in (("fp64", pt.PI4_NARROW_MAX_X), ("fp32", pt.PI4_F32_NARROW_MAX_X),
                     ("fp32acc", pt.PI4_F32_NARROW_MAX_X)):
        lo, hi = X * (1 - 2.0 ** -20), X * (1 + 2.0 ** -20)
        out += [SwitchCase(dtype, X / 2, lo, "below"), SwitchCase(dtype, hi, 2 * X, "beyond"),
                SwitchCase(dtype, lo, hi, "across"), SwitchCase(dtype, hi, lo, "across-rev"),
                SwitchCase(dtype, -hi, -lo, "across-neg")]
    return out


SWITCH_CASES = _switch_cases()
SWITCH_N = 64


# ---------------------------------------------------------------------------- plans
PLAN_CASES = [(path, N192 if path.startswith("fp32") else N384) for path in PATHS]
