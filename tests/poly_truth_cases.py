"""The inputs of the truth-referenced polynomial tests, in one place: test_poly_truth_gpu.py
launches them on the device, test_poly_truth_cpu.py asserts on any box what makes each of them
meaningful (the path the dispatcher runs, every bucket and family present, a tile across zero
really across zero, a far tile really far, the definitions and emulations within their bounds
of the truth, the bounds not vacuous, no fp32 denormals).

Coefficients: c_m = r_m / X^m with |r_m| in [1/2, 1) from a fixed seed (53 random bits each:
non-dyadic in any short sense, all non-zero) and X the family's length scale, so that every
term of every polynomial is O(1) somewhere on its domain and nothing overflows or underflows
in fp32. In the `balanced` family X = 16 |h|: every |b_m| k^m of a sub-tile near x = 0 is O(1)
at the sub-tile's edge k = 16, so every b_m, every row of the shift and both top indices of
Poly<NC>::parts carry weight.

Launch sizes are the smallest that reach each code path: 64 samples (one tile), 64 * 5 + 37
(five lanes with a tile, the rest idle, and per-sample remainder samples), 64 * 256 + 37 at
grids 1 and 3 (a whole round). Nothing larger: the exact integer tests hold the structure of
large launches.
"""
from __future__ import annotations

import dataclasses
import functools
import math
import random

from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.utils import poly_truth as pt

RULES = ("left", "mid", "right")
REQUESTS = (("fp64", "series"), ("fp64", "ieee"), ("fp32", "series"), ("fp32", "ieee"))
SEED = 20260117


@dataclasses.dataclass(frozen=True)
class Domain:
    id: str
    family: str
    a: float
    b: float
    n: int
    scale: float        # X; 0.0: 16 |h| (balanced)
    zero: bool = False  # launches sit around the zero crossing

    @property
    def h(self) -> float:
        return (self.b - self.a) / self.n

    @property
    def X(self) -> float:
        return self.scale or 16.0 * abs(self.h)


DOMAINS = {d.id: d for d in (
    Domain("balanced", "balanced", -1.0, 1.5, 100003, 0.0, zero=True),
    Domain("unit", "unit", 0.0, 1.0, 1061, 1.0),
    Domain("offset-3to5", "offset", 3.0, 5.0, 20011, 4.0),
    Domain("offset-neg", "offset", -7.25, -2.5, 20011, 8.0),
    Domain("rev-unit", "reversed", 1.0, 0.0, 1061, 1.0),
    Domain("rev-offset", "reversed", 5.0, 3.0, 20011, 4.0),
    Domain("rev-balanced", "reversed", 1.5, -1.0, 100003, 0.0, zero=True),
    # a tile whose midpoint is within half a step of 0, coefficients of unit scale
    Domain("across", "across", -1.0, 1.5, 100003, 1.0, zero=True),
    # |x / h| = 3e9 * 2**30 = 3.2e18 > 2**53: u_m -+ 16 is absorbed, samples sit on ulp(u_m)
    Domain("far", "far", 3.0e9, 3.0e9 + 4.0, 1 << 32, 2.0 ** 32),
    # h = 2**-34 (1 - 2**-20) below ulp(1e6) = 2**-33
    Domain("subulp", "subulp", 1.0e6, 1.0e6 + 2.0 ** -14, (1 << 20) + 1, 2.0 ** 20),
)}
FAMILIES = ("balanced", "unit", "offset", "reversed", "across", "far", "subulp")
BIG_OK = {"offset-3to5", "offset-neg", "rev-offset", "across", "far", "subulp"}  # 64 * 256 + 37 fits
SIZES = (64, 64 * 5 + 37, 64 * 256 + 37)


@functools.lru_cache(maxsize=None)
def coefficients(dom: str, ncoef: int) -> tuple:
    rng = random.Random(f"{SEED}-{dom}-{ncoef}")
    X = DOMAINS[dom].X
    out = []
    for m in range(ncoef):
        r = (0.5 + rng.getrandbits(53) / 2.0 ** 54) * rng.choice((-1.0, 1.0))
        out.append(r / X ** m)
    return tuple(out)


def spec(dom: str, ncoef: int) -> integrands.IntegrandSpec:
    d = DOMAINS[dom]
    return integrands.IntegrandSpec("poly", d.a, d.b, coef=coefficients(dom, ncoef))


def zero_index(dom: str) -> int:
    """The sample index nearest x = 0 of a domain that crosses it."""
    d = DOMAINS[dom]
    return round((0.0 - d.a) / d.h)


def start(dom: str, count: int, rule: str) -> int:
    """An odd first sample (a rank slice: i_begin > 0, no multiple of any tile). Around the
    zero crossing the middle tile's midpoint lands within half a step of x = 0: a tile's samples
    are i ... i + 63, its midpoint at index i + 31.5 + off."""
    d = DOMAINS[dom]
    if d.zero:
        z = (0.0 - d.a) / d.h
        i0 = round(z - 31.5 - float(pt.RULE_OFF[rule]))
        back = 64 * ((count // 64) // 2)      # larger launches: zero in the middle tile
        return i0 - back
    return min((d.n // 3) | 1, d.n - count)


def geom(dom: str, ncoef: int, rule: str, i_begin: int, count: int) -> pt.Geometry:
    return pt.geometry(spec(dom, ncoef), DOMAINS[dom].n, rule, i_begin, count)


def series_ncoefs(dtype: str, dom: str) -> tuple:
    """1..8 on a series request. In the far and sub-ulp families h / x < 2**-53, so b_m / b_0 is
    about 2**-53m and an fp32 b_m is a denormal from m = 3, an fp32 c_m from m = 4: the fp32
    paths run them with 1 and 2 coefficients."""
    if dtype == "fp32" and DOMAINS[dom].family in ("far", "subulp"):
        return (1, 2)
    return (1, 2, 3, 4, 5, 6, 7, 8)


HORNER_ONLY = (9, 12, 16)


def ncoefs(dtype: str, div: str, dom: str) -> tuple:
    base = series_ncoefs(dtype, dom)
    if div == "ieee" and len(base) > 2:
        base = (1, 3, 4, 5, 7, 8)
    wide = HORNER_ONLY if (len(base) > 2 and DOMAINS[dom].family in ("unit", "offset", "reversed")
                           and not DOMAINS[dom].zero) else ()
    return base + wide


def path_of(dtype: str, div: str, ncoef: int) -> str:
    """The path a case is filed under (the CPU tests hold it against the dispatcher)."""
    return f"{dtype}-{'series' if div == 'series' and ncoef <= 8 else 'ieee'}"


# ---------------------------------------------------------------------------- launches
@dataclasses.dataclass(frozen=True)
class LaunchCase:
    dtype: str
    div: str
    dom: str
    ncoef: int
    rule: str
    i_begin: int
    count: int
    grid: int
    fused: bool

    @property
    def path(self) -> str:
        return path_of(self.dtype, self.div, self.ncoef)

    @property
    def family(self) -> str:
        return DOMAINS[self.dom].family

    @property
    def id(self) -> str:
        return (f"{self.dtype}-{self.div}-{self.dom}-c{self.ncoef}-{self.rule}-i{self.i_begin}"
                f"-n{self.count}-g{self.grid}-{'fused' if self.fused else 'two'}")

    def geometry(self) -> pt.Geometry:
        return geom(self.dom, self.ncoef, self.rule, self.i_begin, self.count)


def _launch_cases():
    """Every request x domain x coefficient count once, the shape (size and grid), the rule and
    fused / two-kernel taken in turn, so that every family meets all of them on every path."""
    out = []
    for dtype, div in REQUESTS:
        turn = 0
        for dom in DOMAINS:
            shapes = [(SIZES[0], 1), (SIZES[1], 1)]
            if dom in BIG_OK:
                shapes += [(SIZES[2], 1), (SIZES[2], 3)]
            for nc in ncoefs(dtype, div, dom):
                count, grid = shapes[turn % len(shapes)]
                rule = RULES[turn % 3]
                out.append(LaunchCase(dtype, div, dom, nc, rule, start(dom, count, rule), count, grid,
                                      fused=bool(turn % 2)))
                turn += 1
            turn += 1       # the next domain starts on another shape, rule and kernel
    return out


LAUNCH_CASES = _launch_cases()


# ---------------------------------------------------------------------------- per point
POINT_COUNT = 64 * 4 + 37


@dataclasses.dataclass(frozen=True)
class PointCase:
    div: str
    dom: str
    ncoef: int
    rule: str
    i_begin: int

    @property
    def path(self) -> str:
        return path_of("fp64", self.div, self.ncoef)

    @property
    def family(self) -> str:
        return DOMAINS[self.dom].family

    @property
    def id(self) -> str:
        return f"{self.div}-{self.dom}-c{self.ncoef}-{self.rule}-i{self.i_begin}"

    def geometry(self) -> pt.Geometry:
        return geom(self.dom, self.ncoef, self.rule, self.i_begin, POINT_COUNT)


def _point_cases():
    """fp64 series at a coefficient count of every bucket and top-index pattern (2, 4: Poly<4>;
    5, 6: Poly<6>; 7; 8) and Horner at every bucket (3: Poly<4>; 8; 12, 16: Poly<16>), every
    family; four full tiles (series_point; two of Horner's) and 37 samples by point()."""
    out = []
    for k, dom in enumerate(DOMAINS):
        wide = (12, 16) if DOMAINS[dom].family in ("unit", "offset") else ()
        for div, ncs in (("series", (2, 4, 5, 6, 7, 8)), ("ieee", (3, 8) + wide)):
            for j, nc in enumerate(ncs):
                rule = RULES[(k + j) % 3]
                out.append(PointCase(div, dom, nc, rule, start(dom, POINT_COUNT, rule)))
    return out


POINT_CASES = _point_cases()


# ---------------------------------------------------------------------------- degenerate
DEGENERATE_COUNT = 64 * 3 + 5
DEGENERATE_N = 1000


@dataclasses.dataclass(frozen=True)
class DegenerateCase:
    """a == b: h = 0, every sample at a, the value exactly 0.0 whatever p(a) is, as long as it
    is finite."""
    dtype: str
    div: str
    a: float
    ncoef: int

    @property
    def id(self) -> str:
        return f"{self.dtype}-{self.div}-a{self.a:g}-c{self.ncoef}"

    @property
    def spec(self) -> integrands.IntegrandSpec:
        X = {0.0: 1.0, 1.0: 1.0, -3.5: 4.0, 1e30: 2.0 ** 100}[self.a]
        rng = random.Random(f"{SEED}-point-{self.a}-{self.ncoef}")
        coef = tuple((0.5 + rng.getrandbits(53) / 2.0 ** 54) * rng.choice((-1.0, 1.0)) / X ** m
                     for m in range(self.ncoef))
        return integrands.IntegrandSpec("poly", self.a, self.a, coef=coef)

    def geometry(self) -> pt.Geometry:
        return pt.geometry(self.spec, DEGENERATE_N, "mid", 0, DEGENERATE_COUNT)


def _degenerate_cases():
    """At 1e30 p(a) must stay finite: 1e30^7 = 1e210 does in fp64 (8 coefficients), fp32 holds
    x^1 only (2 coefficients)."""
    out = []
    for dtype, div in REQUESTS:
        for a in (0.0, 1.0, -3.5):
            out += [DegenerateCase(dtype, div, a, nc) for nc in (1, 4, 6, 7, 8, 12)]
        out += [DegenerateCase(dtype, div, 1e30, nc) for nc in ((2, 8) if dtype == "fp64" else (2,))]
    return out


DEGENERATE_CASES = _degenerate_cases()


# ---------------------------------------------------------------------------- underflow
UNDERFLOW_INTERVALS = {"0to2p-140": (0.0, 2.0 ** -140), "2p-150to2p-149": (2.0 ** -150, 2.0 ** -149)}
UNDERFLOW_COUNT = 64 * 3 + 5      # = n: the whole interval


@dataclasses.dataclass(frozen=True)
class UnderflowCase:
    """A pure (c_d x^d) or near-pure (c_0 + c_d x^d, c_0 of the top term's size at the right
    end) monomial of degree d whose c_d h^d is a denormal (target 2**-1040) or zero (2**-1090),
    and the plain c_7 = O(1) on [0, 2**-140] (target 0: c_7 h^7 = 2**-1033)."""
    dtype: str
    div: str
    interval: str
    degree: int
    target: int
    near: bool

    @property
    def id(self) -> str:
        return (f"{self.dtype}-{self.div}-{self.interval}-d{self.degree}-t{self.target}"
                f"-{'near' if self.near else 'pure'}")

    @property
    def spec(self) -> integrands.IntegrandSpec:
        a, b = UNDERFLOW_INTERVALS[self.interval]
        h = (b - a) / UNDERFLOW_COUNT
        rng = random.Random(f"{SEED}-under-{self.interval}-{self.degree}-{self.target}")
        r = 0.5 + rng.getrandbits(53) / 2.0 ** 54
        e = self.target - self.degree * math.frexp(h)[1] if self.target else 0
        cd = math.ldexp(r, e)
        coef = [0.0] * (self.degree + 1)
        coef[-1] = cd
        if self.near:
            coef[0] = -0.75 * cd * b ** self.degree
        return integrands.IntegrandSpec("poly", a, b, coef=tuple(coef))

    def geometry(self) -> pt.Geometry:
        return pt.geometry(self.spec, UNDERFLOW_COUNT, "mid", 0, UNDERFLOW_COUNT)


def _underflow_cases():
    out = []
    for dtype, div in REQUESTS:
        for iv in UNDERFLOW_INTERVALS:
            for d in (5, 6, 7):
                for target in (-1040, -1090):
                    out.append(UnderflowCase(dtype, div, iv, d, target, near=(d + target) % 2 == 0))
        out.append(UnderflowCase(dtype, div, "0to2p-140", 7, 0, False))
    return out


UNDERFLOW_CASES = _underflow_cases()


# ---------------------------------------------------------------------------- the plan
# The plan never launches more workgroups than ceil(tiles / block): 5 workgroups of 1024 threads
# need 4097 tiles. [-1, 1.5] in 64 * 4097 + 5 steps: at block 1024 one tile in the fifth
# workgroup, at block 64 twelve rounds and an exec-masked thirteenth; 5 samples left over.
PLAN_N = 64 * 4097 + 5
PLAN_GRID = 5
PLAN_BLOCKS = (64, 1024)
PLAN_STEPS = 8


def plan_spec() -> integrands.IntegrandSpec:
    """Balanced, degree 7: c_m = r_m / (16 h)^m on [-1, 1.5] at PLAN_N steps."""
    X = 16.0 * (2.5 / PLAN_N)
    rng = random.Random(f"{SEED}-plan")
    coef = tuple((0.5 + rng.getrandbits(53) / 2.0 ** 54) * rng.choice((-1.0, 1.0)) / X ** m
                 for m in range(8))
    return integrands.IntegrandSpec("poly", -1.0, 1.5, coef=coef)
