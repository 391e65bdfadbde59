"""The inputs of the truth-referenced velocity-table tests, in one place: test_table_truth_gpu.py
launches them on the device, test_table_truth_cpu.py asserts on any box what makes each of them
meaningful (the branch census by the kernel's own coordinate operations, the distance from a
switch point, the definitions and emulations within their bounds of the truth, the listed
defects outside them).

Tables are seeds and formulas, not data files. `n` only sets h = (b - a) / n: a case runs the
slice [i_begin, i_begin + count), so a launch is microseconds even at h = 1800 / 1e9. Slice
lengths: 64 (one tile), 64 + 17, 16384 + 5 (one workgroup of tiles and a remainder), 64 * 3000 +
5 (thousands of tiles; grids 1, 3 and the default), and the whole range where a case says so.
"""
from __future__ import annotations

import dataclasses
import functools
import random

from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.utils import table_truth as tt

SEED = 20260118
REQUESTS = (("fp64", "series"), ("fp64", "ieee"), ("fp32", "series"), ("fp32", "ieee"))
ONE, REM, WG, MANY = 64, 64 + 17, 16384 + 5, 64 * 3000 + 5
POINT_MAX = 4096


def _r(rng) -> float:
    """53 random bits in [1/2, 1) with a random sign: non-dyadic in any short sense."""
    return (0.5 + rng.getrandbits(53) / 2.0 ** 54) * rng.choice((-1.0, 1.0))


@functools.lru_cache(maxsize=None)
def table(name: str) -> tuple:
    """() is the built-in profile (1801 entries, 0 <= v <= 87.143, 1002 flat segments).
    jag      37 entries of both signs, slopes of both signs, the last entry set so that the
             trapezoid sum over [0, 36] is about 1e-13 of sum |v| (cancellation)
    offset   1e6 + O(1e-2): a large offset and small variation, 64 entries
    decades  |v| over 12 decades (1e-6 ... 1e6), both signs, 48 entries
    two      2 entries: one segment, no tile may take the kink branch
    max      2048 entries, a random walk
    ends     end segments with |d| << |v| (87.1, 87.100001) and |d| >> |v| (1e-3, 250.7)"""
    rng = random.Random(f"{SEED}-{name}")
    if name == "profile":
        return ()
    if name == "jag":
        v = [3.0 * _r(rng) for _ in range(36)]
        inner = sum(v[1:]) + 0.5 * v[0]
        v.append(-2.0 * inner * (1.0 + 2.0 ** -43))
        return tuple(v)
    if name == "offset":
        return tuple(1.0e6 + 1.0e-2 * _r(rng) for _ in range(64))
    if name == "decades":
        return tuple(_r(rng) * 10.0 ** rng.uniform(-6.0, 6.0) for _ in range(48))
    if name == "two":
        return (0.3, -1.7)
    if name == "max":
        v, out = 0.0, []
        for _ in range(2048):
            v += _r(rng)
            out.append(v)
        return tuple(out)
    if name == "ends":
        return (87.1, 87.100001, 3.0, -2.5, 0.7, 1.0e-3, 250.7)
    raise KeyError(name)


TABLES = ("profile", "jag", "offset", "decades", "two", "max", "ends")


def entries(name: str) -> int:
    return 1801 if name == "profile" else len(table(name))


@dataclasses.dataclass(frozen=True)
class Geom:
    """One slice of one rule. need / forbid: branches the census must / must not hold. either:
    the case sits on a switch point on purpose (a knot on an end sample) and either side is
    allowed; everything else must be at least MARGIN ulps of its coordinate away from one."""
    id: str
    table: str
    a: float
    b: float
    n: int
    rule: str
    i_begin: int
    count: int
    need: tuple = ()
    forbid: tuple = ()
    either: bool = False
    grids: tuple = (1,)

    @property
    def spec(self) -> integrands.IntegrandSpec:
        t = table(self.table)
        return integrands.table(t or None, self.a, self.b)

    def geometry(self, count: int | None = None) -> tt.Geometry:
        return tt.geometry(self.spec, self.n, self.rule, self.i_begin, count or self.count)


MARGIN = 8.0
K10 = 1 << 10


def _geoms():
    G = Geom
    out = [
        # ---- 63 |h| far below 1: line tiles (a knot now and then in the long slices)
        G("profile-line-1", "profile", 0.0, 1800.0, 10 ** 9, "mid", 55833333, ONE, ("line",), ("kink", "coarse")),
        G("profile-line-rem", "profile", 0.0, 1800.0, 10 ** 9, "left", 55833333, REM, ("line",), ("kink", "coarse")),
        G("profile-line-wg", "profile", 0.0, 1800.0, 10 ** 9, "right", 55833333, WG, ("line",), ("coarse",)),
        G("profile-accel-many", "profile", 0.0, 1800.0, 18 * 10 ** 6, "mid", 1200001, MANY, ("line", "kink"),
          ("coarse",), grids=(1, 3, 0)),
        G("jag-line-1", "jag", 0.0, 36.0, 3600007, "mid", 730001, ONE, ("line",), ("kink", "coarse")),
        G("jag-line-wg", "jag", 0.0, 36.0, 3600007, "left", 730001, WG, ("line",), ("coarse",)),
        G("jag-many", "jag", 0.0, 36.0, 3600007, "right", 730001, MANY, ("line", "kink"), ("coarse",),
          grids=(1, 3, 0)),
        G("offset-line", "offset", 0.0, 63.0, 6300007, "mid", 2150001, REM, ("line",), ("kink", "coarse")),
        G("decades-line", "decades", 0.0, 47.0, 4700007, "mid", 1550001, WG, ("line",), ("coarse",)),
        # ---- one knot inside the tile, h = 2**-10, the knot x = 8 at index 8192
        G("kink-on-sample-20", "jag", 0.0, 36.0, 36 * K10, "left", 8192 - 20, ONE, ("kink",), ("line", "coarse")),
        G("kink-at-midpoint", "jag", 0.0, 36.0, 36 * K10, "mid", 8192 - 32, ONE, ("kink",), ("line", "coarse")),
        G("kink-half-step", "jag", 0.0, 36.0, 36 * K10, "mid", 8192 - 10, REM, ("kink",), ("line", "coarse")),
        G("kink-in-first-half", "jag", 0.0, 36.0, 36 * K10, "left", 8192 - 3, ONE, ("kink",), ("line", "coarse")),
        G("kink-in-last-half", "jag", 0.0, 36.0, 36 * K10, "left", 8192 - 50, ONE, ("kink",), ("line", "coarse")),
        G("kink-on-last-sample", "jag", 0.0, 36.0, 36 * K10, "left", 8192 - 63, ONE, (), ("coarse",), either=True),
        G("kink-last-knot", "jag", 0.0, 36.0, 36 * K10, "left", 35 * K10 - 40, REM, ("kink",), ("coarse",)),
        G("kink-last-knot-max", "max", 0.0, 2047.0, 2047 * 512, "mid", 2046 * 512 - 41, REM, ("kink",), ("coarse",)),
        G("kink-offset", "offset", 0.0, 63.0, 15013, "mid", 5001, 64 * 40 + 17, ("line", "kink"), ("coarse",)),
        G("kink-decades", "decades", 0.0, 47.0, 11003, "left", 3001, 64 * 40 + 17, ("line", "kink"), ("coarse",)),
        G("kink-jag-mix", "jag", 0.0, 36.0, 7561, "right", 101, 64 * 40 + 17, ("line", "kink"), ("coarse",)),
        G("kink-max-mix", "max", 0.0, 2047.0, 409507, "mid", 333333, 64 * 40 + 17, ("line", "kink"), ("coarse",)),
        # ---- clamped knots are not kinks: a tile across x = 0 and one across x = entries - 1
        G("across-zero", "jag", -4.0, 40.0, 44 * K10, "left", 4096 - 30, ONE, ("line",), ("kink", "coarse")),
        G("across-end", "jag", -4.0, 40.0, 44 * K10, "mid", 40 * K10 - 30, ONE, ("line",), ("kink", "coarse")),
        G("below-zero-wg", "jag", -10.0, 50.0, 60007, "mid", 1, WG, ("line", "kink"), ("coarse",)),
        G("beyond-end-wg", "jag", -10.0, 50.0, 60007, "left", 60007 - WG, WG, ("line", "kink"), ("coarse",)),
        G("ends-beyond", "ends", -20.0, 30.0, 50021, "mid", 1, 50021 - 1, ("line", "kink"), ("coarse",), grids=(3,)),
        # ---- the line / kink / coarse switch points: 63 |h| just below and above 1 and 2
        G("switch-below-1", "jag", 0.0, 36.0, 2269, "mid", 7, 64 * 12 + 17, ("kink",), ("coarse",)),
        G("switch-above-1", "jag", 0.0, 36.0, 2267, "mid", 7, 64 * 12 + 17, ("kink",), ("line",)),
        G("switch-below-2", "jag", 0.0, 36.0, 1135, "left", 7, 64 * 12 + 17, ("coarse",), ("line",)),
        # one tile just on the rarer side of each switch: its first sample 2e-4 ... 2e-3 past a knot
        G("switch-below-1-line", "jag", 0.0, 36.0, 2273, "mid", 189, ONE, ("line",), ("kink", "coarse")),
        G("switch-above-1-coarse", "jag", 0.0, 36.0, 2261, "mid", 439, ONE, ("coarse",), ("line", "kink")),
        G("switch-below-2-kink", "jag", 0.0, 36.0, 1135, "left", 536, ONE, ("kink",), ("line", "coarse")),
        # the first sample exactly on the knot x = 18 (1134.5 * 36 / 2269): either side is allowed
        G("switch-on-knot", "jag", 0.0, 36.0, 2269, "mid", 1134, ONE, (), ("coarse",), either=True),
        G("switch-above-2", "jag", 0.0, 36.0, 1133, "right", 7, 64 * 12 + 17, ("coarse",), ("line", "kink")),
        # ---- coarse steps spanning tens of segments
        G("coarse-jag", "jag", 0.0, 36.0, 100, "mid", 0, 100, ("coarse",), ("line", "kink")),
        G("coarse-max", "max", 0.0, 2047.0, 1500, "left", 11, 64 * 20 + 17, ("coarse",), ("line", "kink")),
        G("coarse-profile", "profile", 0.0, 1800.0, 1000, "mid", 0, 1000, ("coarse",), ("line", "kink")),
        # ---- one segment
        G("two-dyadic", "two", -3.0, 5.0, 1024, "mid", 0, 1024, ("line",), ("kink", "coarse")),
        G("two-odd", "two", -3.0, 5.0, 1000, "left", 3, 997, ("line",), ("kink", "coarse")),
        # ---- reversed: h < 0, lo >= hi, so never the kink branch
        G("rev-mix", "jag", 36.0, 0.0, 7561, "mid", 101, 64 * 40 + 17, ("line", "coarse"), ("kink",)),
        G("rev-line", "jag", 30.0, 5.0, 3600007, "left", 730001, WG, ("line",), ("kink",)),
        G("rev-ends", "ends", 30.0, -20.0, 50021, "right", 1, 50021 - 1, ("line",), ("kink",), grids=(3,)),
        # ---- far coordinates, h above and below ulp(x): everything is an end segment
        G("far+3e9-sub", "ends", 3.0e9, 3.0e9 + 4.0, 1 << 32, "mid", 1431655765, WG, ("line",), ("kink", "coarse")),
        G("far-3e9", "ends", -3.0e9, -3.0e9 + 4000.0, 1000, "left", 1, 64 * 8 + 17, ("line",), ("kink", "coarse")),
        G("far-1e15-sub", "jag", 1.0e15, 1.0e15 + 1.0, K10, "mid", 3, 64 * 8 + 17, ("line",), ("kink", "coarse")),
        G("far-1e15", "ends", 1.0e15, 2.0e15, 1000, "right", 1, 64 * 8 + 17, ("line",), ("kink", "coarse")),
        G("far-2p60", "ends", 2.0 ** 60, 2.0 ** 60 + 2.0 ** 20, 256, "mid", 1, 255, ("line",), ("kink", "coarse")),
        G("far-2p60-sub", "jag", 2.0 ** 60, 2.0 ** 60 + 2.0 ** 10, 256, "left", 1, 255, ("line",), ("kink", "coarse")),
        G("far-neg-2p60", "ends", -2.0 ** 60, -2.0 ** 60 + 2.0 ** 20, 256, "mid", 1, 255, ("line",), ("kink", "coarse")),
        # ---- i_begin beyond 2**32
        G("ibegin-profile", "profile", 0.0, 1800.0, 10 ** 13, "mid", 5 * 10 ** 12 + 1, REM, ("line",), ("kink", "coarse")),
        G("ibegin-kink", "jag", 0.0, 36.0, 36 << 40, "left", (8 << 40) - 20, REM, ("kink",), ("line", "coarse")),
    ]
    return out


GEOMS = {g.id: g for g in _geoms()}

# The first entry of `ends` rounds to the same float as the second and x - lo reaches 3e9 ... 2**60
# there: the cases the fp32 per-sample form failed on before its slope was subtracted in fp64.
F32_SLOPE_CASES = ("far-3e9", "far-neg-2p60", "far+3e9-sub", "far-1e15", "far-2p60")


# ---------------------------------------------------------------------------- launches
@dataclasses.dataclass(frozen=True)
class LaunchCase:
    geom: str
    dtype: str
    div: str
    grid: int           # 0: the default grid
    fused: bool

    @property
    def path(self) -> str:
        return tt.effective_path(self.dtype, self.div)

    @property
    def id(self) -> str:
        return f"{self.geom}-{self.dtype}-{self.div}-g{self.grid}-{'fused' if self.fused else 'two'}"


def _launch_cases():
    out, turn = [], 0
    for g in GEOMS.values():
        for dtype, div in REQUESTS:
            for grid in g.grids:
                out.append(LaunchCase(g.id, dtype, div, grid, fused=bool(turn % 2)))
                turn += 1
        turn += 1
    return out


LAUNCH_CASES = _launch_cases()
POINT_CASES = [(g.id, div) for g in GEOMS.values() for div in ("series", "ieee")]


def point_count(g: Geom) -> int:
    return min(g.count, POINT_MAX)


# ---------------------------------------------------------------------------- whole range
# The built-in profile over [0, 1800]; the truth is the closed form.
WHOLE = ((100003, "mid"), (1000003, "left"), (18000000, "left"), (10 ** 9, "mid"))
WHOLE_1E9_MID = 122000.00400000015

# ---------------------------------------------------------------------------- a == b
DEGENERATE = (("jag", 7.3), ("jag", -2.0), ("ends", 1.0e15), ("profile", 900.25))
DEGENERATE_N, DEGENERATE_COUNT = 1000, 64 * 3 + 5

# ---------------------------------------------------------------------------- interp_fill
FILL_DTS = (1e-4, 0.37, 2.3e-3)
FILL_NS = (1, 2, 10001)


def fill_cases():
    """(table, dt, i0, n): i0 = 0, 7, the table's end (a window across t = entries - 1) and
    2**33; n = 1, 2 and 10 001 (odd)."""
    out = []
    for name in ("profile", "jag"):
        for dt in FILL_DTS:
            end = int((entries(name) - 1) / dt) - 5000
            for k, i0 in enumerate((0, 7, max(end, 0), 1 << 33)):
                for n in (FILL_NS if k != 1 else (10001,)):
                    out.append((name, dt, i0, n))
    return out


FILL_CASES = fill_cases()
