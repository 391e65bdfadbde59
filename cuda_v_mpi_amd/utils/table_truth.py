"""True values of the velocity-table kernels, what a segment-line tile is DEFINED to evaluate,
operation-by-operation emulations of the four paths, a tile census by the kernel's own
coordinate operations, and derived error bounds.

The sibling of trig_truth.py, pi4_truth.py and poly_truth.py for Integrand::kTable
(csrc/include/miint/integrands.hpp: Table; integrands_f32.hpp: TableF32; csrc/kernels/riemann.hip:
lane_sum, point_values_kernel; csrc/kernels/table.hip: interp_fill_kernel; the host engine's
feval<4>). Pure Python: fractions, integers and numpy; no GPU, no torch. a, h = (b - a) / n, the
rule offset and the table's entries are doubles, i.e. dyadic rationals, so every sample
x_i = a + (i_begin + i + off) h, every interpolated value and every sum is an exact rational.

truth       v(x) = v_s + (v_{s+1} - v_s) (x - s), s = floor(x) clamped to [0, entries - 2]: the
            piecewise-linear interpolant at unit spacing from x = 0 whose two end segments
            extrapolate (what the clamped segment index means). true_values / direct_sum per
            sample; true_sum in closed form: the index range of each segment by exact rational
            division, each segment's contribution an arithmetic series (h > 0, h < 0, h = 0).
definition  A segment tile (64 samples, sub-tile centres at -+16 steps of the midpoint x_m)
            evaluates an exact function of ROUNDED inputs (defined_tile): x_m as riemann.hip
            hands it over, the segments lo, hi of fma(-+31.5, h, x_m), d = fl(v_{lo+1} - v_lo),
            v_m = fma(d, fl(x_m - lo), v_lo), D = fl(d h) and, with one knot inside
            (hi == lo + 1), dD = fl(fl(fl(v_{lo+2} - v_{lo+1}) - d) h) and the knot offset
            kk = fl(fl(lo + 1 - x_m) fl(1 / h)). From them sample u is
                v_m + k D + max(k - kk, 0) dD,   k = u - 31.5,
            exactly. hi > lo + 1 or hi < lo (a coarse or a reversed step) is the per-sample
            form at fma(u, h, fma(-31.5, h, x_m)). `defect` mutates the definition.
emulation   emulate_tile / emulate_point run the kernels' operations one by one in exactly
            rounded fp64 / fp32 (fma, add, max and conversions only). They check the bounds on
            a CPU; they are not what the GPU is compared with.

Bounds. ABSOLUTE, per sample (sample_bounds, fill_bounds) and per launch (launch_sum_bound,
launch_value_bound, host_value_bound), derived in the docstrings from the operations of the
code with U64 = 2**-53 and U32 = 2**-24. Nothing in them comes from a kernel's output. The
interpolant has zeros and sign changes, so nothing is relative to |v|: the unit is the
magnitude M(x) = |v_s| + |d_s| |x - s| (the sizes the fma adds), and for the operations of a
tile M + K with K = 64 |h| max|d| (the sizes of k D and of the kink term).
"""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction

import numpy as np

from .poly_truth import (BLOCK, F32, PATHS, REQUEST, SECOND_ORDER, _fr, fma64, launch_depth,  # noqa: F401
                         rnd32, rnd64)
from .trig_truth import RULE_OFF, U32, U64

TILE_SERIES = 64        # Table::kSeriesTile
TILE_PER_SAMPLE = 32    # every ieee tile
SUB = 32
PAIRS = 16
HSPAN = 31.5            # Table::hspan
MAX_ENTRIES = 2048      # kMaxTable
HOST_BLOCK = 4096       # host.cpp kHostBlock
F32_FLOOR = 128.0 * 2.0 ** -149   # see sample_bounds


# ---------------------------------------------------------------------------- geometry
@dataclasses.dataclass(frozen=True)
class Geometry:
    """The samples of one launch, x_i = a + (i_begin + i + off) h, i < count, exactly, and the
    table's doubles."""
    a: float
    h: float
    off: Fraction
    i_begin: int
    count: int
    table: tuple

    def x(self, i) -> Fraction:
        return Fraction(self.a) + (self.i_begin + Fraction(i) + self.off) * Fraction(self.h)

    @property
    def nseg(self) -> int:
        return len(self.table) - 1

    @property
    def x_abs_max(self) -> float:
        return float(max(abs(self.x(0)), abs(self.x(self.count - 1))))


def geometry(spec, n: int, rule: str, i_begin: int = 0, count: int | None = None) -> Geometry:
    if spec.name != "table":
        raise ValueError("table_truth covers table")
    h = (spec.b - spec.a) / n          # as ops/kernels.py and RiemannPlan form it
    count = n if count is None else count
    tab = tuple(float(v) for v in spec.native_table())
    if count < 1 or i_begin < 0 or not 2 <= len(tab) <= MAX_ENTRIES:
        raise ValueError("need count >= 1, i_begin >= 0 and 2..2048 entries")
    return Geometry(float(spec.a), h, RULE_OFF[rule], int(i_begin), int(count), tab)


# ---------------------------------------------------------------------------- the truth
def seg_exact(g: Geometry, x: Fraction) -> int:
    return min(max(math.floor(x), 0), g.nseg - 1)


def interp_exact(g: Geometry, x: Fraction, s: int | None = None) -> Fraction:
    s = seg_exact(g, x) if s is None else s
    v0, v1 = Fraction(g.table[s]), Fraction(g.table[s + 1])
    return v0 + (v1 - v0) * (x - s)


def true_values(g: Geometry):
    """(fp64 array, list of Fraction): v at every sample, rounded at the very end only."""
    exact = [interp_exact(g, g.x(i)) for i in range(g.count)]
    return np.array([rnd64(v) for v in exact], dtype=np.float64), exact


def direct_sum(g: Geometry) -> Fraction:
    return sum((interp_exact(g, g.x(i)) for i in range(g.count)), Fraction(0))


def segment_ranges(g: Geometry):
    """(x0, h, [(s, i0, i1)]): the launch's samples as an ASCENDING sequence x0 + i h, h >= 0
    (a reversed launch read from its last sample: a sum does not care), and for every segment
    that holds samples the index range [i0, i1). x0 + i h >= s + 1 from i = ceil((s + 1 - x0) /
    h) on, an exact rational division; h = 0 puts every sample in one segment."""
    h = Fraction(g.h)
    x0 = g.x(0)
    if h < 0:
        x0, h = g.x(g.count - 1), -h
    n = g.count
    if h == 0:
        return x0, h, [(seg_exact(g, x0), 0, n)]
    first, last = seg_exact(g, x0), seg_exact(g, x0 + (n - 1) * h)
    out, i0 = [], 0
    for s in range(first, last + 1):
        i1 = n if s == last else min(n, math.ceil((s + 1 - x0) / h))
        if i1 > i0:
            out.append((s, i0, i1))
        i0 = i1
    return x0, h, out


def true_sum(g: Geometry) -> Fraction:
    """sum of v over the launch's samples (unscaled: what the partials add up to), segment by
    segment: sum_{i0 <= i < i1} v_s + d_s (x0 + i h - s) = m (v_s + d_s (x0 - s)) + d_s h (i0 +
    i1 - 1) m / 2, m = i1 - i0."""
    x0, h, ranges = segment_ranges(g)
    tot = Fraction(0)
    for s, i0, i1 in ranges:
        m = i1 - i0
        v0 = Fraction(g.table[s])
        d = Fraction(g.table[s + 1]) - v0
        tot += m * (v0 + d * (x0 - s)) + d * h * Fraction((i0 + i1 - 1) * m, 2)
    return tot


def true_value(g: Geometry) -> Fraction:
    """h sum: what a launch returns (Table::kScale = 1)."""
    return Fraction(g.h) * true_sum(g)


# ---------------------------------------------------------------------------- dispatch mirror
def effective_path(dtype: str, div: str) -> str:
    """kernels.hpp effective_div for the table: fp64 runs the segment tiles on a series or
    series_exact request, fp32 on anything but ieee; at any h."""
    ser = div in ("series", "series_exact") if dtype == "fp64" else div != "ieee"
    return f"{dtype}-{'series' if ser else 'ieee'}"


def tile_len(path: str) -> int:
    return TILE_SERIES if path.endswith("series") else TILE_PER_SAMPLE


def base_index(g: Geometry) -> float:
    """lane_sum's `base`: double(i_begin) + off (exact: i_begin < 2**52)."""
    return float(g.i_begin) + float(g.off)


def inv_h(g: Geometry) -> float:
    if g.h == 0.0:
        return math.inf
    return rnd64(1 / Fraction(g.h))


def seg_kernel(g: Geometry, t: float, short: bool = False) -> int:
    """Table::segment: int(fmin(fmax(t, 0), nseg - 1)) (NaN: 0). `short`: the defect of a
    clamp one segment short."""
    if t != t:
        return 0
    top = g.nseg - 1 - (1 if short and g.nseg > 1 else 0)
    return int(min(max(t, 0.0), float(top)))


def tile_midpoint(g: Geometry, tile: int, points: bool = False) -> float:
    """The fp64 midpoint a series tile is handed. lane_sum: fma(base + 64 tile + 31.5, h, a),
    one rounding; point_values_kernel: fma(31.5, h, fma(base + 64 tile, h, a)), two."""
    if points:
        return fma64(HSPAN, g.h, fma64(base_index(g) + 64.0 * tile, g.h, g.a))
    return fma64(base_index(g) + 64.0 * tile + HSPAN, g.h, g.a)


def tile_ends(g: Geometry, xm: float, short: bool = False):
    """Table::ends: the segments of the tile's first and last sample, and their coordinates."""
    x_lo, x_hi = fma64(-HSPAN, g.h, xm), fma64(HSPAN, g.h, xm)
    return seg_kernel(g, x_lo, short), seg_kernel(g, x_hi, short), x_lo, x_hi


def kind_of(lo: int, hi: int) -> str:
    return "line" if lo == hi else "kink" if hi == lo + 1 else "coarse"


def tile_kinds(g: Geometry, points: bool = False) -> list:
    """The branch every full 64-sample tile of a series launch takes, by the kernel's own
    coordinate operations."""
    out = []
    for t in range(g.count // TILE_SERIES):
        lo, hi, _, _ = tile_ends(g, tile_midpoint(g, t, points))
        out.append(kind_of(lo, hi))
    return out


def tile_census(g: Geometry, points: bool = False) -> dict:
    """{"line", "kink", "coarse": tiles; "rem": samples past the last whole tile}. Unlike
    exact_riemann.table_tile_census this works at any coordinates, dyadic or not."""
    kinds = tile_kinds(g, points)
    out = {k: kinds.count(k) for k in ("line", "kink", "coarse")}
    out["rem"] = g.count - len(kinds) * TILE_SERIES
    return out


def switch_margin(g: Geometry, points: bool = False) -> float:
    """The least distance, in ulps of the coordinate, between a full tile's end coordinate
    (fma(-+31.5, h, x_m)) and a knot 1 ... entries - 2: a case with a margin of a few ulps or
    more takes the same branch whichever way its coordinates round."""
    best = math.inf
    for t in range(g.count // TILE_SERIES):
        _, _, x_lo, x_hi = tile_ends(g, tile_midpoint(g, t, points))
        for x in (x_lo, x_hi):
            k = min(max(round(x), 1), g.nseg - 1) if g.nseg > 1 else None
            if k is not None:
                best = min(best, abs(x - k) / math.ulp(max(abs(x), 1.0)))
    return best


# ---------------------------------------------------------------------------- the definition
def _slope(v0: float, v1: float, f32_slope: bool) -> float:
    if f32_slope:     # the defect: both entries rounded to fp32 before the subtraction
        return rnd64(_fr(rnd32(_fr(v1))) - _fr(rnd32(_fr(v0))))
    return rnd64(_fr(v1) - _fr(v0))


def point_defined(g: Geometry, t: float, defect: tuple | None = None) -> Fraction:
    """What the per-sample form is defined to evaluate at the ROUNDED coordinate t: the exact
    line of the kernel's own segment of t. defect ("f32_slope",): the slope from fp32-rounded
    entries; ("clamp_short",): the end clamp one segment short."""
    kind = defect[0] if defect else None
    s = seg_kernel(g, t, short=kind == "clamp_short")
    v0, v1 = g.table[s], g.table[s + 1]
    d = _fr(_slope(v0, v1, True)) if kind == "f32_slope" else _fr(v1) - _fr(v0)
    return _fr(v0) + d * (_fr(t) - s)


def defined_tile(g: Geometry, tile: int = 0, points: bool = False, defect: tuple | None = None):
    """(kind, values): the 64 samples tile `tile` of a series launch is defined to evaluate, in
    sample order, as Fractions.

    defect mutates the definition (the defect tests; None is the definition):
      ("knot_half",)     the knot offset kk half a step off
      ("centres",)       the sub-tile centres at -+15.5 instead of -+16
      ("wrong_dd",)      the slope change taken at the neighbouring knot
      ("f32_slope",)     the slope formed from fp32-rounded entries
      ("clamp_short",)   the end clamp one segment short
    """
    kind = defect[0] if defect else None
    short = kind == "clamp_short"
    xm = tile_midpoint(g, tile, points)
    lo, hi, x_lo, _ = tile_ends(g, xm, short)
    branch = kind_of(lo, hi)
    if branch == "coarse":
        return branch, [point_defined(g, fma64(float(u), g.h, x_lo), defect)
                        for u in range(TILE_SERIES)]
    v = g.table
    d = _slope(v[lo], v[lo + 1], kind == "f32_slope")
    vm = _fr(fma64(d, rnd64(_fr(xm) - lo), v[lo]))
    D = _fr(rnd64(_fr(d) * _fr(g.h)))
    dD, kk = Fraction(0), Fraction(0)
    if branch == "kink":
        k0 = lo + 1
        if kind == "wrong_dd":
            k0 = lo + 2 if lo + 3 <= g.nseg else lo
        d_right = rnd64(_fr(v[k0 + 1]) - _fr(v[k0]))
        d_left = d if k0 == lo + 1 else rnd64(_fr(v[k0]) - _fr(v[k0 - 1]))
        dD = _fr(rnd64(_fr(rnd64(_fr(d_right) - _fr(d_left))) * _fr(g.h)))
        kk = _fr(rnd64(_fr(rnd64(Fraction(lo + 1) - _fr(xm))) * _fr(inv_h(g))))
        if kind == "knot_half":
            kk += Fraction(1, 2)
    vals = []
    for u in range(TILE_SERIES):
        k = Fraction(2 * u - 63, 2)
        if kind == "centres":
            k += Fraction(1, 2) if u < SUB else Fraction(-1, 2)
        val = vm + k * D
        if branch == "kink":
            val += max(k - kk, Fraction(0)) * dD
        vals.append(val)
    return branch, vals


# ---------------------------------------------------------------------------- emulation
def emulate_point(path: str, g: Geometry, t: float, F: F32 | None = None,
                  f32_slope: bool = False) -> float:
    """Table::point / TableF32::pointf at the fp64 coordinate t. f32_slope: pointf as it was
    before the slope was subtracted in fp64 (fmaf(fl32(v1) - fl32(v0), fr, fl32(v0)))."""
    s = seg_kernel(g, t)
    fr = rnd64(_fr(t) - s)
    v0, v1 = g.table[s], g.table[s + 1]
    if path.startswith("fp64"):
        return fma64(rnd64(_fr(v1) - _fr(v0)), fr, v0)
    F = F or F32()
    v0f = F.rnd(_fr(v0))
    d = F.add(F.rnd(_fr(v1)), -v0f) if f32_slope else F.rnd(_fr(rnd64(_fr(v1) - _fr(v0))))
    return F.fma(d, F.rnd(_fr(fr)), v0f)


def sample_coordinate(g: Geometry, i: int, roundings: int, T: int = TILE_PER_SAMPLE) -> float:
    """fma(base + i, h, a) (1: lane_sum's remainder loop) or fma(u, h, fma(base + i - u, h, a)),
    u = i mod T (2: a per-sample tile, the point kernel)."""
    if roundings == 1:
        return fma64(base_index(g) + float(i), g.h, g.a)
    u = i % T
    return fma64(float(u), g.h, fma64(base_index(g) + float(i - u), g.h, g.a))


def emulate_tile(path: str, g: Geometry, tile: int = 0, points: bool = False, fused: bool = False,
                 f32_slope: bool = False):
    """(tile sum, the values in sample order or None in fp32, fp32 denormal seen): one full tile
    of `path` operation by operation. `fused`: the compiler contracts r = c0 - A inv_h into one
    fma (HIP contracts by default; both are allowed)."""
    F = F32()
    f32 = path.startswith("fp32")
    if path.endswith("ieee"):
        x0 = fma64(base_index(g) + float(TILE_PER_SAMPLE * tile), g.h, g.a)
        vals = [emulate_point(path, g, fma64(float(u), g.h, x0), F, f32_slope)
                for u in range(TILE_PER_SAMPLE)]
        return _two_chains(vals, F if f32 else None), (None if f32 else vals), F.denormal
    xm = tile_midpoint(g, tile, points)
    lo, hi, x_lo, _ = tile_ends(g, xm)
    branch = kind_of(lo, hi)
    if branch == "coarse":
        vals = [emulate_point(path, g, fma64(float(u), g.h, x_lo), F, f32_slope)
                for u in range(TILE_SERIES)]
        return _two_chains(vals, F if f32 else None), (None if f32 else vals), F.denormal
    v = g.table
    d = rnd64(_fr(v[lo + 1]) - _fr(v[lo]))
    vm = fma64(d, rnd64(_fr(xm) - lo), v[lo])
    D = rnd64(_fr(d) * _fr(g.h))
    dD = A = 0.0
    if branch == "kink":
        dD = rnd64(_fr(rnd64(_fr(rnd64(_fr(v[lo + 2]) - _fr(v[lo + 1]))) - _fr(d))) * _fr(g.h))
        A = rnd64(Fraction(lo + 1) - _fr(xm))
    ih = inv_h(g)
    t, vals = 0.0, [None] * TILE_SERIES
    for q in range(2):
        c0 = -16.0 if q == 0 else 16.0
        vc = fma64(c0, D, vm)
        r = 0.0
        if branch == "kink":
            r = fma64(-A, ih, c0) if fused else rnd64(_fr(c0) - _fr(rnd64(_fr(A) * _fr(ih))))
        if not f32:
            for j in range(PAIRS):
                k = j + 0.5
                gp, gn = fma64(k, D, vc), fma64(-k, D, vc)
                if branch == "kink":
                    gp = fma64(max(r + k, 0.0), dD, gp)
                    gn = fma64(max(r - k, 0.0), dD, gn)
                t = (t + gp) + gn
                vals[q * SUB + SUB // 2 + j], vals[q * SUB + SUB // 2 - 1 - j] = gp, gn
            continue
        Df, dDf, vcf, rf = F.rnd(_fr(D)), F.rnd(_fr(dD)), F.rnd(_fr(vc)), F.rnd(_fr(r))
        a = [0.0, 0.0]
        for j in range(PAIRS):
            k = j + 0.5
            pair = [F.fma(k, Df, vcf), F.fma(-k, Df, vcf)]
            if branch == "kink":
                pair[0] = F.fma(max(F.add(rf, k), 0.0), dDf, pair[0])
                pair[1] = F.fma(max(F.add(rf, -k), 0.0), dDf, pair[1])
            a = [F.add(a[0], pair[0]), F.add(a[1], pair[1])]
        t = t + (a[0] + a[1])
    return t, (None if f32 else vals), F.denormal


def _two_chains(vals, F: F32 | None) -> float:
    """acc0 += even samples, acc1 += odd samples, acc0 + acc1 (fp32: two fp32 chains joined in
    fp64)."""
    a = [0.0, 0.0]
    for u, v in enumerate(vals):
        a[u & 1] = F.add(a[u & 1], v) if F else a[u & 1] + v
    return a[0] + a[1]


def emulate_fill(g_table: tuple, dt: float, i: int) -> float:
    """interp_fill_kernel's sample i: t = fl(dt i), seg_of, fma(fl(v1 - v0), fl(t - k), v0)."""
    t = rnd64(_fr(dt) * i)
    nseg = len(g_table) - 1
    k = nseg - 1 if t >= float(nseg) else (0 if t < 1.0 else int(t))
    v0 = g_table[k]
    return fma64(rnd64(_fr(g_table[k + 1]) - _fr(v0)), rnd64(_fr(t) - k), v0)


# ---------------------------------------------------------------------------- bounds
class _Segs:
    """Per-segment sizes of a table, each the largest over the segment and its two neighbours
    (a sample's rounded coordinate, and the tile that holds it, may sit one segment over):
    dn = |d|; W = |d_s| + the larger slope change |d_s - d_{s-+1}| at the segment's own knots."""

    def __init__(self, table):
        self.v = np.asarray(table, dtype=np.float64)
        self.d = np.diff(self.v)
        n = self.d.size
        ad = np.abs(self.d)
        dd = np.abs(np.diff(self.d))                     # at the knots 1 ... n - 1
        jump = np.zeros(n)
        if n > 1:
            jump[:-1] = dd
            jump[1:] = np.maximum(jump[1:], dd)
        self.dn = self._neigh(ad)
        self.W = self._neigh(ad + jump)
        self.n = n

    @staticmethod
    def _neigh(a):
        p = np.pad(a, 1, mode="edge")
        return np.maximum(np.maximum(p[:-2], p[1:-1]), p[2:])

    def seg(self, x):
        return np.clip(np.floor(x), 0, self.n - 1).astype(np.int64)

    def sizes(self, s, x):
        """(W, M, dn) of samples at x in segment s. A sample within one unit of the table,
        -1 <= x <= entries, takes the neighbours in: M = max over t in {s - 1, s, s + 1} of |v_t|
        + |d_t| |x - t|. Further out on an extrapolating end segment no rounding can reach
        another segment, and only the sample's own line counts: W = dn = |d_s|, M = |v_s| + |d_s|
        |x - s|."""
        x = np.asarray(x, dtype=np.float64)
        own = np.abs(self.v[s]) + np.abs(self.d[s]) * np.abs(x - s)
        M = own
        for o in (-1, 1):
            t = np.clip(s + o, 0, self.n - 1)
            M = np.maximum(M, np.abs(self.v[t]) + np.abs(self.d[t]) * np.abs(x - t))
        near = (x >= -1.0) & (x <= self.n + 1.0)
        ad = np.abs(self.d[s])
        return (np.where(near, self.W[s], ad), np.where(near, M, own) * SECOND_ORDER,
                np.where(near, self.dn[s], ad))


def _terms(fp32: bool, form: str, W, M, K, ulp: float, rm: int):
    """|computed - v(x_i)| of one sample. W, M, K as in _Segs and the module docstring, ulp the
    ulp of the launch's largest coordinate, rm the roundings of the coordinate the form starts
    from (x_m of a tile: 1 in a launch, 2 in the point kernel; a per-sample coordinate: 1 or 2).

    Coordinates. v is continuous and piecewise linear, so a coordinate off by e costs at most
    (the local slope) e; where the sample's own segment and the one the kernel read differ
    because a rounded coordinate fell across a knot, the two lines differ by |slope change|
    times the distance to the knot, which is at most e too: W e in all.
      point  (Table::point at a rounded coordinate; the coarse branch):  e = rm ulp / 2
             fr = t - i is exact up to ulp(t) > 1: U64 |d| |fr|; d = fl(v1 - v0): U64 |d| |fr|;
             the fma: U64 |result|:                                      3 U64 M
      fp32   fr, d and v0 each converted once (d after its fp64 subtraction), fmaf:
             3 U32 M + 3 U64 M + floor
      line   the samples sit at x_m + k h exactly: e = rm ulp / 2 for x_m, and one more
             ulp / 2 for the end coordinates that chose the branch (a sample a rounding past
             the knot is read off the neighbouring line).
             fl(x_m - lo), d, v_m, D = fl(d h) (relative U64 of k D), v_c = fma(c0, D, v_m),
             the sample fma: 6 roundings of quantities <= M + K:         6 U64 (M + K)
      fp32   v_m and v_c in fp64 as above (5 U64), then v_c, D converted and the pk_fma:
             3 U32 (M + K) + floor
      kink   line, and the kink term over dD, over = max(r +- k, 0) <= 63, |dD| <= 2 max|d| |h|,
             so |over dD| <= 2 K:
             dD: two subtractions at the size |d0| + |d1| and one product: 3 roundings, 6 U64 K;
             kk: fl(lo + 1 - x_m), fl(1 / h) and the product, |kk| <= 32: 3 U64 32 |dD| <= 3 U64 K;
             r = fl(c0 - kk), |r| <= 48 (fused or not: one rounding less): 1.5 U64 K;
             r +- k, <= 64: 2 U64 K;  the second fma: U64 (M + K):       U64 (M + K) + 12.5 U64 K
      fp32   dD and kk in fp64 (9 U64 K); dD converted (2 U32 K), r converted (1.5 U32 K),
             r +- k in fp32 (2 U32 K), the second pk_fma U32 (M + K):
             U32 (M + K) + 5.5 U32 K + 9 U64 K
      any    the larger of kink and the coarse branch's point form at rm + 2 roundings (x0 =
             fma(-31.5, h, x_m), then fma(u, h, x0)): what a launch's series tiles can cost
             without knowing each tile's branch.
    floor: an fp32 result below 2**-126 loses up to 2**-149 (gradual underflow); the half dozen
    fp32 results of a sample are multiplied by at most 64 on their way: 128 2**-149."""
    MK = M + K
    if form == "point":
        e = W * (rm * 0.5 * ulp) + 3.0 * U64 * M
        return e + (3.0 * U32 * M + F32_FLOOR if fp32 else 0.0)
    if form == "any":
        return np.maximum(_terms(fp32, "kink", W, M, K, ulp, rm),
                          _terms(fp32, "point", W, M, K, ulp, rm + 2))
    coord = W * ((rm + 1) * 0.5 * ulp)
    if not fp32:
        e = coord + 6.0 * U64 * MK
        if form == "kink":
            e = e + U64 * MK + 12.5 * U64 * K
        return e
    e = coord + 5.0 * U64 * MK + 3.0 * U32 * MK + F32_FLOOR
    if form == "kink":
        e = e + U32 * MK + 5.5 * U32 * K + 9.0 * U64 * K
    return e


def _launch_ulp(g: Geometry) -> float:
    return math.ulp(g.x_abs_max + 64.0 * abs(g.h))


def sample_bounds(path: str, g: Geometry, points: bool = False) -> np.ndarray:
    """|computed - v(x_i)| for every sample of the launch (_terms): the samples of the launch's
    full tiles by the branch their tile takes (tile_kinds: the kernel's own coordinate
    operations), the rest by the per-sample form (lane_sum's remainder loop at one rounding; in
    the point kernel, whose coordinates round once more, a partial tile)."""
    S = _Segs(g.table)
    idx = np.arange(g.count, dtype=np.float64) + (float(g.i_begin) + float(g.off))
    x = g.a + idx * g.h
    W, M, dn = S.sizes(S.seg(x), x)
    K = 64.0 * abs(g.h) * dn
    fp32 = path.startswith("fp32")
    ulp = _launch_ulp(g)
    T = tile_len(path)
    full = (g.count // T) * T
    out = _terms(fp32, "point", W, M, K, ulp, 2 if points else 1)
    if full and path.endswith("ieee"):
        out[:full] = _terms(fp32, "point", W[:full], M[:full], K[:full], ulp, 2)
    elif full:
        kinds = np.repeat(np.array(tile_kinds(g, points)), T)
        rm = 2 if points else 1
        for form in ("line", "kink"):
            m = np.flatnonzero(kinds == form)
            out[m] = _terms(fp32, form, W[m], M[m], K[m], ulp, rm)
        m = np.flatnonzero(kinds == "coarse")
        out[m] = _terms(fp32, "point", W[m], M[m], K[m], ulp, rm + 2)
    return out * SECOND_ORDER


def _aggregate(path: str, g: Geometry, form: str, rm: int):
    """(sum of the per-sample bounds, S = sum of M + K) over the launch, segment by segment: a
    segment's m samples each at the segment's largest magnitude (M is convex in x: at the
    first or the last of them). This is what makes a 1e9-sample bound cost nothing."""
    S = _Segs(g.table)
    x0, h, ranges = segment_ranges(g)
    s = np.array([r[0] for r in ranges], dtype=np.int64)
    m = np.array([r[2] - r[1] for r in ranges], dtype=np.float64)
    xa = np.array([float(x0 + r[1] * h) for r in ranges])
    xb = np.array([float(x0 + (r[2] - 1) * h) for r in ranges])
    Wa, Ma, da = S.sizes(s, xa)
    Wb, Mb, db = S.sizes(s, xb)
    W, M, K = np.maximum(Wa, Wb), np.maximum(Ma, Mb), 64.0 * abs(g.h) * np.maximum(da, db)
    e = _terms(path.startswith("fp32"), form, W, M, K, _launch_ulp(g), rm)
    return float(np.sum(m * e)), float(np.sum(m * (M + K)))


def launch_magnitude(g: Geometry) -> float:
    """sum_i (M + K): the size a launch's bound is held against (never |v|: it has zeros)."""
    return _aggregate("fp64-ieee", g, "point", 1)[1]


def launch_sum_bound(path: str, g: Geometry, grid: int, block: int = BLOCK) -> float:
    """ABSOLUTE bound of the sum of a launch's partials against true_sum: the per-sample bounds
    summed (series: form `any`; ieee: the per-sample form at two roundings), and the additions,
    every one rounding at most U of a partial sum of |values| <= S:
      fp64 series   the 64-term running sum t: 63 U64 (coarse: two chains of 32 and their join);
      fp64 ieee     two chains of 16 and their join: 16 U64;
      fp32 series   16 fp32 additions into each lane of `a` per sub-tile, or the coarse
                    branch's two fp32 chains of 32: 32 U32; the fold and t += fold: 2 U64;
      fp32 ieee     two fp32 chains of 16: 16 U32; their fp64 join: U64;
      all           launch_depth further fp64 additions (acc + t, the lanes, the partials)."""
    series = path.endswith("series")
    total, S = _aggregate(path, g, "any" if series else "point", 1 if series else 2)
    if path.startswith("fp32"):
        adds = (32.0 if series else 16.0) * U32 + 2.0 * U64
    else:
        adds = (63.0 if series else 16.0) * U64
    adds += launch_depth(g.count, tile_len(path), grid, block) * U64
    return (total + adds * S) * SECOND_ORDER


def launch_value_bound(path: str, g: Geometry, grid: int, block: int = BLOCK) -> float:
    """ABSOLUTE bound of a launch's VALUE, h sum, against true_value: launch_sum_bound times |h|
    and U64 of the value for the multiplication (tot * scale)."""
    S = launch_magnitude(g)
    return abs(g.h) * (launch_sum_bound(path, g, grid, block) + U64 * S) * SECOND_ORDER


def host_value_bound(g: Geometry, threads: int = 1) -> float:
    """The host engine (host_kernels.inc feval<4>, sum_slice_t): the per-sample form at one
    coordinate rounding; 8 lane accumulators over blocks of 4096 samples (512 additions), the
    3-level lane sum, the compensated block total (counted as plain additions: one per block
    and its correction) and the threads' slices; then h * sum."""
    total, S = _aggregate("fp64-ieee", g, "point", 1)
    depth = HOST_BLOCK // 8 + 3 + 2 * -(-g.count // HOST_BLOCK) + threads
    return abs(g.h) * (total + (depth + 1) * U64 * S) * SECOND_ORDER * SECOND_ORDER


def fill_true(table: tuple, dt: float, i: int) -> Fraction:
    g = Geometry(0.0, dt, Fraction(0), 0, 1, tuple(table))
    return interp_exact(g, Fraction(dt) * i)


def fill_bounds(table: tuple, dt: float, i0: int, n: int) -> np.ndarray:
    """interp_fill against the truth at the exact dt i: t = fl(dt i) is one rounding (i < 2**53
    is exact as a double), ulp(t) / 2 times W, and the per-sample form's 3 U64 M."""
    S = _Segs(table)
    t = dt * (np.arange(n, dtype=np.float64) + float(i0))
    W, M, _ = S.sizes(S.seg(t), t)
    ulp = math.ulp(dt * float(i0 + n))
    return _terms(False, "point", W, M, 0.0, ulp, 1) * SECOND_ORDER
