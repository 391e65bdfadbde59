"""True values of the sin and train-velocity Riemann kernels, and derived error bounds.

The sibling of exact_riemann.py for the two integrands that have no exact inputs: sin(x) and
v(t) = vs (1 - cos(t / ts)) (csrc/include/miint/integrands.hpp, integrands_f32.hpp,
fast_trig.hpp). Pure Python and mpmath at a fixed 200-bit precision; no GPU, no torch.

Coordinates. The kernel's fp64 a, its fp64 h = (b - a) / n and ts, vs are taken as exact
reals: sample i of a launch sits at x_i = a + (i_begin + i + off) h (off = 0, 1/2, 1) and
its angle is theta_i = x_i (sin) or x_i / ts (train), an arithmetic progression of step
delta = h or h / ts. What a kernel makes of these in fp64 (the rounding of a coordinate, of
1 / ts, of t * (1 / ts)) is the kernel's error and is bounded below, never folded into the
truth.

    g = geometry(spec, n, "mid", i_begin, count)
    vals, exact = true_values(spec, n, "mid", i_begin, count)   # fp64 array, list of mpf
    s = true_sum(spec, n, "mid", i_begin, count)                # mpf: sum of f, unscaled

Sums use the closed form of a trigonometric progression,
    sum_{i<m} sin(t0 + i d) = sin(t0 + (m - 1) d / 2) sin(m d / 2) / sin(d / 2)
(cos alike), so N = 1e10 costs what N = 10 does.

Bounds. Every helper returns an ABSOLUTE bound and derives it in its docstring from the
operations of the code, with U64 = 2**-53 and U32 = 2**-24 the relative error of one
rounding (half an ulp of a value below 1 is U / 2). Nothing in them is taken from a kernel's
output. They are worst-case sums of the individual roundings, not statistical estimates.
"""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction

import mpmath
import numpy as np

PREC = 200
MP = mpmath.MPContext()
MP.prec = PREC

U64 = 2.0 ** -53
U32 = 2.0 ** -24
SQRT2 = math.sqrt(2.0)
RULE_OFF = {"left": Fraction(0), "mid": Fraction(1, 2), "right": Fraction(1)}

# tile_sincos's pi/2 = hi + lo (integrands.hpp): what the pair misses per quadrant
PIO2_HI = float.fromhex("0x1.921fb544p+0")
PIO2_LO = 6.07710050650619224932e-11
PIO2_RESIDUAL = float(abs(MP.pi / 2 - MP.mpf(PIO2_HI) - MP.mpf(PIO2_LO)))   # 3.6e-27
TWO_OVER_PI = 6.36619772367581382433e-01
# fast_trig.hpp
PIO2_P1 = 1.57079632673412561417e+00
PIO2_P2 = 6.07710050630396597660e-11
FAST_TRIG_MAX_N = 65536.0
# kernels.hpp: the series tiles run while both end angles have |n| <= this many quadrants
TRIG_SERIES_MAX_N = 2.0 ** 31 - 2.0 ** 16

# tile lengths (asserted against the extension's riemann_tile_len in the tests)
SERIES_TILE = {"sin": 192, "train": 128}
IEEE_TILE = 32
LIB_ULPS = 2.0   # library sin / cos (ocml), fp64 and fp32: see ieee_value_bound


def _mpq(fr: Fraction):
    return MP.mpf(fr.numerator) / MP.mpf(fr.denominator)


@dataclasses.dataclass(frozen=True)
class Geometry:
    """The samples of one launch: x_i = a + (i_begin + i + off) h, i < count, exactly."""
    name: str
    a: float
    h: float
    off: Fraction
    i_begin: int
    count: int
    ts: float
    vs: float

    def x(self, i: int) -> Fraction:
        return Fraction(self.a) + (self.i_begin + i + self.off) * Fraction(self.h)

    @property
    def omega(self):
        return MP.mpf(1) if self.name == "sin" else MP.mpf(1) / MP.mpf(self.ts)

    def theta(self, i):
        """theta of sample i (i may be a Fraction: tile midpoints)."""
        x = Fraction(self.a) + (self.i_begin + Fraction(i) + self.off) * Fraction(self.h)
        return _mpq(x) * self.omega

    @property
    def delta(self):
        return MP.mpf(self.h) * self.omega

    @property
    def x_abs_max(self) -> float:
        return float(max(abs(self.x(0)), abs(self.x(self.count - 1))))

    @property
    def theta_abs_max(self) -> float:
        return float(max(abs(self.theta(0)), abs(self.theta(self.count - 1))))

    @property
    def quadrants(self) -> float:
        """|n| = |theta| 2 / pi at the farther end."""
        return self.theta_abs_max * TWO_OVER_PI

    @property
    def amp(self) -> float:
        """max |f|: 1 for sin, 2 |vs| for the train velocity."""
        return 1.0 if self.name == "sin" else 2.0 * abs(self.vs)

    @property
    def gain(self) -> float:
        """|d f / d (trig value)|: 1 for sin, |vs| for the train velocity."""
        return 1.0 if self.name == "sin" else abs(self.vs)


def geometry(spec, n: int, rule: str, i_begin: int = 0, count: int | None = None) -> Geometry:
    if spec.name not in ("sin", "train"):
        raise ValueError("trig_truth covers sin and train")
    h = (spec.b - spec.a) / n          # as ops/kernels.py and RiemannPlan form it
    count = n if count is None else count
    if count < 1 or i_begin < 0:
        raise ValueError("need count >= 1 and i_begin >= 0")
    return Geometry(spec.name, float(spec.a), h, RULE_OFF[rule], int(i_begin), int(count),
                    float(spec.p0) if spec.name == "train" else 1.0,
                    float(spec.p1) if spec.name == "train" else 1.0)


# ---------------------------------------------------------------------------- the truth
def _f(g: Geometry, th):
    return MP.sin(th) if g.name == "sin" else MP.mpf(g.vs) * (1 - MP.cos(th))


def true_values(spec, n, rule, i_begin=0, count=None):
    """(fp64 array, list of mpf): f at every sample of the launch, rounded to fp64 at the
    very end only."""
    g = geometry(spec, n, rule, i_begin, count)
    exact = [_f(g, g.theta(i)) for i in range(g.count)]
    return np.array([float(v) for v in exact], dtype=np.float64), exact


def true_trig(spec, n, rule, i_begin=0, count=None):
    """(trig, slope) as fp64 arrays: the trig value each sample's f is made of (sin theta; the
    train's cos theta) and d f / d i = delta f'(theta_i), what moving a sample by one step is
    worth (the sensitivity of a sum to a misplaced sample)."""
    g = geometry(spec, n, rule, i_begin, count)
    th = [g.theta(i) for i in range(g.count)]
    if g.name == "sin":
        trig = [MP.sin(t) for t in th]
        slope = [g.delta * MP.cos(t) for t in th]
    else:
        trig = [MP.cos(t) for t in th]
        slope = [g.delta * MP.mpf(g.vs) * MP.sin(t) for t in th]
    return (np.array([float(v) for v in trig]), np.array([float(v) for v in slope]))


def trig_progression_sum(t0, d, m: int, cos: bool):
    """sum_{i<m} sin (or cos) (t0 + i d) by the closed form. Raises where sin(d / 2) is too
    small for 200 bits to carry it (|sin(d/2)| 2**100 < max(1, |t0| + m |d|): the quotient
    would lose more than half the working precision)."""
    t0, d = MP.mpf(t0), MP.mpf(d)
    s = MP.sin(d / 2)
    if abs(s) * MP.mpf(2) ** 100 < max(MP.mpf(1), abs(t0) + m * abs(d)):
        raise ValueError("closed form ill-conditioned: sin(delta / 2) too close to zero")
    mid = t0 + (m - 1) * d / 2
    return (MP.cos(mid) if cos else MP.sin(mid)) * MP.sin(m * d / 2) / s


def true_sum(spec, n, rule, i_begin=0, count=None):
    """mpf: sum of f over the launch's samples (unscaled: what the partials add up to)."""
    g = geometry(spec, n, rule, i_begin, count)
    if g.name == "sin":
        return trig_progression_sum(g.theta(0), g.delta, g.count, cos=False)
    return MP.mpf(g.vs) * (g.count - trig_progression_sum(g.theta(0), g.delta, g.count, cos=True))


def true_value(spec, n, rule, i_begin=0, count=None):
    """mpf: h * sum, what a launch returns."""
    return MP.mpf(geometry(spec, n, rule, i_begin, count).h) * true_sum(spec, n, rule, i_begin, count)


def brute_sum(spec, n, rule, i_begin=0, count=None):
    """mpf: the same sum sample by sample (the closed form's check; small counts)."""
    g = geometry(spec, n, rule, i_begin, count)
    return MP.fsum(_f(g, g.theta(i)) for i in range(g.count))


def abs_sum_bound(g: Geometry) -> float:
    """A >= sum |f(x_i)|: count * max |f| (no closed form for the absolute values)."""
    return g.count * g.amp


# ---------------------------------------------------------------------------- coordinates
def _pow2(v: float) -> bool:
    return v != 0.0 and math.frexp(abs(v))[0] == 0.5


def coords_exact(g: Geometry) -> bool:
    """True when every coordinate the kernels form for this launch is a double: h = 2**-k, a
    a multiple of h / 2 (samples under any rule, and the midpoints of even-length tiles, sit
    on the grid h / 2), and |x| / (h / 2) < 2**53 at the farther end, half a tile beyond it
    included. Then fma(index, h, a) and fma(u, h, x0) return their exact values."""
    if not _pow2(g.h):
        return False
    q = Fraction(abs(g.h)) / 2
    if (Fraction(g.a) / q).denominator != 1:
        return False
    far = max(abs(g.x(0)), abs(g.x(g.count - 1))) + 256 * Fraction(abs(g.h))
    return far / q < 2 ** 53


def angle_exact(g: Geometry) -> bool:
    """True when theta = x (1 / ts) is formed exactly: sin, or ts a power of two."""
    return g.name == "sin" or _pow2(g.ts)


def angle_input_bound(g: Geometry, roundings: int) -> float:
    """Error of the fp64 angle a path evaluates, against the true theta of that sample.

    Coordinates: each fma that forms a coordinate rounds once, <= ulp(x) / 2 at the launch's
    farther end; `roundings` of them (1: the series tiles' midpoint fma(ib, h, a); 2: the
    per-sample tiles' and point_values' fma(u, h, fma(ib, h, a))). Zero where coords_exact.
    Train: theta = fl(x * fl(1 / ts)): the coordinate error times |1 / ts|, then
    |theta| U64 for the rounding of 1 / ts and |theta| U64 for the product (zero for ts a power
    of two, where both are exact), with (1 + 2 U64) for their interplay."""
    ex = 0.0 if coords_exact(g) else roundings * 0.5 * math.ulp(g.x_abs_max)
    if g.name == "sin":
        return ex
    e = ex / abs(g.ts)
    if not angle_exact(g):
        e = e * (1.0 + U64) + 2.0 * U64 * g.theta_abs_max * (1.0 + 2.0 * U64)
    return e


# ---------------------------------------------------------------------------- series tiles
def reduction_bound(nq: float) -> float:
    """tile_sincos's reduced angle r against theta - n pi / 2 (n = rint(theta 2 / pi)):
    fma(-n, hi, theta) is exact (hi has 33 bits, so n hi needs at most 33 + 31 bits and the
    difference, below 1 in magnitude, is a multiple of min(ulp(theta), 2**-32)); fma(-n, lo, .)
    rounds once, <= ulp(r) / 2 <= 2**-54 (|r| < 1); and hi + lo misses pi / 2 by
    PIO2_RESIDUAL = 3.6e-27 per quadrant."""
    return 2.0 ** -54 + abs(nq) * PIO2_RESIDUAL


def seed_bound(nq: float) -> float:
    """Each of S and C from tile_sincos against sin / cos of its input angle: the fdlibm
    kernels are < 1 ulp of a value below 1 (2**-53), and an error e of the reduced angle
    moves sin and cos by at most e."""
    return 2.0 ** -53 + reduction_bound(nq)


def series_point_bound(nq: float, fp32: bool = False) -> float:
    """One sin / cos sample of an angle-addition tile against the true value at the tile's
    input midpoint angle plus the sample's exact offset (AngleSeries / AngleSeriesF32), with
    u = U64 or U32:

    seed      (S, C) each within e_s = seed_bound(nq), in fp32 plus u / 2 for the rounding of
              S and C to fp32; as a vector at most sqrt(2) e_s, and a rotation keeps that.
    centre    S_q = fma(C, s, S c): the table's c = cos(c0 d), s = sin(c0 d) are rounded from
              long double (relative u; fp32: through fp64, (1 + 2**-29) u, absorbed below),
              moving S_q by at most u (|S c| + |C s|) <= sqrt(2) u; the product and the fma
              round once each at a value below 1, u / 2 + u / 2. Per component t + r with
              t = sqrt(2) u and r = u; as a vector sqrt(2) (t + r).
    pair      fma(+-side, sk, base ck): the same again for one component, t + r.

    Total sqrt(2) e_s + (sqrt(2) + 1) (sqrt(2) + 1) u: in fp64 for |theta| <= 1e5
    2.12 U64 + 5.83 U64 = 7.95 U64 = 8.8e-16, inside the 4 ulp(1) = 8.9e-16 the project
    measures against ocml; in fp32 6.54 U32 = 3.9e-7."""
    u = U32 if fp32 else U64
    es = seed_bound(nq) + (u / 2 if fp32 else 0.0)
    return SQRT2 * es + (SQRT2 + 1.0) ** 2 * u * (1.0 + 2.0 ** -20)


def _wrap_train(g: Geometry, e_cos_sum: float, terms: int, total_abs: float, u: float) -> float:
    """vs (terms - sum cos) by fma(-vs, sum, fma(vs, terms, acc)) (tile_acc) or
    fma(-vs, c, vs * terms) (the per-sample tile): |vs| times the cosine sum's error, one
    rounding at |vs| terms and one at the result."""
    return abs(g.vs) * e_cos_sum + u * (abs(g.vs) * terms + total_abs)


def series_tile_bound(g: Geometry, fp32: bool = False, abs_sum: float | None = None) -> float:
    """partials[0] of a single-tile series launch (g.count = T samples) against true_sum.

    T samples at series_point_bound each; the tile's midpoint angle off by
    angle_input_bound(g, 1), which moves every sample by as much (|d sin| <= |d theta|);
    fp64: T additions into one accumulator, each rounding at most U64 times the running sum,
    itself at most A = sum |trig_i| <= T (`abs_sum`, in units of the trig values); fp32: the two
    packed accumulators take T / 2 additions each of U32 times at most their own share of A,
    (T / 2) U32 A in all, then two exact conversions and one fp64 addition. The train
    velocity wraps the cosine sum (_wrap_train, fp64 in both types)."""
    T = g.count
    A = float(T) if abs_sum is None else abs_sum
    e = T * (series_point_bound(g.quadrants, fp32) + angle_input_bound(g, 1))
    e += (T / 2 * U32 * A + U64 * A) if fp32 else T * U64 * A
    return e if g.name == "sin" else _wrap_train(g, e, T, 2.0 * abs(g.vs) * T, U64)


def series_value_point_bound(g: Geometry) -> float:
    """One value of point_values(div='series') against the truth: series_point_bound, the
    midpoint angle's two coordinate roundings (x0 = fma(ib, h, a), xm = fma((T - 1) / 2, h,
    x0)), and for the train velocity (1 - c) vs: |vs| (e_c + U64) for the subtraction's
    rounding (a value of at most 2) and U64 |v| for the product."""
    e = series_point_bound(g.quadrants) + angle_input_bound(g, 2)
    return e if g.name == "sin" else abs(g.vs) * (e + U64) + U64 * g.amp


# ---------------------------------------------------------------------------- per-sample tiles
def ieee_tile_fast(th0: float, th1: float) -> bool:
    """fast_trig.hpp's trig_tile on the tile's first and last angle, operation for operation
    (Python floats are fp64, round() is rint): True where the tile runs the fdlibm kernels
    with the Cody-Waite tail, False where it hands its samples to the library."""
    n = float(round(th0 * TWO_OVER_PI))
    if n != float(round(th1 * TWO_OVER_PI)) or not abs(n) <= FAST_TRIG_MAX_N:
        return False
    c1, t = n * PIO2_P1, n * PIO2_P2
    r0, r1, at = th0 - c1, th1 - c1, abs(t)
    return not (at > 0.0 and not (abs(r0) >= at and abs(r1) >= at and (r0 >= 0.0) == (r1 >= 0.0)))


def ieee_value_bound(v: float, fast: bool, fp32: bool = False) -> float:
    """A per-sample sin / cos against the true value at its input angle: the fdlibm kernels
    with the reduction's tail are < 1 ulp of the value (fast_trig.hpp; the project measures
    < 0.9 on the host twin, which is a measurement, so the bound keeps fdlibm's 1); the
    library's sin / cos are taken at LIB_ULPS = 2 ulp, fp64 and fp32 (ocml documents no
    tighter figure over its whole range). ulp of the true value, never below that of the
    smallest normal."""
    if fp32:
        a = max(abs(v), 2.0 ** -126)
        return LIB_ULPS * 2.0 ** (math.frexp(a)[1] - 24)
    return (1.0 if fast else LIB_ULPS) * math.ulp(max(abs(v), 2.0 ** -1022))


def ieee_point_bound(g: Geometry, trig_true: float, fast: bool) -> float:
    """One value of point_values(div='ieee') against the truth: ieee_value_bound at the true
    trig value, the angle's two coordinate roundings (angle_input_bound(g, 2)), and the train
    velocity's (1 - c) vs as in series_value_point_bound."""
    e = ieee_value_bound(trig_true, fast) + angle_input_bound(g, 2)
    return e if g.name == "sin" else abs(g.vs) * (e + U64) + U64 * g.amp


def _ieee_per_sample(g: Geometry, fp32: bool) -> float:
    """One term of a per-sample tile's sum, in units of f (see ieee_tile_bound)."""
    ang = angle_input_bound(g, 2)
    if not fp32:
        return g.gain * (LIB_ULPS * U64 + ang)
    ang += 0.5 * 2.0 ** (math.frexp(max(g.theta_abs_max, 2.0 ** -126))[1] - 24)
    per = LIB_ULPS * U32 + ang
    return per if g.name == "sin" else abs(g.vs) * (per + U32) + 2.0 * U32 * g.amp


def ieee_tile_bound(g: Geometry, fp32: bool = False, abs_sum: float | None = None) -> float:
    """partials[0] of a single-tile per-sample launch (g.count = 32) against true_sum.

    fp64 (trig_tile_sum): every sample within LIB_ULPS ulp of a value below 1 (the looser of
    the two evaluators) plus angle_input_bound(g, 2); two chains of T / 2 additions and one
    to join them, each at most U64 A (A = sum |trig_i| <= T); the train wraps the cosine sum
    (_wrap_train).
    fp32 (SinF32 / TrainVelF32::tile): the angle is rounded to fp32 first, ulp32(theta) / 2
    on top of the fp64 angle error; sinf / cosf within LIB_ULPS U32; for the train each term
    (1 - c) v rounds the subtraction (U32 at a value up to 2), the product and v = fl32(vs)
    (2 U32 of the term); two fp32 chains of T / 2 additions, (T / 2) U32 A in all with
    A = sum |f_i|, and one fp64 addition."""
    T = g.count
    if not fp32:
        A = float(T) if abs_sum is None else abs_sum
        e = T * _ieee_per_sample(g, False) / g.gain + (T / 2 + 1) * U64 * A
        return e if g.name == "sin" else _wrap_train(g, e, T, 2.0 * abs(g.vs) * T, U64)
    A = T * g.amp if abs_sum is None else abs_sum
    return T * _ieee_per_sample(g, True) + T / 2 * U32 * A + U64 * A


# ---------------------------------------------------------------------------- whole launches
def launch_depth(count: int, tile: int, grid: int, block: int = 256, fin_block: int = 256) -> int:
    """The longest chain of fp64 additions between one tile sum and the launch's result
    (riemann.hip lane_sum, wave_reduce.hpp, finalize): a lane adds its ceil(tiles / lanes)
    tile sums and its share of the < T remainder samples; 6 DPP steps across the wave and up
    to 4 across the workgroup's waves; the finalize adds ceil(grid / fin_block) partials per
    thread, then the same 10 steps."""
    lanes = grid * block
    tiles = count // tile
    rem = count - tiles * tile
    return (-(-tiles // lanes) + -(-rem // lanes)) + 10 + -(-grid // fin_block) + 10


def launch_value_bound(g: Geometry, div: str, fp32: bool, grid: int, block: int = 256,
                       abs_sum: float | None = None) -> float:
    """h * sum of a whole launch of path (`div`, fp32 or fp64) against true_value.

    Full tiles: every sample at the path's per-sample figure (series: series_point_bound
    plus the midpoint angle's one rounding, times |vs| for the train; per-sample tiles:
    _ieee_per_sample). The < T remainder samples run f.point, the library per sample
    (_ieee_per_sample, in fp32 with its fp32 coordinate). Inside the tiles the additions cost
    T U64 A (fp64 series), (T / 2) U32 A (packed series) or (T / 2 + 1) U64 A and
    (T / 2) U32 A (per-sample), A = sum |f_i| <= count max |f|: the tile bounds above without
    their per-sample part, summed over the tiles; the train tile's two fma roundings add
    2 U64 (|vs| T + |tile|) <= 3 U64 max |f| T per tile, 3 U64 A' with A' = count max |f|.
    Between tile and result launch_depth additions of U64 A each (any order of summation
    rounds at most depth * U64 * sum |terms|); times |h|, and U64 of the value for the final
    multiplication by the scale."""
    A = abs_sum_bound(g) if abs_sum is None else abs_sum
    rem_per = _ieee_per_sample(g, fp32)
    if div == "series":
        T = SERIES_TILE[g.name]
        per = g.gain * (series_point_bound(g.quadrants, fp32) + angle_input_bound(g, 1))
        inner = T / 2 * U32 + U64 if fp32 else T * U64
    else:
        T = IEEE_TILE
        per = rem_per
        inner = T / 2 * U32 + U64 if fp32 else (T / 2 + 1) * U64
    full = (g.count // T) * T
    e = full * per + (g.count - full) * rem_per
    e += (inner + launch_depth(g.count, T, grid, block, block) * U64) * A * (1.0 + 2.0 ** -20)
    if g.name == "train":
        e += 3.0 * U64 * abs_sum_bound(g)
    return abs(g.h) * (e + U64 * A)


# ---------------------------------------------------------------------------- the host twin
HOST_BLOCK = 4096        # host.cpp kHostBlock: samples per compensated block
HOST_FAST_MAX = 1.0e5    # host_kernels.inc vsincos: |x| beyond it goes to libm per lane


def host_value_bound(g: Geometry, threads: int) -> float:
    """host_riemann (host.cpp, host_kernels.inc) over the launch's samples against true_value.

    Per sample: vsincos is tile_sincos's reduction and kernels per lane, seed_bound at
    min(|n|, 1e5 2 / pi) quadrants (beyond 1e5 libm, within 1 ulp: no looser); the coordinate
    fma(idx, h, a) rounds once and the train's x / ts once more (angle_input_bound(g, 1),
    which charges the device's two roundings of the angle); the train's 1 - c rounds at a
    value up to 2 (U64); vs multiplies the whole sum. Sum: 8 lane accumulators of at most
    HOST_BLOCK / 8 additions, 3 in the pairwise lane sum, 2 per block in the compensated
    total (counted as plain additions: the compensation only helps), one per thread; each at
    most U64 A. Then h and the scale: 2 U64 of the value."""
    per = seed_bound(min(g.quadrants, HOST_FAST_MAX * TWO_OVER_PI)) + angle_input_bound(g, 1)
    if g.name == "train":
        per += U64
    A = abs_sum_bound(g)
    blocks = -(-g.count // (HOST_BLOCK * max(1, threads))) + 1
    depth = HOST_BLOCK // 8 + 3 + 2 * blocks + threads
    return abs(g.h) * (g.gain * g.count * per + (depth + 2) * U64 * A * (1.0 + 2.0 ** -20))
