"""True values of the 4/(1+x^2) Riemann kernels, what each series tile is DEFINED to evaluate,
bitwise models of the per-sample paths, and derived error bounds.

The sibling of trig_truth.py for the headline integrand (csrc/include/miint/integrands.hpp:
Pi4, Pi4Wide; csrc/kernels/riemann.hip: Pi4F32, Pi4F32Wide, Pi4F32Acc32, lane_sum,
partials_body; csrc/include/miint/wave_reduce.hpp). Pure Python, mpmath and numpy; no GPU, no
torch. Everything here is in units of f(x) = 1 / (1 + x^2): the kernels' partials are unscaled
sums of f, point_values and a launch's value carry the factor SCALE = 4 (a power of two:
exact), a value also h.

Three levels of reference, none of them a kernel:

truth       The kernel's fp64 a, h = (b - a) / n and rule offset are exact reals; sample i of a
            launch sits at x_i = a + (i_begin + i + off) h. f(x_i) in mpmath at >= 200 bits;
            sums by the closed form
                sum_{i<m} 1 / (1 + (x0 + i h)^2) = Im[psi(m + w) - psi(w)] / h,  w = (x0 - j) / h
            (1 / (1 + x^2) = Im 1 / (x - j); psi = digamma), at a working precision chosen
            from |w| (true_sum), so N = 1e10 costs what N = 10 does.
definition  A series tile does not evaluate the truth but an exactly stated function of ROUNDED
            inputs (its midpoint coordinate, for some paths its d_m = 1 + x_m^2 or h):
            defined_tile_sum. GPU against definition is a statement about the tile's arithmetic
            alone (dropped e^2 or e^3, running sums, the fold); definition against truth is
            host mathematics (test_pi4_truth_cpu.py).
model       The per-sample paths hold no approximate instruction whose result is not pinned
            (recip_narrow is tested bitwise IEEE; point() and the Wide tiles divide by the
            library), so exact rational arithmetic rounded once per operation reproduces them
            bit for bit: model_tile, model_point, model_partials (lane loop, DPP wave sum, LDS
            block step included).

Bounds. Every helper returns an ABSOLUTE bound in units of f and derives it in its docstring
from the operations of the code, with U64 = 2**-53 and U32 = 2**-24 the relative error of one
rounding. Nothing in them is taken from a kernel's output; they are worst-case sums of the
individual roundings. f > 0, so the sum of the absolute values of any partial sum's terms is
the sum itself, and relative bounds of the samples carry over to sums unchanged.
"""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction

import mpmath
import numpy as np

from .trig_truth import RULE_OFF, U32, U64

PREC = 200
MP = mpmath.MPContext()
MP.prec = 2 * PREC      # values; true_sum raises it with |w|

SCALE = 4.0             # Pi4::kScale
# tile lengths (asserted against the extension's riemann_tile_len in the GPU tests)
TILE64 = 384            # Pi4::kSeriesTile: series, series_exact
TILE64_LONG = 1536      # Pi4Long::kTile: series_exact where 768 |h| <= HALF_SPAN_H (LONG_PATH)
TILE32 = 192            # Pi4F32::kSubs * kSubLen: fp32 and fp32acc series
TILE_PER_SAMPLE = 32    # series_direct and every ieee tile
HALF_SPAN_H = 2.0e-6    # kernels.hpp series_ok / series_ok_f32 / direct_ok: (T / 2) |h| <= this
BLOCK = 256             # kRiemannBlock
WAVE = 64

# dispatcher limits (kernels.hpp, riemann.hip)
PI4_NARROW_MAX_X = 2.0 ** 249        # kPi4NarrowMaxX: fp64 ieee, recip_narrow below, Pi4Wide beyond
PI4_F32_NARROW_MAX_X = 2.0 ** 49     # kPi4F32NarrowMaxX: the same for fp32
PI4_SERIES_MAX_X = 2.0 ** 249        # kPi4SeriesMaxX: fp64 series tiles below
PI4_F32_SERIES_MAX_X = 2.0 ** 62     # kPi4SeriesMaxXF32: fp32 / fp32acc series tiles below

# v_rcp_f64 is documented at 2**29 ulp (2**-23 relative): |e_m| of a raw-rcp seed stays under
# 2**-22 with a factor two of room; v_rcp_f32 at 1 ulp (2**-23), one Newton step squares it
# and the step's own two roundings leave |e_m| <= 2**-24 (1 + 2**-20): under 2**-23.
EM_RAW64 = 2.0 ** -22
EM_NEWTON32 = 2.0 ** -23
SECOND_ORDER = 1.0 + 1.0e-5   # covers every product of two of the small terms below

PATHS = ("fp64-series_exact", "fp64-series", "fp64-series_direct", "fp64-ieee",
         "fp32-series", "fp32-ieee", "fp32acc-series", "fp32acc-ieee")
SERIES_PATHS = ("fp64-series_exact", "fp64-series", "fp64-series_direct", "fp32-series",
                "fp32acc-series")


# The long series_exact tile (integrands.hpp Pi4Long; kernels.hpp pi4_tile_long): a path name of
# its own here, the same division ("series_exact") on the device. Not in PATHS / SERIES_PATHS,
# which enumerate the cases of the tests written before it existed.
LONG_PATH = "fp64-series_exact-long"


def _series(path: str) -> bool:
    return path in SERIES_PATHS or path == LONG_PATH


def long_tile_admitted(h: float) -> bool:
    """kernels.hpp series_ok_long: 0 < 768 |h| <= 2e-6 (a degenerate interval keeps the short
    tile)."""
    return 0.0 < abs(h) and (TILE64_LONG // 2) * abs(h) <= HALF_SPAN_H


def tile_len(path: str) -> int:
    return {"fp64-series_exact": TILE64, "fp64-series": TILE64, "fp32-series": TILE32,
            "fp32acc-series": TILE32, LONG_PATH: TILE64_LONG}.get(path, TILE_PER_SAMPLE)


def seed_residual(path: str) -> float:
    """A cap on |e_m| = |1 - d_m s| of the seed a series path uses: the raw v_rcp_f64
    (seed_half, seed_exact: EM_RAW64), v_rcp_f64 and one Newton step (Pi4::seed: the step
    squares 2**-23 to 2**-46 and rounds s once, 2**-53: under 2**-45), v_rcp_f32 and one
    Newton step (EM_NEWTON32)."""
    return {"fp64-series_exact": EM_RAW64, "fp64-series": EM_RAW64, LONG_PATH: EM_RAW64,
            "fp64-series_direct": 2.0 ** -45}.get(path, EM_NEWTON32)


def _mpq(fr: Fraction):
    return MP.mpf(fr.numerator) / MP.mpf(fr.denominator)


# ---------------------------------------------------------------------------- geometry
@dataclasses.dataclass(frozen=True)
class Geometry:
    """The samples of one launch: x_i = a + (i_begin + i + off) h, i < count, exactly."""
    a: float
    h: float
    off: Fraction
    i_begin: int
    count: int

    def x(self, i) -> Fraction:
        """Sample i (i may be a Fraction: tile midpoints)."""
        return Fraction(self.a) + (self.i_begin + Fraction(i) + self.off) * Fraction(self.h)

    @property
    def x_abs_max(self) -> float:
        return float(max(abs(self.x(0)), abs(self.x(self.count - 1))))

    @property
    def x_abs_min(self) -> float:
        x0, x1 = self.x(0), self.x(self.count - 1)
        return 0.0 if (x0 <= 0 <= x1 or x1 <= 0 <= x0) else float(min(abs(x0), abs(x1)))


def geometry(spec, n: int, rule: str, i_begin: int = 0, count: int | None = None) -> Geometry:
    if spec.name != "pi4":
        raise ValueError("pi4_truth covers pi4")
    h = (spec.b - spec.a) / n          # as ops/kernels.py and RiemannPlan form it
    count = n if count is None else count
    if count < 1 or i_begin < 0:
        raise ValueError("need count >= 1 and i_begin >= 0")
    return Geometry(float(spec.a), h, RULE_OFF[rule], int(i_begin), int(count))


# ---------------------------------------------------------------------------- the truth
def f_true(x: Fraction):
    return 1 / (1 + _mpq(x) ** 2)


def true_values(g: Geometry):
    """(fp64 array, list of mpf): f at every sample, rounded to fp64 at the very end only."""
    exact = [f_true(g.x(i)) for i in range(g.count)]
    return np.array([float(v) for v in exact], dtype=np.float64), exact


def direct_sum(g: Geometry):
    """mpf: the sum sample by sample (the closed form's check; small counts)."""
    return MP.fsum(f_true(g.x(i)) for i in range(g.count))


def progression_sum(x0: Fraction, h: Fraction, m: int):
    """sum_{i<m} 1 / (1 + (x0 + i h)^2) by the digamma closed form. h < 0 is re-indexed from the
    other end (the same samples), h = 0 is m f(x0). The difference psi(m + w) - psi(w) loses
    about log2 |w| bits of its imaginary part twice over (Im psi(w) ~ arg w differs from
    Im psi(m + w) in its low bits when m << |w|, and the result is divided by h), so the
    working precision is 2 PREC + 3 log2(2 + |w| + m) bits: the CPU tests check the outcome
    against direct_sum to 2**-150 relative at every kind of case."""
    if h == 0:
        return m * f_true(x0)
    if h < 0:
        x0, h = x0 + (m - 1) * h, -h
    wr = x0 / h
    mag = abs(wr) + 1 / h + m + 2
    bits = 2 * PREC + 3 * (mag.numerator.bit_length() - mag.denominator.bit_length() + 2)
    with MP.workprec(max(MP.prec, bits)):
        hh = _mpq(h)
        w = MP.mpc(_mpq(wr), -1 / hh)
        return +((MP.digamma(m + w) - MP.digamma(w)).imag / hh)


def true_sum(g: Geometry):
    """mpf: sum of f over the launch's samples (unscaled: what the partials add up to)."""
    return progression_sum(g.x(0), Fraction(g.h), g.count)


def true_value(g: Geometry):
    """mpf: SCALE h sum, what a launch returns."""
    return MP.mpf(SCALE) * MP.mpf(g.h) * true_sum(g)


# ---------------------------------------------------------------------------- rounding
def rnd64(fr: Fraction) -> float:
    """fr rounded to the nearest double (ties to even); beyond the range, infinity."""
    try:
        return float(fr)          # int / int true division: correctly rounded
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


def rnd32(fr: Fraction) -> np.float32:
    """fr rounded ONCE to the nearest fp32 (ties to even, gradual underflow, overflow to
    infinity): np.float32(float(fr)) would round twice."""
    if fr == 0:
        return np.float32(0.0)
    sign, q = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = q.numerator.bit_length() - q.denominator.bit_length()     # 2**(e-1) < q < 2**(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                    # 2**e <= q < 2**(e+1)
    e = max(e, -126)
    scaled = q / Fraction(2) ** (e - 23)                          # ulp = 2**(e-23)
    n, r = divmod(scaled.numerator, scaled.denominator)
    if 2 * r > scaled.denominator or (2 * r == scaled.denominator and n & 1):
        n += 1
    v = math.ldexp(float(n), e - 23)                              # exact: n <= 2**24
    return np.float32(sign * v) if v < 2.0 ** 128 else np.float32(sign * math.inf)


def _fr(v) -> Fraction:
    return Fraction(float(v))


def fma64(a: float, b: float, c: float) -> float:
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c          # the model only meets +-inf here (never inf - inf)
    return rnd64(_fr(a) * _fr(b) + _fr(c))


def fma32(a, b, c) -> np.float32:
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return np.float32(a * b + c)
    return rnd32(_fr(a) * _fr(b) + _fr(c))


def recip64(d: float) -> float:
    """IEEE 1.0 / d (d >= 1, or +inf)."""
    return 0.0 if math.isinf(d) else rnd64(1 / _fr(d))


def recip32(d) -> np.float32:
    return np.float32(0.0) if math.isinf(float(d)) else rnd32(1 / _fr(d))


# ---------------------------------------------------------------------------- coordinates
def _pow2(v: float) -> bool:
    return v != 0.0 and math.frexp(abs(v))[0] == 0.5


def coords_exact(g: Geometry) -> bool:
    """True when every fp64 coordinate the kernels form for this launch is exact: h = +-2**-k,
    a a multiple of h / 2 (samples under any rule and the midpoints of even-length tiles sit on
    the grid h / 2), and |x| / (h / 2) < 2**53 at the farther end, a tile beyond it included.
    Then fma(index, h, a) and fma(u, h, x0) return their exact values."""
    if not _pow2(g.h):
        return False
    q = Fraction(abs(g.h)) / 2
    if (Fraction(g.a) / q).denominator != 1:
        return False
    far = max(abs(g.x(0)), abs(g.x(g.count - 1))) + 512 * Fraction(abs(g.h))
    return far / q < 2 ** 53


def base_index(g: Geometry) -> float:
    """lane_sum's `base`: double(i_begin) + off (exact: i_begin < 2**52)."""
    return float(g.i_begin) + float(g.off)


def tile_anchor(g: Geometry, path: str, tile: int = 0) -> float:
    """The fp64 coordinate lane_sum hands tile `tile` of the launch: fma(ib, h, a) with
    ib = base + tile * T + anchor, anchor = (T - 1) / 2 for the midpoint-anchored series tiles
    (Pi4::anchor, Pi4F32::anchor) and 0 otherwise. ib is an exact double (< 2**52 + T)."""
    T = tile_len(path)
    mid = path in ("fp64-series_exact", "fp64-series", "fp32-series", "fp32acc-series", LONG_PATH)
    ib = base_index(g) + float(tile * T) + (0.5 * (T - 1) if mid else 0.0)
    return fma64(ib, g.h, g.a)


def ulp32(v: float) -> float:
    a = max(abs(v), 2.0 ** -126)
    return 2.0 ** (math.frexp(a)[1] - 24)


def rel_slope(g: Geometry) -> float:
    """sup over the launch of |f'(x)| / f(x) |x|-free part: 2 |x| / (1 + x^2), which rises to 1
    at |x| = 1 and falls beyond: what a displacement dx costs, relative, is this times dx."""
    lo, hi = g.x_abs_min, g.x_abs_max
    if lo <= 1.0 <= hi:
        return 1.0
    x = hi if hi < 1.0 else lo
    return 2.0 * x / (1.0 + x * x) if x < 1e150 else 2.0 / x


def coord_rel(g: Geometry, roundings64: int, fp32: bool = False, exact: bool | None = None) -> float:
    """Relative error of f from the roundings of a sample's (or a tile midpoint's) coordinate:
    rel_slope times the displacement. Each fp64 fma that forms a coordinate rounds once,
    <= ulp(x) / 2 at the launch's farther end, `roundings64` of them; zero where coords_exact.
    fp32=True adds ONE fp32 rounding, ulp32(x) / 2: the conversion of the fp64 midpoint or
    anchor to fp32 (callers add what else their path rounds in fp32)."""
    exact = coords_exact(g) if exact is None else exact
    dx = 0.0 if exact else roundings64 * 0.5 * math.ulp(g.x_abs_max)
    if fp32:
        dx += 0.5 * ulp32(g.x_abs_max)
    return rel_slope(g) * dx * SECOND_ORDER


# ---------------------------------------------------------------------------- definitions
def _offsets(T: int):
    return [Fraction(2 * j + 1 - T, 2) for j in range(T)]      # -(T-1)/2 ... (T-1)/2


def defined_inputs(path: str, g: Geometry, tile: int = 0) -> dict:
    """The rounded inputs a series tile works from (g.count >= (tile + 1) T):
    xm   fp64 series / series_exact: fl64(fma(ib, h, a)), the midpoint lane_sum passes;
         fp32 / fp32acc: that, converted to fp32 (Pi4F32::tile_acc `xm`);
    h    fp64: h itself; fp32: fl32(h) (`hf`);
    dm   fp64 series: fl64(fma(xm, xm, 1)) (seed_half); fp32: fl32(fmaf(xm, xm, 1));
         series_exact: the exact 1 + xm^2 (seed_exact forms e_m from x_m itself).
    series_direct has no midpoint form: its inputs are the 32 rounded d_u (defined_tile_sum)."""
    xa = tile_anchor(g, path, tile)
    if path in ("fp32-series", "fp32acc-series"):
        xm = np.float32(xa)
        hf = np.float32(g.h)
        return {"xm": _fr(xm), "h": _fr(hf), "dm": _fr(fma32(xm, xm, np.float32(1.0)))}
    if path == "fp64-series":
        return {"xm": _fr(xa), "h": Fraction(g.h), "dm": _fr(fma64(xa, xa, 1.0))}
    if path in ("fp64-series_exact", LONG_PATH):
        return {"xm": _fr(xa), "h": Fraction(g.h), "dm": 1 + _fr(xa) ** 2}
    raise ValueError(path)


def defined_tile_sum(path: str, g: Geometry, tile: int = 0):
    """mpf: what tile `tile` of a launch of `path` is defined to sum.

    series_exact, series, fp32, fp32acc: sum over k = +-1/2 ... +-(T-1)/2 of
        1 / (dm + 2 xm h k + h^2 k^2)
    from defined_inputs (the exact quadratic in k the tiles expand their residuals from:
    e_k = e_m + k A + k^2 B is 1 - d_k s term by term). series_direct: sum over u < 32 of
    1 / d_u, d_u = fl64(fma(x_u, x_u, 1)), x_u = fl64(fma(u, h, x0)), x0 = fl64(fma(ib, h, a))
    (Pi4::tile: `series_direct rounds every coordinate`)."""
    T = tile_len(path)
    if path == "fp64-series_direct":
        x0 = tile_anchor(g, path, tile)
        tot = MP.mpf(0)
        for u in range(T):
            x = fma64(float(u), g.h, x0)
            tot += 1 / _mpq(_fr(fma64(x, x, 1.0)))
        return tot
    p = defined_inputs(path, g, tile)
    return MP.fsum(1 / _mpq(p["dm"] + 2 * p["xm"] * p["h"] * k + p["h"] ** 2 * k * k)
                   for k in _offsets(T))


# ---------------------------------------------------------------------------- bitwise models
def _per_sample_kind(path: str) -> str:
    if path.startswith("fp64"):
        return "fp64"
    return "fp32acc" if path.startswith("fp32acc") else "fp32"


def model_point(path: str, g: Geometry, i: int):
    """f.point of sample i of the launch, as lane_sum's remainder loop evaluates it:
    x = fma(base + i, h, a) (one rounding); fp64 (Pi4, Pi4Wide): 1.0 / fma(x, x, 1);
    fp32 (Pi4F32::point, inherited by the Wide and Acc32 functors): x to fp32, then
    1.0f / fmaf(x, x, 1.0f), widened. Returns a double (fp32: exactly an fp32 value)."""
    x = fma64(base_index(g) + float(i), g.h, g.a)
    if _per_sample_kind(path) == "fp64":
        return recip64(fma64(x, x, 1.0))
    with np.errstate(over="ignore"):
        xf = np.float32(x)      # beyond the fp32 range: infinity, as the device's conversion
    return float(recip32(fma32(xf, xf, np.float32(1.0))))


def model_tile(path: str, g: Geometry, tile: int = 0):
    """One 32-sample ieee tile, bit for bit.

    fp64 (Pi4::tile<U, kIeee>, Pi4Wide::tile): x = fma(u, h, x0), acc += 1 / fma(x, x, 1) in
    sample order from 0.0 (recip_narrow is bitwise the IEEE quotient for |x| < 2**249; Pi4Wide
    divides by the library). fp32 (Pi4F32::tile, Pi4F32Wide::tile): x0 and h to fp32,
    x = fmaf(u, hf, x0), the even samples summed in one fp32 chain and the odd ones in another
    (the two packed lanes; acc0 / acc1 of the Wide tile), widened and added in fp64. fp32acc
    (Pi4F32Acc32::tile_acc, kIeee branch): the same two chains, added in fp32.
    Returns the tile's value as the lane accumulator's type: a float (fp32acc: an fp32 value)."""
    if path.split("-")[1] != "ieee":
        raise ValueError("bitwise models exist for the per-sample (ieee) tiles")
    x0 = tile_anchor(g, path, tile)
    kind = _per_sample_kind(path)
    if kind == "fp64":
        acc = 0.0
        for u in range(TILE_PER_SAMPLE):
            x = fma64(float(u), g.h, x0)
            acc += recip64(fma64(x, x, 1.0))
        return acc
    lanes = [np.float32(0.0), np.float32(0.0)]
    with np.errstate(all="ignore"):
        x0f, hf, one = np.float32(x0), np.float32(g.h), np.float32(1.0)
        for u in range(TILE_PER_SAMPLE):
            x = fma32(np.float32(u), hf, x0f)
            lanes[u & 1] = np.float32(lanes[u & 1] + recip32(fma32(x, x, one)))
        if kind == "fp32":
            return float(lanes[0]) + float(lanes[1])
        return float(np.float32(lanes[0] + lanes[1]))


def _dpp_sum(v: list, add, steps: int) -> list:
    """wave_reduce.hpp row_sum / lanes_sum_small on a 64-lane list: quad_perm [1,0,3,2] and
    [2,3,0,1], row_half_mirror, row_mirror (every lane adds its partner's value)."""
    perms = (lambda i: i ^ 1, lambda i: i ^ 2, lambda i: (i & ~7) | (7 - (i & 7)),
             lambda i: (i & ~15) | (15 - (i & 15)))
    for p in perms[:steps]:
        v = [add(v[i], v[p(i)]) for i in range(len(v))]
    return v


def model_block_sum(lane_values: list, add=lambda a, b: a + b, zero=0.0):
    """block_sum_dyn of one workgroup's lane values (a multiple of 64 of them): per wave
    row_sum, then rows 1 and 3 += lane 15 / 47 (row_bcast:15), rows 2 and 3 += lane 31
    (row_bcast:31), the total in lane 63; the wave totals through LDS into lanes 0 .. nw - 1
    of wave 0 and lanes_sum_small there (2 steps for up to 4 waves, 4 beyond)."""
    nw = len(lane_values) // WAVE
    totals = []
    for w in range(nw):
        v = _dpp_sum(list(lane_values[w * WAVE:(w + 1) * WAVE]), add, 4)
        v = [add(v[i], v[(i // 16) * 16 - 1]) if (i // 16) in (1, 3) else v[i] for i in range(WAVE)]
        v = [add(v[i], v[31]) if i >= 32 else v[i] for i in range(WAVE)]
        totals.append(v[63])
    if nw == 1:
        return totals[0]
    r = totals + [zero] * (WAVE - nw)
    return _dpp_sum(r, add, 2 if nw <= 4 else 4)[0]


def model_partials(path: str, g: Geometry, grid: int, block: int = BLOCK) -> list:
    """The per-workgroup partials of a per-sample (ieee) launch, bit for bit: lane_sum's deal
    of tiles (lane g owns tiles g, g + L, ...; ntile = q L + rem, the first rem lanes one round
    more), its remainder loop (sample done + k to lane k, k += L), the accumulator's type
    (fp32 for fp32acc) and block_sum_dyn. Only lanes that own work are evaluated; the others
    hold zero. A launch of a SERIES path shorter than its tile runs the remainder loop alone
    (f.point per sample) and is modelled too; one with a full series tile is not."""
    T = tile_len(path)
    if g.count >= T and path.split("-")[1] != "ieee":
        raise ValueError("no bitwise model of a series tile")
    kind = _per_sample_kind(path)
    f32 = kind == "fp32acc"
    zero = np.float32(0.0) if f32 else 0.0
    add = (lambda a, b: np.float32(a + b)) if f32 else (lambda a, b: a + b)
    lanes = grid * block
    ntile = g.count // T
    done = ntile * T
    acc = [zero] * lanes
    for t in range(ntile):
        lane = t % lanes
        v = model_tile(path, g, t)
        acc[lane] = add(acc[lane], np.float32(v) if f32 else v)
    for k in range(g.count - done):
        lane = k % lanes
        v = model_point(path, g, done + k)
        acc[lane] = add(acc[lane], np.float32(v) if f32 else v)
    return [float(model_block_sum(acc[b * block:(b + 1) * block], add, zero)) for b in range(grid)]


# ---------------------------------------------------------------------------- bounds: per point
def underflow_floor(g: Geometry, fp32: bool) -> float:
    """What underflow can cost ONE sample, absolute, on top of the relative terms. Nothing while
    f = 1 / (1 + x^2) stays a normal number over the whole launch: |x| < 2**63 in fp32
    (f >= 2**-126), |x| < 2**511 in fp64. Beyond, the quotient is denormal (the library
    division keeps denormals): it rounds at half the smallest denormal, 2**-150 / 2**-1075;
    the bound takes one whole denormal step, 2**-149 / 2**-1074. From where d = 1 + x^2 can
    round to infinity the quotient is an exact 0 and the sample's own f is lost:
    f < 2**-128 (1 + 2**-23) once fl32(x)^2 >= 2**128 (1 - 2**-25), taken from |x| >= 1.8e19
    at 2**-127; in fp64 f < 2**-1023 from |x| >= 1.3e154 (2**512 = 1.34e154)."""
    x = g.x_abs_max
    if fp32:
        return 0.0 if x < 2.0 ** 63 else (2.0 ** -149 if x < 1.8e19 else 2.0 ** -127)
    return 0.0 if x < 2.0 ** 511 else (2.0 ** -1074 if x < 1.3e154 else 2.0 ** -1023)


def point_bound(path: str, g: Geometry, vals: np.ndarray, full_tile: bool = True) -> np.ndarray:
    """|point_values - f| per sample, fp64 paths (point_values_kernel; in units of f).

    Common: the sample's coordinate is x = fma(u, h, x0), x0 = fma(i, h, a): two roundings
    (coord_rel(g, 2)); a sample of a partial last tile (`full_tile` False) runs f.point at that
    same twice-rounded x (the ieee terms). The value is rounded once at the end: ulp(v) / 2.
    ieee (Pi4::recip_narrow(fma(x, x, 1)), bitwise IEEE): d rounds once (U64 relative), the
        quotient once.
    series_direct (Pi4::seed; e = fma(-fma(x, x, 1), s, 1); v = fma(s, e + e e, s)): d rounds
        (U64), e rounds (U64 |e|), e e and the sum round (2 U64 |e|), the series drops
        e^3 / (1 - e), |e| <= E = seed_residual + 16 |h| (1 + ..): the seed is formed at the
        rounded midpoint from the rounded d_m, but e is each sample's own exact residual
        against whatever s came out, so the seed's roundings cost nothing.
    series (series_point: s (3/4 + g^2), g = 1/2 + e): the midpoint x_m = fma((T-1)/2, h, x0)
        rounds twice like a sample (the offsets k h from it are exact in the quadratic);
        d_m = fl(fma(x_m, x_m, 1)) shifts every residual of the tile by U64 relative;
        centre_g, c = fma(pk2, B, eh) and g = fma(k, A', c) round at ulp(1/2) / 2 = 2**-54
        each and d(g^2) = 2 g dg ~ dg: 3 * 2**-54; fma(g, g, 3/4) rounds at a value near 1
        (2**-53); A = fl(fl(-2 h x_m) s) and B = fl(-fl(h h) s) carry 2 U64 each, times
        k <= 192 and k^2: 2 U64 (192 |h| + 192^2 h^2); the series drops e^3 / (1 - e) with
        E = EM_RAW64 + 192 |h| (1 + 192 |h|).
    series_exact (series_exact_point: fma(s, e + e_sq^2, s)): the midpoint's two roundings;
        e_m from the exact d_m: 1 - s is exact for s in [1/2, 2] (|x_m| <= 1) and rounds at
        2**-54 beyond; the two fma that finish e_m round at U64 of values below 2 EM_RAW64;
        e in fp64 (3 roundings at U64 E); the fp32 square and its inputs 2.2e-18 (the
        derivation above Pi4::tile_acc; 4 U32 E on e_sq, U32 on the square, the dropped pair
        curvature); e + sq rounds at U64 E; dropped e^3 / (1 - e).
    Far from the origin (|x| >= 2**511) 1 + x^2 nears overflow and the quotient the
    denormals: every bound adds underflow_floor."""
    div = path.split("-")[1]
    v = np.abs(np.asarray(vals, dtype=np.float64))
    half_ulp = 0.5 * np.array([math.ulp(t) for t in v]) + underflow_floor(g, False)
    if div == "ieee" or not full_tile:
        rel = coord_rel(g, 2) + U64
        return v * rel * SECOND_ORDER + half_ulp
    h = abs(g.h)
    if div == "series_direct":
        E = seed_residual(path) + 16.0 * h * (1.0 + 16.0 * h)
        rel = coord_rel(g, 2) + U64 + 3.0 * U64 * E + E ** 3 / (1.0 - E)
    elif div == "series":
        E = EM_RAW64 + 192.0 * h * (1.0 + 192.0 * h)
        rel = (coord_rel(g, 2) + U64 + 3.0 * 2.0 ** -54 + 2.0 ** -53
               + 2.0 * U64 * (192.0 * h + (192.0 * h) ** 2) + E ** 3 / (1.0 - E))
    elif div == "series_exact":
        E = EM_RAW64 + 192.0 * h * (1.0 + 192.0 * h)
        off_unit = 2.0 ** -54 if g.x_abs_max + 192.0 * h > 1.0 else 0.0
        rel = (coord_rel(g, 2) + off_unit + 4.0 * U64 * EM_RAW64 + 4.0 * U64 * E + 2.2e-18
               + E ** 3 / (1.0 - E))
    else:
        raise ValueError(path)
    return v * rel * SECOND_ORDER + half_ulp


def point32_bound(g: Geometry, v: float) -> float:
    """One fp32 sample (Pi4F32::point through an n_local = 1 launch) against the truth: the
    fp64 coordinate rounds once and its conversion to fp32 once (coord_rel(g, 1, fp32=True)),
    d = fmaf(x, x, 1) once (U32), the quotient once (ulp32(v) / 2). The bitwise model is the
    sharper statement; this one ties the model to the truth."""
    rel = coord_rel(g, 1, fp32=True) + U32
    return abs(v) * rel * SECOND_ORDER + 0.5 * ulp32(v) + underflow_floor(g, True)


# ---------------------------------------------------------------------------- bounds: tiles
def tile_defn_rel(path: str, g: Geometry) -> float:
    """RELATIVE bound of a single series tile's sum (grid = 1, n_local = T, acc = 0) against
    defined_tile_sum; multiply by the defined sum. Every sample's value is s (1 + e_k + ...)
    with s within E of 1 / d_k, so an absolute error de of a residual is a relative error
    de (1 + 2 E) of that sample, and of the sum of such samples.

    Identity: 1 / d_k = s (1 + e_k + e_k^2 + e_k^3 / (1 - e_k)) for ANY seed s with
    e_k = 1 - d_k s, |e_k| <= E = seed_residual + (T / 2) |h| (1 + (T / 2) |h|)
    (|2 x s| <= 1 + E, s <= 1 + E).

    fp32-series (Pi4F32::tile_acc, riemann.hip), u = U32, A = -2 hf xm s, B = -hf^2 s:
      e_m = fmaf(-dm, s, 1)                 one rounding of the exact value: u EM
      a, b                                   two roundings each: 2 u |A|, 2 u |B|
      in  = fma(c0, b, a)                   u (|A| + 80 |B|), and a's, b's errors
      ec  = fma(c0, in, em)                 u E; carries c0 <= 80 times in's error
      A'  = fma(2 c0, b, a)                 u (|A| + 160 |B|); carried times k <= 15.5
      cc  = fma(1/4 | 9/4, b, ec), then up to 7 steps fma(4 j + 6 | 10, b, cc): 8 u E
      e   = fma(+-k, A', cc)                u E
    with |A| <= |h| (1 + E), |B| <= h^2 (1 + E): per residual
      de <= u [EM + (2 * 96 + 80 + 15.5) |h| + (2 * 96^2 + 80^2 + 160 * 15.5) h^2 + 10 E].
      sums: four fp32 lanes (t.x, t.y, t1.x, t1.y) of 48 residuals each, 47 additions of at
      most u 48 E each; t += t1 (2 additions at 96 E) and t.x + t.y (192 E): in all
      u E (4 * 47 * 48 + 2 * 96 + 192) = 9408 u E, spread over 192 samples: 49 u E each.
      dropped e^2 / (1 - e): E^2 / (1 - E) per sample.
      fold (fp64): 192 + double(t) rounds at U64, the fma once more: 2 U64.
    At the largest admitted h (96 h = 2e-6): 1.7e-12 + 6.2e-12 + 4.5e-12 = 1.2e-11, an
    eightieth of the 1e-9 an eighth of the old fold bias would show as.

    fp32acc-series (Pi4F32Acc32::tile_acc): the same residuals and sums, but the fold is
    fmaf(s, 192 + (t.x + t.y), acc) in fp32: 192 + t rounds at ulp32(192) / 2 = 2**-17, i.e.
    U32 relative, and the product once more: 2 U32 = 1.2e-7 in place of 2 U64. That fold is
    what the code documents Pi4F32 as correcting (the -8e-9 bias of tiles left at U fl(1/d_m)):
    no derivation can put this path's bound under U32.

    fp64-series (Pi4::tile_acc kSeries), per sample as point_bound's series without the
    coordinate, the d_m and the final rounding terms (they belong to the definition or to the
    sum): 3 * 2**-54 + 2 U64 (192 |h| + (192 h)^2) + E^3 / (1 - E); sums: one chain
    t = fma(g, g, t) from 288 to 384, each step rounding at half an ulp of [256, 512), 2**-45:
    384 * 2**-45 absolute on a sum of 384: 2**-45 relative; fold fma(s, t, 0): U64.

    fp64-series_exact (Pi4::tile_acc kSeriesExact): s 384 + s (lin + sum e_sq^2):
      e_m (seed_exact)      2**-54 where |x| can pass 1 (1 - s inexact), 4 U64 EM_RAW64
      lin = fma(kSumK2, B, 384 e_m)   384 e_m rounds (U64 E), B carries 2 U64 (h^2 kSumK2 / 384
                            <= (192 h)^2 / 3 per sample), the fma rounds (U64 E)
      squares               2.2e-18 per sample (above Pi4::tile_acc); four fp32 lanes of 96
                            squares of at most E^2: 4 * 96 * 96 u E^2 / 384 per sample
      t = lin + (x + y)     2 U64 E
      fl(384 s) and the outer fma       2 U64
      dropped e^3 / (1 - e)
    about 2.3e-16 on [0, 1], 2.9e-16 beyond.

    fp64-series_exact-long (Pi4Long::tile_acc, T = 1536): s 1536 + s (lin + sum e_sq^2), the
    short tile's terms with the long tile's spans (E = seed_residual + 768 |h| (1 + 768 |h|)):
      e_m (seed_exact)      as above: 2**-54 where |x| can pass 1, 4 U64 EM_RAW64
      lin = fma(kSumK2, B, 1536 e_m)  1536 e_m rounds (U64 E), B carries 2 U64 (h^2 kSumK2 /
                            1536 <= (768 h)^2 / 3 per sample), the fma rounds (U64 E)
      squares               per sample 2 E |de| + U32 E^2 with |de| <= 5 U32 E (A, B, the base
                            e_m + 341.25 B, in, e_c, A', e: derivation above Pi4Long), and the
                            curvature the square leaves out, 2 E 651 h^2; four fp32 lanes of 384
                            squares of at most E^2: 4 * 384 * 384 U32 E^2 / 1536 per sample
      t = lin + (x + y)     2 U64 E
      fl(1536 s) and the outer fma    2 U64
      dropped e^3 / (1 - e)
    about 3.5e-16 at the largest admitted h on [0, 1] (the fp32 sums' worst case, 9.2e-17, is
    what it adds to the short tile's), 2.4e-16 at N = 1e9.

    fp64-series_direct (Pi4::tile kSeriesDirect, 32 samples): e = fma(-d, s, 1) rounds
    (U64 E); t1a, t1b: 16 additions each of at most U64 16 E, joined (U64 32 E); t2: 32 fma of
    at most U64 32 E^2; (t1a + t1b) + t2 (U64 32 E): per sample U64 E (1 + 16 + 1 + 1) and the
    squares'; fl(32 s) is exact (a power of two), the final fma rounds (U64); dropped
    e^3 / (1 - e)."""
    h = abs(g.h)
    T = tile_len(path)
    E = seed_residual(path) + (T / 2) * h * (1.0 + (T / 2) * h)
    if path in ("fp32-series", "fp32acc-series"):
        de = U32 * (EM_NEWTON32 + 287.5 * h + (2 * 9216 + 6400 + 2480) * h * h + 10.0 * E)
        sums = 49.0 * U32 * E
        fold = 2.0 * U64 if path == "fp32-series" else 2.0 * U32 + U64
        rel = (de + sums + E * E / (1.0 - E)) * (1.0 + 2.0 * E) + fold
    elif path == "fp64-series":
        rel = (3.0 * 2.0 ** -54 + 2.0 * U64 * (192.0 * h + (192.0 * h) ** 2)
               + E ** 3 / (1.0 - E)) * (1.0 + 2.0 * E) + 2.0 ** -45 + U64
    elif path == "fp64-series_exact":
        off_unit = 2.0 ** -54 if g.x_abs_max + 192.0 * h > 1.0 else 0.0
        rel = (off_unit + 4.0 * U64 * EM_RAW64 + 2.0 * U64 * E
               + 2.0 * U64 * (192.0 * h) ** 2 / 3.0 + 2.2e-18 + 96.0 * U32 * E * E
               + 2.0 * U64 * E + E ** 3 / (1.0 - E)) * (1.0 + 2.0 * E) + 2.0 * U64
    elif path == LONG_PATH:
        off_unit = 2.0 ** -54 if g.x_abs_max + 768.0 * h > 1.0 else 0.0
        squares = 2.0 * E * 5.0 * U32 * E + U32 * E * E + 2.0 * E * 651.0 * h * h
        rel = (off_unit + 4.0 * U64 * EM_RAW64 + 2.0 * U64 * E
               + 2.0 * U64 * (768.0 * h) ** 2 / 3.0 + squares + 384.0 * U32 * E * E
               + 2.0 * U64 * E + E ** 3 / (1.0 - E)) * (1.0 + 2.0 * E) + 2.0 * U64
    elif path == "fp64-series_direct":
        rel = (19.0 * U64 * E + 33.0 * U64 * E * E + E ** 3 / (1.0 - E)) * (1.0 + 2.0 * E) + U64
    else:
        raise ValueError(path)
    return rel * SECOND_ORDER


def defn_truth_rel(path: str, g: Geometry) -> float:
    """RELATIVE bound of defined_tile_sum against the tile's true sum: what the rounded inputs
    cost (host mathematics; checked on the CPU on every case).

    series_exact   the midpoint fma(ib, h, a) rounds once: coord_rel(g, 1).
    series         that, and d_m = fl(fma(x_m, x_m, 1)): U64 of d_m, which is at most
                   U64 (1 + E_h) of every d_k of the tile (d_k >= d_m (1 - E_h), E_h = (T/2)|h|).
    series_direct  x0 rounds once and every x_u once more (coord_rel(g, 2)); every d_u once (U64).
    fp32, fp32acc  the fp64 midpoint once, its conversion to fp32 once (coord_rel(g, 1,
                   fp32=True)); h to fp32 moves sample k by k |h| U32 <= 96 |h| U32 (times
                   rel_slope); d_m = fl32(fmaf(x_m, x_m, 1)): U32. Where the coordinates are
                   exact in fp32 too (`exact`-coordinate family: callers pass a geometry for
                   which float32(x_m) == x_m; see fp32_coords_exact) only the d_m term is left."""
    h = abs(g.h)
    if path in ("fp64-series_exact", LONG_PATH):
        rel = coord_rel(g, 1)
    elif path == "fp64-series":
        rel = coord_rel(g, 1) + U64 * (1.0 + 2.0 * 192.0 * h)
    elif path == "fp64-series_direct":
        rel = coord_rel(g, 2) + U64
    elif path in ("fp32-series", "fp32acc-series"):
        ex32 = fp32_coords_exact(g)
        rel = (coord_rel(g, 1, fp32=not ex32) + (0.0 if _pow2(g.h) else rel_slope(g) * 96.0 * h * U32)
               + U32 * (1.0 + 2.0 * 96.0 * h))
    else:
        raise ValueError(path)
    return rel * SECOND_ORDER


def fp32_coords_exact(g: Geometry) -> bool:
    """True when the midpoint of every 192-sample tile of the launch is an fp32 number and h is
    one: fp64-exact coordinates, h a power of two and both end tiles' midpoints unchanged by
    the conversion (the midpoints are an arithmetic progression of step 192 h on one fp32 grid
    when the farther end's is)."""
    if not (coords_exact(g) and _pow2(g.h)) or g.count < TILE32:
        return False
    last = g.count // TILE32 - 1
    for t in (0, last):
        xm = tile_anchor(g, "fp32-series", t)
        if float(np.float32(xm)) != xm:
            return False
    far = max(abs(tile_anchor(g, "fp32-series", 0)), abs(tile_anchor(g, "fp32-series", last)))
    return (Fraction(192) * Fraction(abs(g.h)) / Fraction(ulp32(far))).denominator == 1


def ieee_rel(path: str, g: Geometry, point: bool = False) -> float:
    """RELATIVE error of one per-sample value against the truth (ieee tiles and f.point).
    fp64: coordinate (tile: two roundings, point(): one), d once (U64), quotient once (U64).
    fp32: the fp64 anchor rounds (tile: once, as x0; point(): once), converts to fp32
    (ulp32 / 2) and the tile's fmaf(u, hf, x0) rounds again (ulp32 / 2); hf = fl32(h) moves
    sample u by at most 31 |h| U32; d and the quotient U32 each."""
    if path.startswith("fp64"):
        return (coord_rel(g, 1 if point else 2) + 2.0 * U64) * SECOND_ORDER
    dx = 0.0 if point else 0.5 * ulp32(g.x_abs_max) + 31.0 * abs(g.h) * U32
    return (coord_rel(g, 1, fp32=True) + rel_slope(g) * dx + 2.0 * U32) * SECOND_ORDER


def tile_truth_bound(path: str, g: Geometry, true_tile_sum: float) -> float:
    """ABSOLUTE bound of a single-tile launch's partial against the true sum of its samples.
    Series paths: tile_defn_rel + defn_truth_rel. ieee tiles (for completeness; the bitwise
    model is the sharper statement): ieee_rel per sample and the additions: fp64 32 in one
    chain (32 U64), fp32 two chains of 16 (16 U32) and one fp64 (U64) or fp32 (U32) join.
    Where f leaves the normal range every sample adds underflow_floor (sums of denormals are
    exact)."""
    S = abs(true_tile_sum)
    T = tile_len(path)
    if _series(path):
        rel = tile_defn_rel(path, g) + defn_truth_rel(path, g)
    elif path == "fp64-ieee":
        rel = ieee_rel(path, g) + 32.0 * U64
    else:
        rel = ieee_rel(path, g) + 16.0 * U32 + (U32 if path.startswith("fp32acc") else U64)
    return S * rel * SECOND_ORDER + T * underflow_floor(g, not path.startswith("fp64"))


# ---------------------------------------------------------------------------- bounds: launches
def launch_depth(count: int, tile: int, grid: int, block: int = BLOCK) -> int:
    """The longest chain of additions between one tile sum and the launch's result
    (riemann.hip lane_sum, wave_reduce.hpp block_sum_dyn, finalize / ordered_partials): a lane
    adds its ceil(tiles / lanes) tile sums and its share of the < T remainder samples; 6 DPP
    steps across the wave and up to 4 across the workgroup's waves; the finalize adds
    ceil(grid / block) partials per thread, then the same 10 steps."""
    lanes = grid * block
    tiles = count // tile
    rem = count - tiles * tile
    return (-(-tiles // lanes) + -(-rem // lanes)) + 10 + -(-grid // block) + 10


def launch_sum_bound(path: str, g: Geometry, true_total: float, grid: int, block: int = BLOCK) -> float:
    """ABSOLUTE bound of the sum of a launch's partials (or of its value divided by SCALE h)
    against true_sum: slices of several tiles and lanes, whole ranges and plan steps alike.

    Every full tile within its single-tile relative bound of its own true sum (series:
    tile_defn_rel + defn_truth_rel; ieee: ieee_rel and the in-tile additions), taken at the
    launch's worst coordinate (coord_rel uses the farther end's ulp and the sup of the slope);
    the < T remainder samples run f.point (ieee_rel(point=True)); f > 0, so these relative
    bounds apply to the total. Between tile and result launch_depth additions, each rounding
    at most U of the running sum, itself at most the total: depth U64 S; for fp32acc the lane
    accumulation, the wave's DPP steps and the LDS step are fp32 (Pi4F32Acc32: AccOf = float;
    the partials meet in fp64): the first ceil(tiles / lanes) + ceil(rem / lanes) + 10
    additions at U32, the finalize's at U64. The tile's fold into a non-zero accumulator
    (fma(s, t, acc), acc + tile) is one of those additions. Where f leaves the normal range
    every sample adds underflow_floor."""
    T = tile_len(path)
    S = abs(true_total)
    if _series(path):
        rel = tile_defn_rel(path, g) + defn_truth_rel(path, g)
    elif path == "fp64-ieee":
        rel = ieee_rel(path, g) + 32.0 * U64
    else:
        rel = ieee_rel(path, g) + 16.0 * U32 + (U32 if path.startswith("fp32acc") else U64)
    ipath = path.split("-")[0] + "-ieee"
    rel = max(rel, ieee_rel(ipath, g, point=True))
    depth = launch_depth(g.count, T, grid, block)
    if path.startswith("fp32acc"):
        fin = -(-grid // block) + 10
        acc = (depth - fin) * U32 + fin * U64
    else:
        acc = depth * U64
    return S * (rel + acc) * SECOND_ORDER + g.count * underflow_floor(g, not path.startswith("fp64"))


def launch_value_bound(path: str, g: Geometry, true_total: float, grid: int, block: int = BLOCK) -> float:
    """ABSOLUTE bound of a launch's VALUE, SCALE h sum, against true_value: launch_sum_bound
    times SCALE |h| (h SCALE is exact) and U64 of the value for the multiplication by it
    (finalize_kernel, fused_body, multistep_close_kernel: tot * scale). A plan step is such a
    launch at the plan's grid and block."""
    s = SCALE * abs(g.h)
    return s * (launch_sum_bound(path, g, true_total, grid, block) + U64 * abs(true_total))


# ---------------------------------------------------------------------------- host emulation
def emulate_f32_tile(path: str, g: Geometry, tile: int = 0, seed_rel: float = 0.0,
                     defect: str | None = None) -> float:
    """Pi4F32::tile_acc / Pi4F32Acc32::tile_acc (kSeries, acc = 0) operation by operation in
    exactly rounded fp32 (fma32), for the CPU tests: NOT a bitwise model, because the tile's
    seed comes from v_rcp_f32, whose result is not pinned; here the seed is the correctly
    rounded 1 / d_m times (1 + seed_rel), then the tile's own Newton step. The tile's value
    must not depend on the seed beyond its bound: the CPU tests perturb it.
    defect = "fold32": the fp32 tile's fold done in fp32 (what dropped e_m and biased every
    tile by up to 8e-9 once)."""
    f = np.float32
    one = f(1.0)
    xm, hf = f(tile_anchor(g, path, tile)), f(g.h)
    dm = fma32(xm, xm, one)
    s = rnd32(_fr(recip32(dm)) * (1 + Fraction(seed_rel)))
    s = fma32(s, fma32(-dm, s, one), s)
    em = fma32(-dm, s, one)
    a = rnd32(_fr(rnd32(_fr(f(-2.0) * hf) * _fr(xm))) * _fr(s))
    b = rnd32(-_fr(rnd32(_fr(hf) * _fr(hf))) * _fr(s))
    lanes = {"t.x": None, "t.y": None, "t1.x": None, "t1.y": None}

    def add(key, v):
        lanes[key] = v if lanes[key] is None else f(lanes[key] + v)

    for q in range(6):
        c0 = f((q - 2.5) * 32)
        ec = fma32(c0, fma32(c0, b, a), em)
        aq = fma32(f(c0 + c0), b, a)
        cc = [fma32(f(0.25), b, ec), fma32(f(2.25), b, ec)]
        for j in range(0, 16, 2):
            k0, k1 = f(j + 0.5), f(j + 1.5)
            add("t.x", fma32(k0, aq, cc[0]))
            add("t.y", fma32(-k0, aq, cc[0]))
            add("t1.x", fma32(k1, aq, cc[1]))
            add("t1.y", fma32(-k1, aq, cc[1]))
            if j + 2 < 16:
                cc = [fma32(f(4.0 * j + 6.0), b, cc[0]), fma32(f(4.0 * j + 10.0), b, cc[1])]
    tx, ty = f(lanes["t.x"] + lanes["t1.x"]), f(lanes["t.y"] + lanes["t1.y"])
    t = f(tx + ty)
    if path == "fp32acc-series" or defect == "fold32":
        return float(fma32(s, f(f(192.0) + t), f(0.0)))
    return fma64(float(s), 192.0 + float(t), 0.0)
