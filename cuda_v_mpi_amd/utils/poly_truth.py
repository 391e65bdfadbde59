"""True values of the polynomial Riemann kernels, what a Taylor-pair tile is DEFINED to
evaluate, operation-by-operation emulations of the four paths, and derived error bounds.

The sibling of trig_truth.py and pi4_truth.py for Integrand::kPoly
(csrc/include/miint/integrands.hpp: Poly<NC>; integrands_f32.hpp: PolyF32<NC>;
csrc/kernels/riemann.hip: prepared, lane_sum, point_values_kernel; kernels.hpp:
effective_div, poly_series_in_range). Pure Python: fractions, integers and numpy; no GPU, no
torch, and no working precision to choose: a, h = (b - a) / n, the rule offset and the
coefficients are doubles, i.e. dyadic rationals, so every sample x_i = a + (i_begin + i + off) h,
every p(x_i) and every sum of them is an exact rational.

truth       p(x_i) by Horner in Fractions (true_values, direct_sum), and the sum in closed form
            by power sums (true_sum):
                sum_{i<m} p(x0 + i h) = sum_j c_j sum_t C(j, t) x0^(j-t) h^t S_t(m),
            S_t(m) = sum_{i<m} i^t from the recurrence m^(t+1) = sum_{j<=t} C(t+1, j) S_j(m).
            Rounded to fp64 once, by the caller.
definition  A Taylor-pair tile (64 samples, two 32-sample sub-tiles) evaluates an exact function
            of ROUNDED inputs: cs_i = fl(c_i h^i) as riemann.hip prepared() forms them (long
            double products, rounded to double), inv_h = fl(1 / h), the tile midpoint x_m the
            kernel is handed, u_m = fl(x_m inv_h) and the centres u_c = fl(u_m -+ 16) (or the
            fused fl(x_m inv_h -+ 16): HIP contracts by default; both are allowed). From them:
            the exact Taylor shift b_m = sum_j C(j, m) cs_j u_c^(j-m), the even and odd parts
            E(k^2), O(k^2) and the samples E +- k O, k = 1/2 ... 31/2 (defined_tile). Its
            `defect` argument mutates the definition for the defect tests.
emulation   emulate_tile / emulate_horner run the kernels' operations one by one in exactly
            rounded fp64 / fp32 (no approximate instruction is involved: the paths are fma,
            add and conversions only). They check the bounds below on a CPU and look for fp32
            denormals; they are not what the GPU is compared with.

Bounds. ABSOLUTE, per sample (sample_bounds) and per launch (launch_sum_bound,
launch_value_bound), derived in the docstrings from the operations of the code, with
U64 = 2**-53 and U32 = 2**-24 the relative error of one rounding. Nothing in them comes from a
kernel's output. A polynomial has roots, so nothing is relative to |p|: the unit is
M(x) = sum_i |c_i| |x|^i, and for the tile-local operations L(k) = sum_m |b_m| k^m
(L(k) <= sum_j |cs_j| (|u_c| + k)^j = M(|x_c| + k |h|) <= M(|x| + 32 |h|) for a sample x of
the sub-tile: where the b_m are not at hand the bounds use that).
"""
from __future__ import annotations

import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np

from .trig_truth import RULE_OFF, U32, U64

TILE_SERIES = 64        # Poly::kSeriesTile
TILE_PER_SAMPLE = 32    # every ieee tile
SUB = 32                # Poly::kSub: samples per sub-tile, centres at -+16 steps of the midpoint
PAIRS = 16
BLOCK = 256             # kRiemannBlock
MAX_SERIES_COEFFS = 8   # kPolySeriesMaxCoeffs
MAX_COEFFS = 16         # kMaxPolyCoeffs
SECOND_ORDER = 1.0 + 1.0e-5     # every product of two small terms; float evaluation of M
MIN_NORMAL64 = 2.0 ** -1022
MIN_NORMAL32 = 2.0 ** -126

PATHS = ("fp64-series", "fp64-ieee", "fp32-series", "fp32-ieee")
REQUEST = {"fp64-series": ("fp64", "series"), "fp64-ieee": ("fp64", "ieee"),
           "fp32-series": ("fp32", "series"), "fp32-ieee": ("fp32", "ieee")}


# ---------------------------------------------------------------------------- geometry
@dataclasses.dataclass(frozen=True)
class Geometry:
    """The samples of one launch, x_i = a + (i_begin + i + off) h, i < count, exactly, and the
    polynomial's coefficients c_0 ... c_{ncoef-1}."""
    a: float
    h: float
    off: Fraction
    i_begin: int
    count: int
    coef: tuple

    def x(self, i) -> Fraction:
        return Fraction(self.a) + (self.i_begin + Fraction(i) + self.off) * Fraction(self.h)

    @property
    def ncoef(self) -> int:
        return len(self.coef)

    @property
    def x_abs_max(self) -> float:
        return float(max(abs(self.x(0)), abs(self.x(self.count - 1))))


def geometry(spec, n: int, rule: str, i_begin: int = 0, count: int | None = None) -> Geometry:
    if spec.name != "poly":
        raise ValueError("poly_truth covers poly")
    h = (spec.b - spec.a) / n          # as ops/kernels.py and RiemannPlan form it
    count = n if count is None else count
    if count < 1 or i_begin < 0 or not 1 <= len(spec.coef) <= MAX_COEFFS:
        raise ValueError("need count >= 1, i_begin >= 0 and 1..16 coefficients")
    return Geometry(float(spec.a), h, RULE_OFF[rule], int(i_begin), int(count),
                    tuple(float(c) for c in spec.coef))


# ---------------------------------------------------------------------------- the truth
def p_exact(coef, x: Fraction) -> Fraction:
    r = Fraction(0)
    for c in reversed(coef):
        r = r * x + Fraction(c)
    return r


def true_values(g: Geometry):
    """(fp64 array, list of Fraction): p at every sample, rounded at the very end only."""
    exact = [p_exact(g.coef, g.x(i)) for i in range(g.count)]
    return np.array([rnd64(v) for v in exact], dtype=np.float64), exact


def direct_sum(g: Geometry) -> Fraction:
    """The sum sample by sample (the closed form's check)."""
    return sum((p_exact(g.coef, g.x(i)) for i in range(g.count)), Fraction(0))


@functools.lru_cache(maxsize=None)
def power_sums(m: int, top: int) -> tuple:
    """S_t = sum_{i<m} i^t, t = 0 ... top, exact integers (0^0 = 1)."""
    s = []
    for t in range(top + 1):
        acc = m ** (t + 1) - sum(math.comb(t + 1, j) * s[j] for j in range(t))
        assert acc % (t + 1) == 0
        s.append(acc // (t + 1))
    return tuple(s)


def true_sum(g: Geometry) -> Fraction:
    """sum of p over the launch's samples (unscaled: what the partials add up to)."""
    x0, h = g.x(0), Fraction(g.h)
    s = power_sums(g.count, g.ncoef - 1)
    xp = [x0 ** e for e in range(g.ncoef)]
    hp = [h ** e for e in range(g.ncoef)]
    return sum((Fraction(c) * math.comb(j, t) * xp[j - t] * hp[t] * s[t]
                for j, c in enumerate(g.coef) for t in range(j + 1)), Fraction(0))


def true_value(g: Geometry) -> Fraction:
    """h sum: what a launch returns (Poly::kScale = 1)."""
    return Fraction(g.h) * true_sum(g)


# ---------------------------------------------------------------------------- rounding
def rnd64(fr: Fraction) -> float:
    """fr rounded to the nearest double (ties to even, gradual underflow); beyond the range,
    infinity."""
    try:
        return float(fr)          # int / int true division: correctly rounded
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


def _round_sig(fr: Fraction, bits: int, emin: int) -> Fraction:
    """fr rounded to `bits` significant bits (ties to even), exponents not below emin."""
    if fr == 0:
        return Fraction(0)
    q = abs(fr)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                     # 2**e <= q < 2**(e+1)
    e = max(e, emin)
    ulp = Fraction(2) ** (e - bits + 1)
    n, r = divmod(q / ulp, 1)
    if 2 * r > 1 or (2 * r == 1 and n % 2):
        n += 1
    v = n * ulp
    return v if fr > 0 else -v


def rnd_ld(fr: Fraction) -> Fraction:
    """x87 long double: 64 significant bits (its exponent range is never reached here)."""
    return _round_sig(fr, 64, -16382)


def rnd32(fr: Fraction) -> float:
    """fr rounded ONCE to the nearest fp32 (ties to even, gradual underflow, overflow to
    infinity), returned as a Python float holding that fp32 value."""
    v = _round_sig(fr, 24, -126)
    if abs(v) >= Fraction(2) ** 128:
        return math.inf if v > 0 else -math.inf
    return float(v)


def _fr(v) -> Fraction:
    return Fraction(float(v))


def fma64(a: float, b: float, c: float) -> float:
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c          # 0 * inf is NaN here as on the device
    return rnd64(_fr(a) * _fr(b) + _fr(c))


def ulp32(v: float) -> float:
    return 2.0 ** (math.frexp(max(abs(v), MIN_NORMAL32))[1] - 24)


class F32:
    """Exactly rounded fp32 operations on Python floats that hold fp32 values; `denormal` turns
    True when any result is a non-zero denormal (whether the packed instructions flush those
    is not something the tests may depend on)."""

    def __init__(self):
        self.denormal = False

    def rnd(self, fr: Fraction) -> float:
        v = rnd32(fr)
        if v != 0.0 and abs(v) < MIN_NORMAL32:
            self.denormal = True
        if v == 0.0 and fr != 0:
            self.denormal = True          # underflowed to zero
        return v

    def fma(self, a, b, c) -> float:
        return self.rnd(_fr(a) * _fr(b) + _fr(c))

    def add(self, a, b) -> float:
        return self.rnd(_fr(a) + _fr(b))


# ---------------------------------------------------------------------------- dispatch mirror
def bucket(ncoef: int, series: bool) -> int:
    """riemann.hip dispatch: the coefficient bucket (zero-padded at the top). Series 4, 6, 7, 8;
    Horner 4, 8, 16."""
    if series:
        if ncoef > MAX_SERIES_COEFFS:
            raise ValueError("no series bucket beyond 8 coefficients")
        return 4 if ncoef <= 4 else 6 if ncoef <= 6 else ncoef
    return 4 if ncoef <= 4 else 8 if ncoef <= 8 else 16


def top_indices(nc: int) -> tuple:
    """Poly<NC>::parts: the top even and odd index of the bucket."""
    return (nc - 1) & ~1, (nc - 2) | 1


def prepared_cs(g: Geometry) -> list:
    """riemann.hip prepared(): cs_i = double((long double) c_i * hp), hp = h^i by repeated long
    double products."""
    out, hp = [], Fraction(1)
    for c in g.coef:
        out.append(rnd64(rnd_ld(Fraction(c) * hp)))
        hp = rnd_ld(hp * Fraction(g.h))
    return out


def inv_h(g: Geometry) -> float:
    if g.h == 0.0:
        return math.inf
    return rnd64(1 / Fraction(g.h))


def series_in_range(g: Geometry) -> bool:
    """kernels.hpp poly_series_in_range: h and 1 / h finite and non-zero, every non-zero c_i
    with a normal c_i h^i."""
    if not math.isfinite(g.h) or g.h == 0.0 or not math.isfinite(inv_h(g)):
        return False
    return all(c == 0.0 or (math.isfinite(cs) and abs(cs) >= MIN_NORMAL64)
               for c, cs in zip(g.coef, prepared_cs(g)))


def effective_path(dtype: str, div: str, g: Geometry) -> str:
    """kernels.hpp effective_div(params, div, dtype) for the polynomial: a series request
    (fp64: series, series_exact; fp32: anything but ieee) runs the Taylor-pair tiles for 1..8
    coefficients inside poly_series_in_range, Horner per sample otherwise."""
    asks = div in ("series", "series_exact") if dtype == "fp64" else div != "ieee"
    ser = asks and 1 <= g.ncoef <= MAX_SERIES_COEFFS and series_in_range(g)
    return f"{dtype}-{'series' if ser else 'ieee'}"


def tile_len(path: str) -> int:
    return TILE_SERIES if path.endswith("series") else TILE_PER_SAMPLE


def base_index(g: Geometry) -> float:
    """lane_sum's `base`: double(i_begin) + off (exact: i_begin < 2**52)."""
    return float(g.i_begin) + float(g.off)


def tile_midpoint(g: Geometry, tile: int, points: bool = False) -> float:
    """The fp64 midpoint a series tile is handed. lane_sum: fma(base + 64 tile + 31.5, h, a),
    one rounding; point_values_kernel: fma(31.5, h, fma(base + 64 tile, h, a)), two."""
    if points:
        return fma64(31.5, g.h, fma64(base_index(g) + 64.0 * tile, g.h, g.a))
    return fma64(base_index(g) + 64.0 * tile + 31.5, g.h, g.a)


# ---------------------------------------------------------------------------- the definition
def centre(g: Geometry, tile: int, q: int, fused: bool, points: bool = False,
           sign_flip: bool = False, shift_steps: int = 0) -> float:
    """u_c of sub-tile q (0: -16, 1: +16 steps from the midpoint), either rounding."""
    xm, ih = tile_midpoint(g, tile, points), inv_h(g)
    s = (-16.0 if q == 0 else 16.0) * (-1.0 if sign_flip else 1.0) + shift_steps
    if fused:
        return fma64(xm, ih, s)
    return rnd64(_fr(rnd64(_fr(xm) * _fr(ih))) + _fr(s))


def exact_shift(cs, uc: Fraction, nc: int, skip_row: int | None = None) -> list:
    """Poly::shift in exact arithmetic: NC - 1 passes of Horner, pass m leaving b_m final.
    Without skip_row the result is b_m = sum_j C(j, m) cs_j uc^(j-m)."""
    b = [Fraction(c) for c in cs] + [Fraction(0)] * (nc - len(cs))
    for m in range(nc - 1):
        if m == skip_row:
            continue
        for i in range(nc - 2, m - 1, -1):
            b[i] = b[i + 1] * uc + b[i]
    return b


def _parts(b, K, ev: int, od: int, mul):
    E = b[ev]
    for e in range(ev - 2, -1, -2):
        E = mul(E, K, b[e])
    O = b[od]
    for o in range(od - 2, 0, -2):
        O = mul(O, K, b[o])
    return E, O


def sample_slot(u: int) -> tuple:
    """Sample u of a tile: (sub-tile, pair index j, sign) with k = j + 1/2 (series_point)."""
    q, w = divmod(u, SUB)
    return (q, w - SUB // 2, 1) if w >= SUB // 2 else (q, SUB // 2 - 1 - w, -1)


def defined_tile(g: Geometry, tile: int = 0, fused: bool = False, points: bool = False,
                 defect: tuple | None = None):
    """(values, local): the 64 samples tile `tile` of a series launch is defined to evaluate, in
    sample order, as Fractions, and L(k) = sum_m |b_m| k^m per sample (floats).

    defect mutates the definition (the defect tests; None is the definition):
      ("ev", d) / ("od", d)   the top even / odd index moved by d (d = -2: a term dropped)
      ("drop_b", m)           b_m read as zero
      ("skip_row", m)         pass m of the shift skipped
      ("centre_sign", q)      sub-tile q's centre at +-16 with the wrong sign
      ("centre_step",)        both centres one step off
      ("both_plus",)          the -k sample taken at +k
    """
    kind = defect[0] if defect else None
    nc = bucket(g.ncoef, True)
    ev, od = top_indices(nc)
    if kind == "ev":
        ev += defect[1]
    if kind == "od":
        od += defect[1]
    if not (0 <= ev < nc and 1 <= od < nc):
        raise ValueError("mutated index leaves the bucket")
    cs = prepared_cs(g)
    bs = []
    for q in range(2):
        uc = centre(g, tile, q, fused, points, sign_flip=(kind == "centre_sign" and defect[1] == q),
                    shift_steps=1 if kind == "centre_step" else 0)
        b = exact_shift(cs, _fr(uc), nc, defect[1] if kind == "skip_row" else None)
        if kind == "drop_b" and defect[1] < nc:
            b[defect[1]] = Fraction(0)
        bs.append(b)
    vals, local = [], []
    for u in range(TILE_SERIES):
        q, j, sgn = sample_slot(u)
        k = Fraction(2 * j + 1, 2)
        E, O = _parts(bs[q], k * k, ev, od, lambda r, K, c: r * K + c)
        vals.append(E + k * O if (sgn > 0 or kind == "both_plus") else E - k * O)
        local.append(float(sum(abs(bm) * k ** m for m, bm in enumerate(bs[q]))))
    return vals, np.array(local)


def horner_exact(g: Geometry, i: int, drop_top: bool = False) -> Fraction:
    """What Horner per sample is defined to evaluate at sample i; drop_top is the defect of a
    bucket that loses its top coefficient (c[NC - 1] of an NC-wide bucket that is full)."""
    coef = list(g.coef)
    if drop_top:
        if len(coef) != bucket(len(coef), False):
            raise ValueError("the bucket's top coefficient is a padding zero here")
        coef[-1] = 0.0
    return p_exact(coef, g.x(i))


# ---------------------------------------------------------------------------- emulation
def emulate_tile(path: str, g: Geometry, tile: int = 0, fused: bool = False, points: bool = False,
                 defect: tuple | None = None):
    """Poly<NC>::tile_acc / PolyF32<NC>::tile_acc (kSeries, acc = 0) operation by operation.

    fp64-series: shift by fma, parts by fma, t += fma(k, O, E); t += fma(-k, O, E) in pair
    order. Returns (t, the 64 values in SAMPLE order, False).
    fp32-series: the shift in fp64, every b_m rounded once to fp32, two pairs (j, j + 1) per
    packed Horner, a += pk_fma(k, O, E); a += pk_fma(-k, O, E) on the two fp32 lanes of `a`,
    t += double(a.x) + double(a.y) per sub-tile. Returns (t, None, denormal seen).
    defect ("no_f32", m): bf[m] is left out of the conversion loop and stays zero."""
    nc = bucket(g.ncoef, True)
    ev, od = top_indices(nc)
    cs = prepared_cs(g) + [0.0] * (nc - g.ncoef)
    f32 = path == "fp32-series"
    F = F32()
    t, vals = 0.0, [None] * TILE_SERIES
    for q in range(2):
        uc = centre(g, tile, q, fused, points)
        b = list(cs)
        for m in range(nc - 1):
            for i in range(nc - 2, m - 1, -1):
                b[i] = fma64(b[i + 1], uc, b[i])
        if not f32:
            for j in range(PAIRS):
                k = j + 0.5
                E, O = _parts(b, k * k, ev, od, fma64)
                vp, vm = fma64(k, O, E), fma64(-k, O, E)
                t = (t + vp) + vm
                vals[q * SUB + SUB // 2 + j], vals[q * SUB + SUB // 2 - 1 - j] = vp, vm
            continue
        bf = [F.rnd(_fr(v)) for v in b]
        if defect and defect[0] == "no_f32" and defect[1] < nc:
            bf[defect[1]] = 0.0
        a = [0.0, 0.0]
        for j in range(0, PAIRS, 2):
            for lane in range(2):
                k = j + lane + 0.5
                E, O = _parts(bf, k * k, ev, od, F.fma)
                a[lane] = F.add(a[lane], F.fma(k, O, E))
                a[lane] = F.add(a[lane], F.fma(-k, O, E))
        t = t + (a[0] + a[1])
    return t, vals, F.denormal


def emulate_horner(path: str, g: Geometry, i: int, roundings: int = 1):
    """(value, denormal seen): f.point / one sample of an ieee tile at sample i. The coordinate
    is fma(base + i, h, a) (roundings = 1: the remainder loop) or fma(u, h, fma(base + i - u,
    h, a)) with u = i mod 32 (roundings = 2: a tile); fp32 converts it and the coefficients to
    fp32 and runs fmaf."""
    if roundings == 1:
        x = fma64(base_index(g) + float(i), g.h, g.a)
    else:
        u = i % TILE_PER_SAMPLE
        x = fma64(float(u), g.h, fma64(base_index(g) + float(i - u), g.h, g.a))
    if path.startswith("fp64"):
        r = g.coef[-1]
        for c in reversed(g.coef[:-1]):
            r = fma64(r, x, c)
        return r, False
    F = F32()
    xf = F.rnd(_fr(x))
    cf = [F.rnd(_fr(c)) for c in g.coef]
    r = cf[-1]
    for c in reversed(cf[:-1]):
        r = F.fma(r, xf, c)
    return r, F.denormal


# ---------------------------------------------------------------------------- bounds
def _sample_abs_x(g: Geometry) -> np.ndarray:
    idx = np.arange(g.count, dtype=np.float64) + (float(g.i_begin) + float(g.off))
    return np.abs(g.a + idx * g.h)


def mag(coef, x_abs) -> np.ndarray:
    """M(x) = sum_i |c_i| |x|^i, in floats (SECOND_ORDER covers the evaluation)."""
    x = np.asarray(x_abs, dtype=np.float64)
    r = np.zeros_like(x)
    for c in reversed(coef):
        r = r * x + abs(c)
    return r * SECOND_ORDER


def dmag(coef, x_abs) -> np.ndarray:
    """sum_i i |c_i| |x|^(i-1) >= |p'| on [-|x|, |x|]."""
    x = np.asarray(x_abs, dtype=np.float64)
    r = np.zeros_like(x)
    for i in range(len(coef) - 1, 0, -1):
        r = r * x + i * abs(coef[i])
    return r * SECOND_ORDER


def series_displacement(g: Geometry, xm_roundings: int) -> float:
    """How far, as a coordinate, a series tile's samples can sit from their places: the
    definition evaluates at (u_c + k) h, the truth at x_c + k h, so the distance is
    |h| |u_c - x_c / h|:
      x_m                  fma(ib, h, a) rounds once (a launch), the point kernel's
                           fma(31.5, h, x0) once more: xm_roundings ulp(x) / 2;
      inv_h = fl(1 / h)    relative U64 of u_m: |u_m| U64 steps (IEEE division: no fast-math);
      u_m = fl(x_m inv_h)  ulp(u_m) / 2 steps (absent when the compiler fuses; kept);
      u_c = fl(u_m -+ 16)  ulp(|u_m| + 16) / 2 steps.
    Near the origin every term is about U64 |x|. In the far regime |x / h| >= 2**53 the last
    two are its own term: u_m -+ 16 is absorbed in part, ulp(u_m) >= 2, and the tile's samples
    sit up to ulp(u_m) / 2 steps (and as much again) from their places."""
    x = g.x_abs_max + 64.0 * abs(g.h)
    um = x / abs(g.h) * (1.0 + 2.0 ** -50)
    steps = um * U64 + 0.5 * math.ulp(um) + 0.5 * math.ulp(um + 16.0)
    return (xm_roundings * 0.5 * math.ulp(x) + abs(g.h) * steps) * SECOND_ORDER


def underflow_floor(path: str, g: Geometry, x_abs) -> np.ndarray:
    """What underflow can cost one Horner sample, absolute. Zero while every |c_i x^i| term
    and partial result of the launch stays normal, which the accuracy lists guarantee (the CPU
    tests check it in the emulation); the underflow list needs it. Each of the ncoef - 1 fma
    results can lose 2**-1074 (fp64, gradual) or be flushed from below 2**-126 (fp32, and so can
    each coefficient's conversion: twice the sum), and the later steps multiply that by |x|^k;
    an fp32 coordinate below 2**-126 can be flushed whole: |p'| |x|."""
    x = np.asarray(x_abs, dtype=np.float64)
    geo = np.zeros_like(x)
    for _ in range(g.ncoef):
        geo = geo * x + 1.0
    if path.startswith("fp64"):
        return 2.0 ** -1074 * geo
    return 2.0 * MIN_NORMAL32 * geo + dmag(g.coef, x) * np.where(x < MIN_NORMAL32, x, 0.0)


def sample_bounds(path: str, g: Geometry, points: bool = False, local=None,
                  floor: bool = False) -> np.ndarray:
    """|computed - p(x_i)| for every sample of the launch: the samples of the launch's full
    tiles by the path's tile, the rest by f.point (lane_sum's remainder loop; in the point
    kernel a partial tile). `points`: the coordinates of point_values_kernel, which rounds
    once more than a launch (x0 = fma(i, h, a), then fma(u, h, x0)). `local`: L(k) of the full
    tiles' samples where the caller has it (defined_tile), else M(|x| + 32 |h|).

    fp64 Horner (Poly::point; tile: the same at x = fma(u, h, x0)):
      coordinate   1 rounding (point(), launch) or 2 (tile; point kernel): |p'| ulp(x) / 2 each;
      Horner       r = fma(r, x, c_k): the term c_i x^i passes at most ncoef - 1 roundings:
                   (ncoef - 1) U64 M(x).
    fp64 series (Poly::tile_acc kSeries, series_point), against the truth:
      inputs       series_displacement times |p'|; cs_i = fl(c_i h^i) twice rounded (64 bits,
                   then 53): U64 (1 + 2**-9) M;
      shift        (NC - 1) NC / 2 fma; the term C(j, m) cs_j u_c^(j-m) of b_m passes j - m
                   multiplying fma and at most m + 1 more of index m: at most NC roundings:
                   NC U64 sum_m sum_j C(j, m) |cs_j| |u_c|^(j-m) k^m = NC U64 M(|x_c| + k |h|);
      parts        E and O by fma in K = k^2 (k^2 is exact): ev / 2 and (od - 1) / 2 roundings
                   of partial sums of sum |b_m| k^m: max(ev / 2, (od - 1) / 2) U64 L(k);
      final        fma(+-k, O, E): U64 L(k).
    fp32 series (PolyF32::tile_acc): inputs and shift as fp64 (the shift is fp64); each b_m
      rounded once to fp32: U32 L(k); parts and final as above in U32.
    fp32 Horner (PolyF32::pointf): each c_i rounded to fp32: U32 M; the fp64 coordinate as
      above, then its conversion: |p'| ulp32(x) / 2; Horner (ncoef - 1) U32 M."""
    T = tile_len(path)
    full = (g.count // T) * T
    x = _sample_abs_x(g)
    fp32 = path.startswith("fp32")
    u = U32 if fp32 else U64
    xmax = g.x_abs_max
    out = np.empty(g.count)
    # Horner: everything on an ieee path, the remainder on a series path
    rounds = np.full(g.count, 2.0 if points else 1.0)
    if not path.endswith("series"):
        rounds[:full] = 2.0
    dx = rounds * 0.5 * math.ulp(xmax) + (0.5 * ulp32(xmax) if fp32 else 0.0)
    M, D = mag(g.coef, x), dmag(g.coef, x)
    out[:] = D * dx + ((g.ncoef - 1) + (1 if fp32 else 0)) * u * M
    if floor:
        out += underflow_floor(path, g, x)
    if path.endswith("series") and full:
        nc = bucket(g.ncoef, True)
        ev, od = top_indices(nc)
        xp = x[:full] + 32.0 * abs(g.h)
        Mp, Dp = mag(g.coef, xp), dmag(g.coef, xp)
        L = Mp if local is None else np.asarray(local)[:full] * SECOND_ORDER
        inputs = Dp * series_displacement(g, 2 if points else 1) + U64 * (1 + 2.0 ** -9) * Mp
        shift = nc * U64 * Mp
        tile_local = (max(ev // 2, (od - 1) // 2) + 1 + (1 if fp32 else 0)) * u * L
        out[:full] = inputs + shift + tile_local
    return out * SECOND_ORDER


def launch_depth(count: int, tile: int, grid: int, block: int = BLOCK) -> int:
    """The longest chain of fp64 additions between one tile sum and the launch's result
    (riemann.hip lane_sum, wave_reduce.hpp block_sum_dyn, finalize / ordered_partials): a lane
    adds its ceil(tiles / lanes) tile sums and its share of the remainder samples; 6 DPP steps
    across the wave and up to 4 across the workgroup's waves; the finalize adds
    ceil(grid / block) partials per thread, then the same 10 steps."""
    lanes = grid * block
    tiles = count // tile
    rem = count - tiles * tile
    return (-(-tiles // lanes) + -(-rem // lanes)) + 10 + -(-grid // block) + 10


def launch_sum_bound(path: str, g: Geometry, grid: int, block: int = BLOCK,
                     floor: bool = False) -> float:
    """ABSOLUTE bound of the sum of a launch's partials against true_sum: sample_bounds summed,
    and the additions, every one rounding at most U of a partial sum of |values| <= S =
    sum_i M(x_i) (1 + ..):
      fp64 series   the 64-term running sum t (t += v twice per pair): 63 U64;
      fp64 Horner   acc += point over the tile's 32 samples: 31 U64;
      fp32 series   16 fp32 additions into each lane of `a` per sub-tile: 16 U32; the fold
                    double(a.x) + double(a.y) and t += fold: 2 U64;
      fp32 Horner   two fp32 accumulators of 16 samples each: 16 U32; their fp64 join: U64;
      all           launch_depth further fp64 additions (acc + t, the lanes, the partials)."""
    T = tile_len(path)
    S = float(np.sum(mag(g.coef, _sample_abs_x(g))))
    if path.startswith("fp32"):
        adds = 16.0 * U32 + 2.0 * U64
    else:
        adds = (T - 1) * U64
    adds += launch_depth(g.count, T, grid, block) * U64
    under = 0.0
    if floor:   # every addition may lose a denormal step (fp64) or flush a denormal sum (fp32)
        under = g.count * (MIN_NORMAL32 if path.startswith("fp32") else 2.0 ** -1074)
    return (float(np.sum(sample_bounds(path, g, floor=floor))) + adds * S + under) * SECOND_ORDER


def launch_value_bound(path: str, g: Geometry, grid: int, block: int = BLOCK) -> float:
    """ABSOLUTE bound of a launch's VALUE, h sum, against true_value: launch_sum_bound times
    |h| (scale = h * 1.0 is exact) and U64 of the value for the multiplication (finalize_kernel,
    fused_body, the multi-step close: tot * scale). A plan step is such a launch at the plan's
    grid and block."""
    S = float(np.sum(mag(g.coef, _sample_abs_x(g))))
    return abs(g.h) * (launch_sum_bound(path, g, grid, block) + U64 * S) * SECOND_ORDER


def launch_magnitude(g: Geometry) -> float:
    """sum_i M(x_i): the size a launch's bound is held against (never |p|: it has roots)."""
    return float(np.sum(mag(g.coef, _sample_abs_x(g))))
