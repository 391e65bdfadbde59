"""Cases of the infinite-range tests (test_expr_adaptive_inf_cpu.py, test_expr_adaptive_inf_gpu.py):
each integrand as the C++ expression the device compiles, as the numpy function the model
evaluates, its range, its integral in closed form and the conditioning integral of the bound,
both evaluated with mpmath.

The value's bound. A converged run on an infinite range is held to

    |value - truth| <= max(tol, err_est) + (S + 2) * 2^-52 * resabs + 3 u C,    u = 2^-53

S is the finite rule's slack for the order of its sums (96 for ExprAdaptive, 48 for a sweep's
row; test_expr_adaptive_gpu.py and test_expr_adaptive_sweep_gpu.py derive them). The map
(miint/expr.hpp) adds, per node:
  * the division by t * t: the product rounds once and the quotient once, and for (-inf, inf)
    the sum f(q) + f(-q) once more: at most 3 u relative to |g|, which is in the units of resabs
    (the rule's integral of |g|): 1.5 * 2^-52, taken as 2;
  * the abscissa: q = (1.0 - t) / t is two operations and x = end +- q a third, so the device
    evaluates f at x + dx with |dx| <= 2 u |x - end| + u |x|; the bound charges each of the
    three operations one half-ulp u of the whole |x - end| + |x|: |dx| <= 3 u (|x - end| + |x|).
    To first order the value moves by the integral of |f'(x)| |dx| over x (dt / t^2 is dx), at most
        3 u C,   C = integral of (|x - end| + |x|) |f'(x)| dx   (end = 0 for (-inf, inf)).
    This is the integrand's own conditioning, not rounding of the sums, and does not come out
    of resabs. C is computed here with mpmath from the closed form of f'.
Nothing in the bound is tuned to a measured error; the tests print measured / bound."""
from __future__ import annotations

import functools
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 60
U = 2.0 ** -52
INF = float("inf")
MAP_UNITS = 2.0          # the division by t * t and the pair sum, in units of U * resabs
ABSCISSA_HALF_ULPS = 3   # (1.0 - t), / t, end +- q

RTOLS = [1e-6, 1e-10]
FEW_PANELS = 16
PANELS = 4096
MAX_INTERVALS = 1 << 16


def _m(x):
    return mp.mpf(x)


class Case:
    """f on the range between a and b (one or both infinite). ``df`` is f' in mpmath and
    ``points`` the breakpoints mpmath's quadrature needs to see the integrand's features."""

    def __init__(self, name, expr, f, a, b, truth, df, points):
        self.name, self.expr, self.f, self.a, self.b = name, expr, f, a, b
        self._truth, self.df, self.points = truth, df, points

    @functools.cached_property
    def truth(self) -> float:
        return float(self._truth())

    @functools.cached_property
    def conditioning(self) -> float:
        """C of the module docstring."""
        end = 0.0 if math.isinf(self.a) and math.isinf(self.b) else (
            self.b if math.isinf(self.a) else self.a)
        lo, hi = min(self.a, self.b), max(self.a, self.b)
        pts = [lo] + [p for p in self.points if lo < p < hi] + [hi]
        with mp.workdps(25):
            c = mp.quad(lambda x: (abs(x - end) + abs(x)) * abs(self.df(x)), pts)
        return float(c)

    def __repr__(self):
        return self.name


def _gauss_df(s):
    return lambda x: -2 * (x - s) * mp.exp(-(x - s) ** 2)


def _lorentz_df(s, e):
    return lambda x: -2 * (x - s) / ((x - s) ** 2 + e) ** 2


SQRT_PI = lambda: mp.sqrt(mp.pi)   # noqa: E731
E6 = 1e-6   # the double the literal rounds to is the parameter of the closed form

GAUSS = Case("gauss", "exp(-x*x)", lambda x: np.exp(-x * x), -INF, INF, SQRT_PI,
             _gauss_df(0), [-6, -1, 0, 1, 6])
EXP_UP = Case("exp_upper", "exp(-x)", lambda x: np.exp(-x), 0.0, INF, lambda: _m(1),
              lambda x: -mp.exp(-x), [1, 10, 40])
EXP_LOW = Case("exp_lower", "exp(x)", np.exp, -INF, 0.0, lambda: _m(1), mp.exp, [-40, -10, -1])
CAUCHY = Case("cauchy", "1.0/(1.0+x*x)", lambda x: 1.0 / (1.0 + x * x), -INF, INF,
              lambda: mp.pi, _lorentz_df(0, 1), [-10, -1, 0, 1, 10])
CAUCHY_1 = Case("cauchy_from_1", "1.0/(1.0+x*x)", lambda x: 1.0 / (1.0 + x * x), 1.0, INF,
                lambda: mp.pi / 4, _lorentz_df(0, 1), [2, 10, 100])
GAMMA3 = Case("gamma3", "x*x*exp(-x)", lambda x: x * x * np.exp(-x), 0.0, INF, lambda: _m(2),
              lambda x: (2 * x - x * x) * mp.exp(-x), [2, 10, 40])
PLANCK = Case("planck", "x*x*x/expm1(x)", lambda x: x * x * x / np.expm1(x), 0.0, INF,
              lambda: mp.pi ** 4 / 15,
              lambda x: (3 * x * x * mp.expm1(x) - x ** 3 * mp.exp(x)) / mp.expm1(x) ** 2,
              [1, 3, 10, 40])
GAUSS_M2 = Case("gauss_from_minus_2", "exp(-x*x)", lambda x: np.exp(-x * x), -2.0, INF,
                lambda: mp.sqrt(mp.pi) / 2 * (1 + mp.erf(2)), _gauss_df(0), [-1, 0, 1, 6])
GAUSS_50 = Case("gauss_at_50", "exp(-(x-50)*(x-50))", lambda x: np.exp(-(x - 50) * (x - 50)),
                -INF, INF, SQRT_PI, _gauss_df(50), [0, 44, 49, 50, 51, 56])
RESONANCE = Case("resonance_at_3", "1.0/((x-3)*(x-3)+1e-6)",
                 lambda x: 1.0 / ((x - 3) * (x - 3) + 1e-6), -INF, INF,
                 lambda: mp.pi / mp.sqrt(_m(E6)), _lorentz_df(3, _m(E6)),
                 [0, 2, 2.9, 2.99, 2.999, 3, 3.001, 3.01, 3.1, 4, 10])
POWER = Case("x_to_minus_1.5", "1.0/(x*sqrt(x))", lambda x: 1.0 / (x * np.sqrt(x)), 1.0, INF,
             lambda: _m(2), lambda x: -_m(1.5) * x ** _m(-2.5), [2, 10, 1000])
# the kink at 0.3 (1/3 would map onto the panel edge t = 0.75); |f'| = f away from it
KINK = Case("kink", "exp(-fabs(x-0.3))", lambda x: np.exp(-np.abs(x - 0.3)), -INF, INF,
            lambda: _m(2), lambda x: mp.exp(-abs(x - _m(0.3))), [-40, -1, 0.3, 1, 40])

SMOOTH = [GAUSS, EXP_UP, EXP_LOW, CAUCHY, CAUCHY_1, GAMMA3, PLANCK, GAUSS_M2, GAUSS_50,
          RESONANCE, KINK]
TABLE = SMOOTH + [POWER]   # POWER is a t^-1/2 end singularity at t = 0: floor and forced, converged

# honest failures
DIVERGES = Case("one_over_x", "1.0/x", lambda x: 1.0 / x, 1.0, INF, lambda: mp.inf,
                lambda x: -1 / (x * x), [])
END_SINGULAR = Case("exp_over_sqrt", "exp(-x)/sqrt(x)", lambda x: np.exp(-x) / np.sqrt(x), 0.0,
                    INF, SQRT_PI, None, [])
SPLIT_TAIL = Case("exp_over_sqrt_from_1", "exp(-x)/sqrt(x)", lambda x: np.exp(-x) / np.sqrt(x),
                  1.0, INF, lambda: mp.sqrt(mp.pi) * mp.erfc(1),
                  lambda x: -mp.exp(-x) * (1 / mp.sqrt(x) + 1 / (2 * x * mp.sqrt(x))), [2, 10, 40])
SPLIT_HEAD_TRUTH = float(mp.sqrt(mp.pi) * mp.erf(1))   # the finite call on [0, 1]

ALL = TABLE + [DIVERGES, END_SINGULAR, SPLIT_TAIL]
BY_NAME = {c.name: c for c in ALL}


@functools.lru_cache(maxsize=None)
def _model(case_name, a, b, args):
    from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_model

    case = BY_NAME[case_name]
    return adaptive_model(case.f, a, b, unbounded=True, **dict(args))


def model(case: Case, a=None, b=None, **args) -> dict:
    """adaptive_model (unbounded) of the case, computed once per set of arguments and shared:
    read it, do not change it."""
    a = case.a if a is None else a
    b = case.b if b is None else b
    args.setdefault("max_intervals", MAX_INTERVALS)
    return _model(case.name, float(a), float(b), tuple(sorted(args.items())))


def value_bound(r, case, slack_units: float = 96.0) -> float:
    """The bound of the module docstring; r: an AdaptResult, an AdaptiveResult or the model's
    dict."""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return (max(g("tol"), g("err_est")) + (slack_units + MAP_UNITS) * U * g("resabs")
            + ABSCISSA_HALF_ULPS * 0.5 * U * case.conditioning)


# ------------------------------------------------------------------ sweeps: f(x, p) per row
class Family:
    """f(x, *row) on a shared infinite range; ``truth(*row)`` and ``df(*row)`` per row."""

    def __init__(self, name, expr, f, a, b, rows, truth, df, points):
        self.name, self.expr, self.f, self.a, self.b = name, expr, f, a, b
        self.rows = [tuple(float(v) for v in r) for r in rows]
        self._truth, self._df, self._points = truth, df, points

    @property
    def params(self) -> np.ndarray:
        return np.array(self.rows, dtype=np.float64).reshape(len(self.rows), -1)

    @functools.cached_property
    def truths(self) -> list:
        return [float(self._truth(*r)) for r in self.rows]

    def case(self, k: int) -> Case:
        """Row k as a one-integral case (for its conditioning integral and its model)."""
        row = self.rows[k]
        return Case(f"{self.name}[{k}]", self.expr, lambda x: self.f(x, *row), self.a, self.b,
                    lambda: self._truth(*row), self._df(*row), self._points(*row))

    @functools.cached_property
    def conditionings(self) -> list:
        return [self.case(k).conditioning for k in range(len(self.rows))]

    def __repr__(self):
        return self.name


def _around(s, w):
    """Breakpoints around a feature at s of width w."""
    return [s - 100 * w, s - 10 * w, s - w, s, s + w, s + 10 * w, s + 100 * w]


GAUSS_WIDTHS = Family(
    "gauss_widths", "exp(-p0*x*x)", lambda x, p0: np.exp(-p0 * x * x), -INF, INF,
    [(1e-2,), (1e-1,), (1.0,), (1e1,), (1e2,)], lambda p0: mp.sqrt(mp.pi / _m(p0)),
    lambda p0: (lambda x: -2 * _m(p0) * x * mp.exp(-_m(p0) * x * x)),
    lambda p0: _around(0.0, 1.0 / math.sqrt(p0)))
_P1 = [1e-2, 1e-4, 1.0]
RESONANCES = Family(
    "resonances", "1.0/((x-p0)*(x-p0)+p1)", lambda x, p0, p1: 1.0 / ((x - p0) * (x - p0) + p1),
    -INF, INF, [(-5.0 + 10.0 * i / 99.0, _P1[i % 3]) for i in range(100)],
    lambda p0, p1: mp.pi / mp.sqrt(_m(p1)),
    lambda p0, p1: _lorentz_df(_m(p0), _m(p1)),
    lambda p0, p1: sorted(_around(p0, math.sqrt(p1)) + [0.0]))
DECAYS = Family(
    "decays", "p0*exp(-p0*x)", lambda x, p0: p0 * np.exp(-p0 * x), 0.0, INF,
    [(1e-2,), (0.5,), (1.0,), (30.0,), (1e3,)], lambda p0: _m(1),
    lambda p0: (lambda x: -_m(p0) ** 2 * mp.exp(-_m(p0) * x)),
    lambda p0: [0.1 / p0, 1.0 / p0, 10.0 / p0, 40.0 / p0])
# p1 = 0 is 1.0 / (x + p0), which diverges on (0, inf); p1 = 1 is exp(-x), truth 1
MIXED_EXPR = "p1*exp(-x)+(1.0-p1)/(x+p0)"
MIXED_ROWS = np.array([[1.0, 1.0], [1.0, 0.0], [2.0, 1.0]])


def mixed_f(x, p0, p1):
    return p1 * np.exp(-x) + (1.0 - p1) / (x + p0)


FAMILIES = [GAUSS_WIDTHS, RESONANCES, DECAYS]
FAMILY_BY_NAME = {f.name: f for f in FAMILIES}
SWEEP_SLACK_UNITS = 48.0


@functools.lru_cache(maxsize=None)
def _sweep_model(name, args):
    from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_sweep_model

    fam = FAMILY_BY_NAME[name]
    return adaptive_sweep_model(fam.f, fam.params, fam.a, fam.b, unbounded=True, **dict(args))


def sweep_model(fam: Family, **args) -> dict:
    return _sweep_model(fam.name, tuple(sorted(args.items())))


def row_bound(r, k: int, fam: Family) -> float:
    """The bound of the module docstring for row k of a sweep (S = 48)."""
    g = (lambda key: r[key]) if isinstance(r, dict) else (lambda key: getattr(r, key))
    return (max(float(g("tol")[k]), float(g("err_est")[k]))
            + (SWEEP_SLACK_UNITS + MAP_UNITS) * U * float(g("resabs")[k])
            + ABSCISSA_HALF_ULPS * 0.5 * U * fam.conditionings[k])
