"""Cases of the region tests (test_expr_region_cpu.py, test_expr_region_gpu.py): double integrals
of f(x, y) for y between two curves, each as the three C++ expressions the device compiles (f,
the lower and the upper limit), as the three numpy functions the model evaluates, its x range,
and its integral in closed form (for one, the inner integral in closed form and the outer one by
mpmath's quadrature), evaluated with mpmath at 60 digits.

The model's runs are computed once per process and shared (``model``): the GPU tests compare
the device's counts with them, the CPU tests check the model itself.

The value's bound. A converged run is held to

    |value - truth| <= max(tol, err_est) + SLACK_UNITS * 2^-52 * resabs

as the rectangle's cases are (expr_adaptive2d_cases.py), resabs now the rule's integral of
|f (h - g)|. The first term is what the rule promises; the second is rounding. With u = 2^-53
and R_i the rule's integral of |f (h - g)| over rectangle i, from the kernels' own order of
summation, which is ExprAdaptive2D's after the 225 values:
  * a value f(x_i, y_ij) * w_i: f to 2 u relative (the device library's bound for the functions
    used here), the product by w_i u, and w_i itself: the subtraction u and the library's bound
    for the limits, 2 u of |g_i| and 2 u of |h_i|, which is 2 u (|g_i| + |h_i|) / |w_i| of the
    value. That ratio is a property of the case:
      - the disc's limits -+sqrt(1 - x^2): |g| + |h| = |w|, 2 u (and the subtraction is exact);
      - a lower limit 0.0 with the upper limit x or 3.0: both exact, 0;
      - the parabola's x*x .. x: h exact, g one correctly rounded product, u x^2 absolute, which
        is unbounded relative to w = x - x^2 at x = 1 but 0.475 u against resabs = 0.15 once
        integrated with f = x + y (the integral of x^2 (3 x / 2 + x^2 / 2) over [0, 1]): 3.2 u.
    At most 4 u. The fma that forms y_ij is counted as u as well, although it moves f's argument
    and not the sum: 2 + 1 + 1 + 4 + 1 = 9 u where the rectangle's value has 2 u;
  * K_i: the rectangle file's 22 u R_i (a row 9 u, the rows 9 u, s and its product 2 u, f 2 u)
    becomes 29 u R_i;
  * the round's sum of the accepted K: at most 80 u R of the round; the rounds, added in order:
    at most 121 u R; the truth, rounded to a double: u R. All as for the rectangle.
Together 231 u R = 115.5 * 2^-52 R; the tests use 128, the rectangle file's figure, which holds
here too. The model's own sums (a product and an add for every fma, numpy's pairwise sum of a
round) stay inside the same 256 u, as there. What f or a limit makes of a rounded argument is
conditioning, not rounding of the sums, and is not in the slack: the cancellation in 1.0-x*x
loses what x's rounding loses, and the disc cases are held at rtol 1e-10, where that is below
1e-15."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

import expr_adaptive2d_cases as rect_cases

mp.mp.dps = 60
U = 2.0 ** -52
SLACK_UNITS = 128.0


class Case:
    def __init__(self, name, expr, y_lo, y_hi, f, g, h, xrange, truth, args=None):
        self.name, self.expr, self.y_lo, self.y_hi = name, expr, y_lo, y_hi
        self.f, self.g, self.h, self.xrange = f, g, h, xrange      # xrange: ax, bx
        self._truth = truth
        self.args = dict(args or dict(rtol=1e-10))                   # the tolerance it is held at

    @functools.cached_property
    def truth(self) -> float:
        return float(self._truth())

    @property
    def triple(self):
        return self.expr, self.y_lo, self.y_hi

    def __repr__(self):
        return self.name


def _m(x):
    return mp.mpf(x)


def _root(x):
    return np.sqrt(1.0 - x * x)


def _zero(x):
    return 0.0 * x


def _peak_in_disc_truth():
    """The inner integral over y in [-s, s], s = sqrt(1 - x^2), of 1 / ((x - sx)^2 + (y + sy)^2
    + e) in closed form; the outer one by quadrature, broken at the peak."""
    sx, sy, e = _m(0.3), _m(0.2), _m(1e-4)

    def inner(x):
        s = mp.sqrt(1 - x * x)
        c = mp.sqrt((x - sx) ** 2 + e)
        return (mp.atan((s + sy) / c) + mp.atan((s - sy) / c)) / c

    return mp.quad(inner, [-1, -0.5, 0, 0.2, 0.28, sx, 0.32, 0.4, 0.7, 1])


DISC_LIMITS = dict(y_lo="-sqrt(1.0-x*x)", y_hi="sqrt(1.0-x*x)", g=lambda x: -_root(x), h=_root)
DISC = Case("disc", "1.0", f=lambda x, y: 1.0 + 0.0 * x, xrange=(-1.0, 1.0),
            truth=lambda: mp.pi, **DISC_LIMITS)
DISC_GAUSS = Case("disc_gauss", "exp(-(x*x+y*y))", f=lambda x, y: np.exp(-(x * x + y * y)),
                  xrange=(-1.0, 1.0), truth=lambda: mp.pi * (1 - mp.exp(-1)), **DISC_LIMITS)
TRIANGLE = Case("triangle", "x*y", "0.0", "x", lambda x, y: x * y, _zero, lambda x: x,
                (0.0, 1.0), lambda: _m(1) / 8)
PARABOLA = Case("parabola", "x+y", "x*x", "x", lambda x, y: x + y, lambda x: x * x, lambda x: x,
                (0.0, 1.0), lambda: _m(3) / 20)
DUFFY = Case("duffy", "1.0/sqrt(x*x+y*y)", "0.0", "x", lambda x, y: 1.0 / np.sqrt(x * x + y * y),
             _zero, lambda x: x, (0.0, 1.0), lambda: mp.asinh(1))
PEAK_IN_DISC = Case("peak_in_disc", rect_cases.PEAK.expr, f=rect_cases.PEAK.f, xrange=(-1.0, 1.0),
                    truth=_peak_in_disc_truth, **DISC_LIMITS)
# h < g on [-1, 0): that half counts negatively and the two cancel
CROSSING = Case("crossing", "1.0", "0.0", "x", lambda x, y: 1.0 + 0.0 * x, _zero, lambda x: x,
                (-1.0, 1.0), lambda: _m(0), args=dict(atol=1e-10, rtol=0.0))
# constant limits: the rectangle [0, 3] x [0, 3] of the 2-D cases' GAUSS
CONSTANT = Case("constant", rect_cases.GAUSS.expr, "0.0", "3.0", rect_cases.GAUSS.f, _zero,
                lambda x: 3.0 + 0.0 * x, (0.0, 3.0), rect_cases.GAUSS._truth)

ALL = [DISC, DISC_GAUSS, TRIANGLE, PARABOLA, DUFFY, PEAK_IN_DISC, CROSSING, CONSTANT]
BY_NAME = {c.name: c for c in ALL}

# The panel shapes every case runs at: one rectangle, odd counts, a list that crosses a
# 256-lane workgroup (17 * 16 = 272), and the default.
SHAPES = [(1, 1), (3, 5), (17, 16), (64, 64)]
RUNS = [(c, s) for c in ALL for s in SHAPES]


def run_id(run) -> str:
    case, (px, py) = run
    return f"{case.name}-{px}x{py}"


@functools.lru_cache(maxsize=None)
def _model(case_name, xrange, args):
    from cuda_v_mpi_amd.utils.adaptive_quad2d import region_model

    c = BY_NAME[case_name]
    return region_model(c.f, c.g, c.h, *xrange, **dict(args))


def model(case: Case, xrange=None, **args) -> dict:
    """region_model of the case (on its own x range unless ``xrange`` is given), computed once
    per set of arguments. The result is shared: read it, do not change it."""
    xrange = case.xrange if xrange is None else xrange
    return _model(case.name, tuple(float(v) for v in xrange), tuple(sorted(args.items())))


def run_args(run) -> dict:
    case, (px, py) = run
    return dict(case.args, panels_x=px, panels_y=py)


def run_model(run) -> dict:
    return model(run[0], **run_args(run))


def value_bound(r) -> float:
    """|value - truth| <= max(tol, err_est) + SLACK_UNITS * U * resabs for a converged run;
    r: an Adapt2DResult, an AdaptiveRegionResult or the model's dict."""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return max(g("tol"), g("err_est")) + SLACK_UNITS * U * g("resabs")
