"""Cases of the adaptive 2-D tests (test_expr_adaptive2d_cpu.py, test_expr_adaptive2d_gpu.py):
each integrand as the C++ expression the device compiles, as the numpy function the model
evaluates, its rectangle, and its integral in closed form (or, for one, with the inner integral
in closed form and the outer one by mpmath's quadrature), evaluated with mpmath at 60 digits.

The model's runs are computed once per process and shared (``model``): the GPU tests compare
the device's counts with them, the CPU tests check the model itself.

The value's bound. A converged run is held to

    |value - truth| <= max(tol, err_est) + SLACK_UNITS * 2^-52 * resabs

The first term is what the rule promises. The second is rounding, which the estimate does not
see. With u = 2^-53 and R_i the rule's integral of |f| over rectangle i (resabs is their sum),
from the kernels' own order of summation:
  * K_i: f to 2 u relative (the device library's bound for the functions used here); a row: the
    pair sum u and eight chained fma u each, 9 u; the rows: the sum of a pair of rows u and
    eight chained fma u each, 9 u; s = hx * hy and its product with KK, 2 u: 22 u R_i;
  * the round's sum of the accepted K: a 64-lane butterfly (6 additions), the four waves (2),
    then in the closing workgroup a run of at most ceil(workgroups / 256) <= 64 partials and
    another butterfly and four waves (8): at most 80 u R of the round;
  * the rounds, added in order: at most 2 * 60 + 1 = 121 additions, 121 u R;
  * the truth, rounded to a double: u |truth| <= u R.
Together 224 u R = 112 * 2^-52 R; the tests use 128. The model's own sums (a product and an
add for every fma: 16 u for each chain of eight, 38 u R_i; numpy's pairwise sum of a round,
about log2(n) <= 22 additions) stay inside the same 256 u. What f makes of a rounded argument
is not rounding of the sums and is not in the slack."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 60
U = 2.0 ** -52
SLACK_UNITS = 128.0


class Case:
    def __init__(self, name, expr, f, box, truth):
        self.name, self.expr, self.f, self.box = name, expr, f, box   # box: ax, bx, ay, by
        self._truth = truth

    @functools.cached_property
    def truth(self) -> float:
        return float(self._truth())

    def __repr__(self):
        return self.name


def _m(x):
    return mp.mpf(x)


# the doubles the expressions' literals round to are the parameters of the closed forms
def _peak_truth():
    sx, sy, e = _m(0.3), _m(0.2), _m(1e-4)

    def inner(y):   # the integral over x in [-1, 1] of 1 / ((x - sx)^2 + c^2)
        c = mp.sqrt((y + sy) ** 2 + e)
        return (mp.atan((1 - sx) / c) + mp.atan((1 + sx) / c)) / c

    return mp.quad(inner, [-1, -0.5, -0.3, -0.22, -sy, -0.18, -0.1, 0.2, 1])


def _ridge_truth():
    r = mp.sqrt(_m(1e-6))
    return 2 * mp.atan(1 / r) / r * mp.sin(1)


def _diagonal_truth():   # 2 * the integral of (1 - u) / (u^2 + e) over u in [0, 1]
    e = _m(1e-4)
    r = mp.sqrt(e)
    return 2 * (mp.atan(1 / r) / r - mp.log((1 + e) / e) / 2)


UNIT = (0.0, 1.0, 0.0, 1.0)
GAUSS = Case("gauss", "exp(-(x*x+y*y))", lambda x, y: np.exp(-(x * x + y * y)),
             (0.0, 3.0, 0.0, 3.0), lambda: (mp.sqrt(mp.pi) / 2 * mp.erf(3)) ** 2)
PEAK = Case("peak", "1.0/((x-0.3)*(x-0.3)+(y+0.2)*(y+0.2)+1e-4)",
            lambda x, y: 1.0 / ((x - 0.3) * (x - 0.3) + (y + 0.2) * (y + 0.2) + 1e-4),
            (-1.0, 1.0, -1.0, 1.0), _peak_truth)
RIDGE = Case("ridge", "cos(y)/(x*x+1e-6)", lambda x, y: np.cos(y) / (x * x + 1e-6),
             (-1.0, 1.0, 0.0, 1.0), _ridge_truth)
RIDGE_T = Case("ridge_t", "cos(x)/(y*y+1e-6)", lambda x, y: np.cos(x) / (y * y + 1e-6),
               (0.0, 1.0, -1.0, 1.0), _ridge_truth)
DIAGONAL = Case("diagonal", "1.0/((x-y)*(x-y)+1e-4)",
                lambda x, y: 1.0 / ((x - y) * (x - y) + 1e-4), UNIT, _diagonal_truth)
KINK = Case("kink", "fabs(x-y)", lambda x, y: np.abs(x - y), UNIT, lambda: _m(1) / 3)
CORNER = Case("corner", "1.0/sqrt(x*x+y*y)", lambda x, y: 1.0 / np.sqrt(x * x + y * y), UNIT,
              lambda: 2 * mp.asinh(1))
EDGE = Case("edge", "(1.0+y)/sqrt(x)", lambda x, y: (1.0 + y) / np.sqrt(x), UNIT,
            lambda: _m(3))
LOG_CORNER = Case("log_corner", "log(x*x+y*y)", lambda x, y: np.log(x * x + y * y), UNIT,
                  lambda: mp.log(2) - 3 + mp.pi / 2)
SQRT_NEG = Case("sqrt_neg", "sqrt(x-y)", lambda x, y: np.sqrt(x - y), UNIT, lambda: mp.nan)
DISC = Case("disc", "(x*x+y*y<1.0)?1.0:0.0", lambda x, y: np.where(x * x + y * y < 1.0, 1.0, 0.0),
            (-1.0, 1.0, -1.0, 1.0), lambda: mp.pi)
DISC_ARGS = dict(atol=1e-3, rtol=0.0, panels_x=4, panels_y=4, max_intervals=4096)
KINK_ARGS = dict(rtol=1e-6, panels_x=1, panels_y=1)   # 23 rounds, 8188 rectangles, peak 4096

ALL = [GAUSS, PEAK, RIDGE, RIDGE_T, DIAGONAL, KINK, CORNER, EDGE, LOG_CORNER, SQRT_NEG, DISC]
BY_NAME = {c.name: c for c in ALL}

# The panel shapes every converged case runs at: one rectangle, two odd counts, a list that
# crosses a workgroup (17 * 16 = 272 > 256), and the default.
SHAPES = [(1, 1), (3, 5), (17, 16), (64, 64)]
# (case, rtol) of the converged runs; every one at every shape. |x - y| stays at 1e-6: at 1e-10
# it needs more than 2^18 rectangles.
CONVERGED = [(GAUSS, 1e-10), (GAUSS, 1e-6), (PEAK, 1e-8), (RIDGE, 1e-10), (DIAGONAL, 1e-6),
             (KINK, 1e-6), (CORNER, 1e-10), (EDGE, 1e-10), (LOG_CORNER, 1e-10)]
RUNS = [(c, rtol, s) for c, rtol in CONVERGED for s in SHAPES]
RUNS += [(GAUSS, 1e-10, (4, 4)), (PEAK, 1e-10, (64, 64)), (PEAK, 1e-8, (4, 4))]
# From 3 x 5 the ridge sits inside the middle column: the first rounds' sum_K is far too large,
# so is their tolerance, and rectangles accepted then carry more error than the final tolerance
# allows. The run says so: err_est is 2.7 times tol, no cap, nothing forced.
NOT_CONVERGED = [(RIDGE, 1e-10, (3, 5))]


def run_id(run) -> str:
    case, rtol, (px, py) = run
    return f"{case.name}-{rtol:g}-{px}x{py}"


@functools.lru_cache(maxsize=None)
def _model(case_name, box, args):
    from cuda_v_mpi_amd.utils.adaptive_quad2d import adaptive2d_model

    return adaptive2d_model(BY_NAME[case_name].f, *box, **dict(args))


def model(case: Case, box=None, **args) -> dict:
    """adaptive2d_model of the case (on its own rectangle unless ``box`` is given), computed once
    per set of arguments. The result is shared: read it, do not change it."""
    box = case.box if box is None else box
    return _model(case.name, tuple(float(v) for v in box), tuple(sorted(args.items())))


def run_model(run) -> dict:
    case, rtol, (px, py) = run
    return model(case, rtol=rtol, panels_x=px, panels_y=py)


def value_bound(r) -> float:
    """|value - truth| <= max(tol, err_est) + SLACK_UNITS * U * resabs for a converged run;
    r: an Adapt2DResult, an Adaptive2DResult or the model's dict."""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return max(g("tol"), g("err_est")) + SLACK_UNITS * U * g("resabs")
