"""Cases of the adaptive-sweep tests (test_expr_adaptive_sweep_cpu.py,
test_expr_adaptive_sweep_gpu.py): each family f(x, p) as the C++ expression the device compiles,
as the numpy function the model evaluates, its range, its parameter rows and every row's integral
in closed form, evaluated with mpmath at 60 digits (as expr_adaptive_cases.py does).

The model's runs are computed once per process and shared (``model``): read them, do not change
them."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 60
U = 2.0 ** -52


def _m(x):
    return mp.mpf(x)


class Family:
    """f(x, *row) on [a, b]; ``truth(row)`` is the closed form at the row's doubles."""

    def __init__(self, name, expr, f, a, b, rows, truth, args=None):
        self.name, self.expr, self.f, self.a, self.b = name, expr, f, a, b
        self.rows = [tuple(float(v) for v in r) for r in rows]
        self._truth = truth
        self.args = dict(args or {})   # options the family is always run with

    @property
    def params(self) -> np.ndarray:
        return np.array(self.rows, dtype=np.float64).reshape(len(self.rows), -1)

    @functools.cached_property
    def truths(self) -> list:
        return [float(self._truth(*r)) for r in self.rows]

    def with_rows(self, name, rows):
        return Family(name, self.expr, self.f, self.a, self.b, rows, self._truth, self.args)

    def __repr__(self):
        return self.name


def _lorentz_truth(a, b):
    def t(s, e):
        r = mp.sqrt(_m(e))
        return (mp.atan((_m(b) - _m(s)) / r) - mp.atan((_m(a) - _m(s)) / r)) / r
    return t


def _kink_truth(p0, p1):   # p1 |x - p0| on [0, 1], 0 <= p0 <= 1
    return _m(p1) * (_m(p0) ** 2 + (1 - _m(p0)) ** 2) / 2


# the issue's table: model intervals / rounds at rtol = 1e-10 from 16 panels
LORENTZ = Family("lorentz", "1.0/((x-p0)*(x-p0)+p1)",
                 lambda x, p0, p1: 1.0 / ((x - p0) * (x - p0) + p1), -1.0, 1.0,
                 [(0.0, 1e-8), (0.3, 1e-10), (-0.7, 1e-2), (0.5, 1.0), (0.123, 1e-6)],
                 _lorentz_truth(-1, 1))
LORENTZ_MODEL_INTERVALS = [54, 109, 19, 16, 41]
KINK = Family("kink", "p1*fabs(x-p0)", lambda x, p0, p1: p1 * np.abs(x - p0), 0.0, 1.0,
              [(1.0 / 3.0, 2.0), (0.5, 2.0), (0.7, 2.0), (0.123456, 2.0)], _kink_truth)
STEP = Family("step", "(x<p0)?1.0:0.0", lambda x, p0: np.where(x < p0, 1.0, 0.0), 0.0, 1.0,
              [(1.0 / 3.0,), (0.5,), (0.7,)], lambda p0: _m(p0))
COS = Family("cos", "cos(p0*x)", lambda x, p0: np.cos(p0 * x), 0.0, 1.0,
             [(1.0,), (37.5,), (200.0,), (2000.0,)], lambda p0: mp.sin(_m(p0)) / _m(p0),
             args=dict(panels=1, rtol=1e-9))
FAMILIES = [LORENTZ, KINK, STEP, COS]

# segments across workgroups: the four cosine rows repeated to 7 in mixed order, so several
# ~1000-interval segments sit beside 1-interval ones
COS7 = COS.with_rows("cos7", [(2000.0,), (1.0,), (200.0,), (2000.0,), (37.5,), (1.0,), (2000.0,)])
COS7_ARGS = dict(panels=1, rtol=1e-9, max_intervals=2048, max_total=16384)
_P1 = [1e-2, 1e-4, 1e-6]
LORENTZ100 = LORENTZ.with_rows(
    "lorentz100", [(-0.9 + 1.8 * i / 99.0, _P1[i % 3]) for i in range(100)])
LORENTZ3 = LORENTZ.with_rows("lorentz3", LORENTZ.rows[:3])

# sqrt(x - p0) on [0, 1]: no, 4 and 16 of the 16 panels hold a negative argument
SQRT_SHIFT = Family("sqrt_shift", "sqrt(x-p0)", lambda x, p0: np.sqrt(x - p0), 0.0, 1.0,
                    [(-0.5,), (0.25,), (2.0,)],
                    lambda p0: (2 * ((1 - _m(p0)) ** 1.5 - (-_m(p0)) ** 1.5) / 3
                                if p0 <= 0 else mp.nan))
SQRT_SHIFT_NONFINITE = [0, 4, 16]
# a NaN row between two lorentz rows: sqrt(p1) is NaN for the middle row only
LORENTZ_NAN = Family("lorentz_nan", "1.0/((x-p0)*(x-p0)+sqrt(p1)*sqrt(p1))",
                     lambda x, p0, p1: 1.0 / ((x - p0) * (x - p0) + np.sqrt(p1) * np.sqrt(p1)),
                     -1.0, 1.0, [(0.0, 1e-4), (0.3, -1.0), (-0.7, 1e-2)], lambda s, e: mp.nan)

ALL = FAMILIES + [COS7, LORENTZ100, LORENTZ3, SQRT_SHIFT, LORENTZ_NAN]
BY_NAME = {f.name: f for f in ALL}


@functools.lru_cache(maxsize=None)
def _model(name, args):
    from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_sweep_model

    fam = BY_NAME[name]
    return adaptive_sweep_model(fam.f, fam.params, fam.a, fam.b, **dict(args))


def model(fam: Family, **args) -> dict:
    """adaptive_sweep_model of the family's rows with the family's own options and ``args`` on
    top, computed once per set of arguments and shared."""
    return _model(fam.name, tuple(sorted({**fam.args, **args}.items())))


# The rounding slack of a row's value, in units of U * resabs (test_expr_adaptive_sweep_gpu.py
# derives it from the row kernel's order of summation).
SLACK_UNITS = 48.0


def value_bound(r, k: int) -> float:
    """|value[k] - truth| <= max(tol[k], err_est[k]) + SLACK_UNITS * U * resabs[k] for a
    converged row; r: an AdaptSweepResult, an AdaptiveSweepResult or the model's dict."""
    g = (lambda key: r[key]) if isinstance(r, dict) else (lambda key: getattr(r, key))
    return (max(float(g("tol")[k]), float(g("err_est")[k]))
            + SLACK_UNITS * U * float(g("resabs")[k]))
