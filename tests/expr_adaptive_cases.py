"""Cases of the adaptive-integration tests (test_expr_adaptive_cpu.py, test_expr_adaptive_gpu.py):
each integrand as the C++ expression the device compiles, as the numpy function the model
evaluates, its range, and its integral in closed form, evaluated with mpmath at 60 digits.

The model's runs are computed once per process and shared (``model``): the GPU tests compare
the device's counts with them, the CPU tests check the model itself."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 60
U = 2.0 ** -52


class Case:
    def __init__(self, name, expr, f, a, b, truth):
        self.name, self.expr, self.f, self.a, self.b = name, expr, f, a, b
        self._truth = truth

    @functools.cached_property
    def truth(self) -> float:
        return float(self._truth())

    def __repr__(self):
        return self.name


def _m(x):
    return mp.mpf(x)


# 1.0 / ((x - s)^2 + e) on [a, b]: (atan((b - s) / sqrt(e)) - atan((a - s) / sqrt(e))) / sqrt(e)
def _lorentz(a, b, s, e):
    r = mp.sqrt(_m(e))
    return (mp.atan((_m(b) - _m(s)) / r) - mp.atan((_m(a) - _m(s)) / r)) / r


# exp(-k (x - s)^2) on [a, b]
def _gauss(a, b, s, k):
    r = mp.sqrt(_m(k))
    return mp.sqrt(mp.pi) / (2 * r) * (mp.erf(r * (_m(b) - _m(s))) - mp.erf(r * (_m(a) - _m(s))))


PI4 = Case("pi4", "4.0/(1.0+x*x)", lambda x: 4.0 / (1.0 + x * x), 0.0, 1.0, lambda: mp.pi)
GAUSS3 = Case("gauss3", "exp(-x*x)", lambda x: np.exp(-x * x), 0.0, 3.0,
              lambda: _gauss(0, 3, 0, 1))
SMOOTH = [PI4, GAUSS3]

# the doubles the expressions' literals round to are the parameters of the closed forms
RESONANCE = Case("resonance", "1.0/(x*x+1e-8)", lambda x: 1.0 / (x * x + 1e-8), -1.0, 1.0,
                 lambda: _lorentz(-1, 1, 0, 1e-8))
TOLERANCE = [
    RESONANCE,
    Case("offset_resonance", "1.0/((x-0.3)*(x-0.3)+1e-10)",
         lambda x: 1.0 / ((x - 0.3) * (x - 0.3) + 1e-10), 0.0, 1.0,
         lambda: _lorentz(0, 1, 0.3, 1e-10)),
    Case("narrow_gauss", "exp(-1e4*(x-0.37)*(x-0.37))",
         lambda x: np.exp(-1e4 * (x - 0.37) * (x - 0.37)), 0.0, 1.0,
         lambda: _gauss(0, 1, 0.37, 1e4)),
    Case("kink", "fabs(x-1.0/3.0)", lambda x: np.abs(x - 1.0 / 3.0), 0.0, 1.0,
         lambda: (_m(1.0 / 3.0) ** 2 + (1 - _m(1.0 / 3.0)) ** 2) / 2),
    Case("sqrt", "sqrt(x)", np.sqrt, 0.0, 1.0, lambda: _m(2) / 3),
    Case("log", "log(x)", np.log, 0.0, 1.0, lambda: _m(-1)),
    Case("cos200", "cos(200*x)", lambda x: np.cos(200 * x), 0.0, 1.0,
         lambda: mp.sin(200) / 200),
    Case("step", "(x<0.3)?1.0:0.0", lambda x: np.where(x < 0.3, 1.0, 0.0), 0.0, 1.0,
         lambda: _m(0.3)),
]
RTOLS = [1e-6, 1e-10]
# The cases were laid out for 4096 panels (under 1e5 evaluations a call); the tests pass it, so
# they do not move with the default. From 4096 panels the smoother of these need no bisection at all; from 16 every
# one of them does (4 to 81 splits), so the tolerance tests run both.
FEW_PANELS = 16
PANELS = 4096

# several workgroups with interleaved splits: one panel, 11 rounds, a list of up to 998
COS2000 = Case("cos2000", "cos(2000*x)", lambda x: np.cos(2000 * x), 0.0, 1.0,
               lambda: mp.sin(2000) / 2000)
COS2000_ARGS = dict(panels=1, rtol=1e-9)

INV_SQRT = Case("inv_sqrt", "1.0/sqrt(x)", lambda x: 1.0 / np.sqrt(x), 0.0, 1.0, lambda: _m(2))
SQRT_NEG = Case("sqrt_neg", "sqrt(x)", np.sqrt, -1.0, 1.0, lambda: mp.nan)


@functools.lru_cache(maxsize=None)
def _model(case_name, a, b, args):
    from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_model

    case = BY_NAME[case_name]
    return adaptive_model(case.f, a, b, **dict(args))


def model(case: Case, a=None, b=None, **args) -> dict:
    """adaptive_model of the case (on its own range unless a, b are given), computed once per
    set of arguments. The result is shared: read it, do not change it."""
    a = case.a if a is None else a
    b = case.b if b is None else b
    return _model(case.name, float(a), float(b), tuple(sorted(args.items())))


ALL = SMOOTH + TOLERANCE + [COS2000, INV_SQRT, SQRT_NEG]
BY_NAME = {c.name: c for c in ALL}

# The rounding slack of the value, in units of U * resabs (the tests' docstrings derive it).
SLACK_UNITS = 96.0


def value_bound(r) -> float:
    """|value - truth| <= max(tol, err_est) + SLACK_UNITS * U * resabs for a converged run;
    r: an AdaptResult, an AdaptiveResult or the model's dict."""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return max(g("tol"), g("err_est")) + SLACK_UNITS * U * g("resabs")
