"""The cases of the oscillatory integrator's tests (test_expr_osc_cpu.py, test_expr_osc_gpu.py):
the expression as the device compiles it, the same f in numpy, the range, omega, the kind, the
tolerances, and a 30-digit truth from mpmath (computed once per process, on demand).
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    expr: str
    a: float
    b: float
    omega: float
    kind: str
    atol: float = 0.0
    rtol: float = 1e-10
    breaks: tuple = ()      # where mpmath must split the range (a kink, a peak)

    @property
    def id(self) -> str:
        return f"{self.name}-{self.kind}-w{self.omega:g}"


def _fma(a, b, c):
    from cuda_v_mpi_amd import native

    return native().fma(a, b, c)


# f as the device forms it: the expression itself is compiled with contraction on (only the
# rule around it turns it off), so a product that feeds a sum is one fma.
F = {
    "1.0/(1.0+x*x)": lambda x: 1.0 / _fma(x, x, 1.0),
    "exp(-x*x)": lambda x: np.exp(-x * x),
    "1.0/((x-0.3)*(x-0.3)+1e-4)": lambda x: 1.0 / _fma(x - 0.3, x - 0.3, 1e-4),
    "fabs(x-0.3)": lambda x: np.abs(x - 0.3),
    "sqrt(x)": lambda x: np.sqrt(x),
    "x*x*x - x": lambda x: _fma(x * x, x, -x),
    "1.0/x": lambda x: 1.0 / x,
    "x/(1.0+x*x)": lambda x: x / _fma(x, x, 1.0),
    "exp(-x)": lambda x: np.exp(-x),
    "1.0": lambda x: np.ones_like(x),
}


def f_numpy(expr: str):
    return F[expr]


def f_mp(expr: str):
    import mpmath as mp

    return {
        "1.0/(1.0+x*x)": lambda x: 1 / (1 + x * x),
        "exp(-x*x)": lambda x: mp.exp(-x * x),
        "1.0/((x-0.3)*(x-0.3)+1e-4)": lambda x: 1 / ((x - mp.mpf(0.3)) ** 2 + mp.mpf(1e-4)),
        "fabs(x-0.3)": lambda x: abs(x - mp.mpf(0.3)),
        "sqrt(x)": mp.sqrt,
        "x*x*x - x": lambda x: x * x * x - x,
        "1.0/x": lambda x: 1 / x,
        "x/(1.0+x*x)": lambda x: x / (1 + x * x),
        "exp(-x)": lambda x: mp.exp(-x),
    }[expr]


LORENTZ = "1.0/(1.0+x*x)"
PEAK = "1.0/((x-0.3)*(x-0.3)+1e-4)"

# the finite cases of the issue, in its order
FINITE = tuple(
    [Case("lorentz", LORENTZ, 0.0, 10.0, w, kind) for kind in ("cos", "sin")
     for w in (0.0, 1.0, 50.0, 1e4)]
    + [Case("gauss", "exp(-x*x)", -3.0, 3.0, 20.0, "cos", atol=1e-14)]
    + [Case("peak", PEAK, -1.0, 1.0, 200.0, kind, breaks=(0.3,)) for kind in ("cos", "sin")]
    + [Case("kink", "fabs(x-0.3)", 0.0, 1.0, 100.0, kind, breaks=(0.3,))
       for kind in ("cos", "sin")]
    + [Case("sqrt", "sqrt(x)", 0.0, 1.0, 10.0, kind) for kind in ("cos", "sin")])

# omega = 0 on the device: every field and the partition bitwise the model's
ZERO = tuple([c for c in FINITE if c.omega == 0.0]
             + [Case("odd_cubic", "x*x*x - x", -1.0, 2.0, 0.0, "sin")])

PANELS = (4, 64)


@dataclasses.dataclass(frozen=True)
class Tail:
    name: str
    expr: str
    a: float
    omega: float
    kind: str
    atol: float = 1e-10

    @property
    def id(self) -> str:
        return f"{self.name}-{self.kind}-w{self.omega:g}"


TAILS = (Tail("recip", "1.0/x", 1.0, 1.0, "sin"),
         Tail("recip", "1.0/x", 1.0, 2.0, "cos"),
         Tail("lorentz", LORENTZ, 0.0, 0.5, "cos"),
         Tail("lorentz", LORENTZ, 0.0, 3.0, "cos"),
         Tail("xlorentz", "x/(1.0+x*x)", 0.0, 1.0, "sin"),
         Tail("decay", "exp(-x)", 0.0, 10.0, "cos"))
TAILS_GPU = (TAILS[0], TAILS[5])
DIVERGENT = Tail("one", "1.0", 0.0, 1.0, "cos")


WEIGHT_PARS = (0.0, 1e-8, 1e-3, 0.5, 2.0, 7.0, 24.0, 25.0, 100.0, 1e3, 1e5, 1e7)


def weights_mp(par: float, n: int):
    """(Wc, Ws) of the (n + 1)-node rule at par >= 0, 50 digits, by a route of its own per
    regime. The moments M_k of T_k against exp(i par t): below 200 from the Bessel series with
    mpmath's own J_n; from 200 on by parts, the finite sum over the derivatives of T_k at the
    ends, T_k^(d)(1) = prod_{m<d} (k^2 - m^2) / (2 m + 1), at 150 digits. Then the cosine sum
    of miint/expr.hpp."""
    import mpmath as mp

    with mp.workdps(150 if par >= 200 else 60):
        p = mp.mpf(par)
        mom = []
        for k in range(n + 1):
            if p == 0:
                mom.append(mp.mpc(0 if k % 2 else mp.mpf(2) / (1 - k * k), 0))
            elif par < 200:
                top = int(par) + 120
                s = mp.mpf(0)
                for q in range(k % 2, top + 1, 2):
                    pair = mp.mpf(1) / (1 - (k + q) ** 2) + mp.mpf(1) / (1 - (k - q) ** 2)
                    s += (1 if q == 0 else 2) * (-1) ** (q // 2) * mp.besselj(q, p) * pair
                mom.append(mp.mpc(s, 0) if k % 2 == 0 else mp.mpc(0, s))
            else:
                total, deriv = mp.mpc(0), mp.mpf(1)
                for d in range(k + 1):
                    at_minus = (-1) ** (k + d) * deriv
                    total += ((-1) ** d * (deriv * mp.expj(p) - at_minus * mp.expj(-p))
                              / (1j * p) ** (d + 1))
                    deriv = deriv * (k * k - d * d) / (2 * d + 1)
                mom.append(total)
        wc, ws = [], []
        for j in range(n + 1):
            sc = ss = mp.mpf(0)
            for k in range(n + 1):
                half = mp.mpf(1) / 2 if k in (0, n) else 1
                ck = mp.cos(j * k * mp.pi / n)
                sc += half * ck * mom[k].real
                ss += half * ck * mom[k].imag
            scale = mp.mpf(2) / n * (mp.mpf(1) / 2 if j in (0, n) else 1)
            wc.append(+(scale * sc))
            ws.append(+(scale * ss))
        return wc, ws


def lorentz_truth(b: float, omega: float, kind: str) -> float:
    """The integral of exp(i w x) / (1 + x^2) on [0, b] in closed form: the integral to infinity,
    (pi / 2) e^-w + i (e^-w Ei(w) - e^w Ei(-w)) / 2, less the tail from b, which with
    1 / (1 + x^2) = (1 / (x - i) - 1 / (x + i)) / (2 i) is
    (e^-w E1(-w - i w b) - e^w E1(w - i w b)) / (2 i). test_expr_osc_cpu.py checks it against
    plain quadrature at w = 1 and 50."""
    import mpmath as mp

    with mp.workdps(40):
        w, bb = mp.mpf(omega), mp.mpf(b)
        if w == 0:
            return float(mp.atan(bb)) if kind == "cos" else 0.0
        whole = mp.pi / 2 * mp.exp(-w) + 1j * (mp.exp(-w) * mp.ei(w) - mp.exp(w) * mp.ei(-w)) / 2
        tail = (mp.exp(-w) * mp.e1(-w - 1j * w * bb) - mp.exp(w) * mp.e1(w - 1j * w * bb)) / 2j
        v = whole - tail
        return float(v.real if kind == "cos" else v.imag)


@functools.lru_cache(maxsize=None)
def truth(case: Case) -> float:
    """The integral to 30 digits: mpmath's Gauss-Legendre on pieces of at most two periods of
    the weight, split also at the case's own breaks."""
    import mpmath as mp

    if case.expr == LORENTZ and case.a == 0.0:
        return lorentz_truth(case.b, case.omega, case.kind)
    with mp.workdps(30):
        f = f_mp(case.expr)
        w = mp.mpf(case.omega)
        osc = mp.cos if case.kind == "cos" else mp.sin
        a, b = mp.mpf(case.a), mp.mpf(case.b)
        pieces = max(8, int(math.ceil(abs(case.omega) * (case.b - case.a) / (4 * math.pi))))
        pts = sorted(set([a + (b - a) * i / pieces for i in range(pieces + 1)]
                         + [mp.mpf(x) for x in case.breaks]))
        if case.name in ("peak", "sqrt"):  # refine towards the peak or the end's root
            x0 = mp.mpf(case.breaks[0]) if case.breaks else a
            pts = sorted(set(pts + [x0 + s * mp.mpf(2) ** -i for i in range(1, 40)
                                    for s in (1, -1) if a <= x0 + s * mp.mpf(2) ** -i <= b]))
        total = mp.mpf(0)
        for lo, hi in zip(pts[:-1], pts[1:]):
            total += mp.quad(lambda x: f(x) * osc(w * x), [lo, hi])
        return float(total)


@functools.lru_cache(maxsize=None)
def tail_truth(case: Tail) -> float:
    """Closed forms where the issue names them, mpmath's quadosc otherwise."""
    import mpmath as mp

    with mp.workdps(30):
        w = mp.mpf(case.omega)
        if case.expr == "1.0/x" and case.kind == "sin":
            return float(mp.pi / 2 - mp.si(w * mp.mpf(case.a)))
        if case.expr == "1.0/x" and case.kind == "cos":
            return float(-mp.ci(w * mp.mpf(case.a)))
        if case.expr == LORENTZ and case.kind == "cos" and case.a == 0.0:
            return float(mp.pi / 2 * mp.exp(-w))
        if case.expr == "x/(1.0+x*x)" and case.kind == "sin" and case.a == 0.0:
            return float(mp.pi / 2 * mp.exp(-w))
        if case.expr == "exp(-x)" and case.kind == "cos" and case.a == 0.0:
            return float(1 / (1 + w * w))
        raise KeyError(case.id)
