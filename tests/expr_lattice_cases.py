"""Inputs of the lattice-rule tests (test_expr_lattice_cpu.py, test_expr_lattice_gpu.py): the
truth cases with closed forms by mpmath, and the exact cases with their integer reference.

Exact cases. The boxes have sides a_j, b_j that are multiples of 2^-E (E = 2) with power-of-two
widths, so with the unit fraction t = N / D (utils.lattice_rule: numerators, denominator) a
coordinate is x_j = X_j / (2^E D) for the integer X_j = A_j D + W_j N, A_j = a_j 2^E,
W_j = (b_j - a_j) 2^E: |X_j| < 2^37. The integrands are piecewise linear or indicators with
small integer coefficients, so every sample is an integer multiple of one quantum q and so is
every partial sum; while max|sample / q| x points stays below 2^53 (``budget``) every partial
sum is exact in fp64 in ANY order, and the device's S_r must equal the integer sum bit for bit.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from cuda_v_mpi_amd.utils import lattice_rule as lr

E = 2   # the boxes' sides are multiples of 2^-E


# ------------------------------------------------------------------------------ truth cases
@dataclasses.dataclass(frozen=True)
class Truth:
    name: str
    expr: str
    box: tuple
    seed: int          # chosen so that the numpy model stays within 3 err_est at m = 12 and 16
    cond: float        # K of the rounding bound (test_expr_lattice_gpu.py)

    def __repr__(self):
        return self.name

    @property
    def d(self):
        return len(self.box)

    def f(self, x: np.ndarray) -> np.ndarray:
        return _TRUTH_F[self.name](x)

    def truth(self) -> float:
        return _truths()[self.name]


def _sum_expr(term: str, d: int) -> str:
    return "+".join(term.format(j=j) for j in range(d))


GAUSS6 = Truth("gauss6", "exp(-(" + _sum_expr("(x{j}-0.5)*(x{j}-0.5)", 6) + "))",
               ((0.0, 1.0),) * 6, seed=1, cond=1.0)
COS8 = Truth("cos8", "cos(" + _sum_expr("x{j}", 8) + ")", ((0.0, 1.0),) * 8, seed=1, cond=4.0)
EXP16 = Truth("exp16", "exp((" + _sum_expr("x{j}", 16) + ")/16.0)", ((0.0, 1.0),) * 16, seed=1,
              cond=1.0)
BALL3 = Truth("ball3", "(x0*x0+x1*x1+x2*x2<1.0)?1.0:0.0", ((-1.0, 1.0),) * 3, seed=1, cond=1.0)
PROD4 = Truth("prod4", "x0*x1*x2*x3", ((0.0, 2.0),) * 4, seed=0, cond=1.0)
TRUTHS = (GAUSS6, COS8, EXP16, BALL3, PROD4)
TRUTH_LEVELS = (12, 16)
TRUTH_SHIFTS = 16

_TRUTH_F = {
    "gauss6": lambda x: np.exp(-((x - 0.5) ** 2).sum(axis=1)),
    "cos8": lambda x: np.cos(x.sum(axis=1)),
    "exp16": lambda x: np.exp(x.sum(axis=1) / 16.0),
    "ball3": lambda x: ((x * x).sum(axis=1) < 1.0).astype(np.float64),
    "prod4": lambda x: x.prod(axis=1),
}
_TRUTH_CACHE: dict = {}


def _truths() -> dict:
    """The closed forms, by mpmath at 40 digits, rounded to doubles. Computed once."""
    if not _TRUTH_CACHE:
        import mpmath as mp

        with mp.workdps(40):
            one = (mp.e ** (1j) - 1) / 1j                       # the integral of e^{ix} on [0, 1]
            _TRUTH_CACHE.update(
                gauss6=float((mp.sqrt(mp.pi) * mp.erf(mp.mpf(1) / 2)) ** 6),
                cos8=float(mp.re(one ** 8)),
                exp16=float((16 * (mp.e ** (mp.mpf(1) / 16) - 1)) ** 16),
                ball3=float(4 * mp.pi / 3),
                prod4=16.0)
    return _TRUTH_CACHE


_MODEL_CACHE: dict = {}


def truth_model(case: Truth, m: int) -> dict:
    """The numpy model's run of a truth case at level m: computed once, shared, not modified."""
    key = (case.name, m)
    if key not in _MODEL_CACHE:
        _MODEL_CACHE[key] = lr.lattice_model(case.f, case.box, m, shifts=TRUTH_SHIFTS,
                                             seed=case.seed)
    return _MODEL_CACHE[key]


# The tolerance walk's cases (GAUSS6 and BALL3 above) and one that is singular on two faces:
# no face is ever evaluated, so no sample is non-finite.
INV_SQRT2 = Truth("inv_sqrt2", "1.0/sqrt(x0*x1)", ((0.0, 1.0),) * 2, seed=0, cond=1.0)
_TRUTH_F["inv_sqrt2"] = lambda x: 1.0 / np.sqrt(x[:, 0] * x[:, 1])


# ------------------------------------------------------------------------------ exact cases
@dataclasses.dataclass(frozen=True)
class Exact:
    name: str
    expr: str
    box: tuple
    indicator: bool = False   # samples are 0 or 1; else integer multiples of 2^-E / D

    def __repr__(self):
        return self.name

    @property
    def d(self):
        return len(self.box)


ABS1 = Exact("abs1", "fabs(x0-0.25)", ((-0.5, 1.5),))
ABSDIFF = Exact("absdiff", "fabs(x0-x1)", ((-1.0, 1.0), (0.25, 0.75)))
MAX3 = Exact("max3", "fmax(fmax(x0,x1),x2)", ((0.0, 1.0), (2.0, -2.0), (-0.5, 0.5)))
SIMPLEX = Exact("simplex", "(x0+x1+x2<1.5)?1.0:0.0", ((0.0, 1.0), (0.0, 2.0), (1.0, 0.0)), True)
LINEAR16 = Exact("linear16", "+".join(f"{j + 1}.0*x{j}" for j in range(16)).replace(
    "1.0*x0", "x0", 1), tuple((-0.5, 0.5) if j % 3 == 0 else (0.0, 1.0) if j % 3 == 1
                              else (0.75, 0.25) for j in range(16)))
EXACTS = (ABS1, ABSDIFF, MAX3, SIMPLEX, LINEAR16)


def box_ints(case: Exact):
    a = [int(lo * (1 << E)) for lo, _ in case.box]
    w = [int((hi - lo) * (1 << E)) for lo, hi in case.box]
    for (lo, hi), ai, wi in zip(case.box, a, w):
        assert ai == lo * (1 << E) and wi == (hi - lo) * (1 << E)
        assert abs(wi) & (abs(wi) - 1) == 0 and wi != 0            # a power-of-two width
    return a, w


def coordinate_ints(case: Exact, numer: np.ndarray, periodic: bool) -> np.ndarray:
    """X_j = A_j D + W_j N as int64, for numerators of shape (..., d)."""
    a, w = box_ints(case)
    big_d = lr.denominator(periodic)
    return (np.array(a, dtype=np.int64) * big_d
            + np.array(w, dtype=np.int64) * numer.astype(np.int64))


def sample_ints(case: Exact, x: np.ndarray, periodic: bool) -> np.ndarray:
    """The samples in units of the case's quantum, from the coordinate integers X (..., d)."""
    if case.name == "abs1":
        return np.abs(x[..., 0] - (1 << (E - 2)) * lr.denominator(periodic))
    if case.name == "absdiff":
        return np.abs(x[..., 0] - x[..., 1])
    if case.name == "max3":
        return x.max(axis=-1)
    if case.name == "simplex":
        return (x.sum(axis=-1) < 3 * (1 << (E - 1)) * lr.denominator(periodic)).astype(np.int64)
    if case.name == "linear16":
        return (x * np.arange(1, 17, dtype=np.int64)).sum(axis=-1)
    raise KeyError(case.name)


def sample_bound(case: Exact, periodic: bool) -> int:
    """An upper bound of |sample / quantum| over the box."""
    a, w = box_ints(case)
    big_d = lr.denominator(periodic)
    side = [max(abs(ai), abs(ai + wi)) * big_d for ai, wi in zip(a, w)]
    if case.name == "abs1":
        return side[0] + (1 << (E - 2)) * big_d
    if case.name == "absdiff":
        return side[0] + side[1]
    if case.name == "max3":
        return max(side)
    if case.name == "simplex":
        return 1
    return sum((j + 1) * s for j, s in enumerate(side))


def budget(case: Exact, periodic: bool, points: int) -> int:
    """max |sample / quantum| x points: below 2^53 every partial sum is exact in fp64."""
    return sample_bound(case, periodic) * points


def exact_reference(case: Exact, m: int, z, words, periodic: bool, begin: int = 0,
                    count: int | None = None, scale: float = 1.0, ranks: int = 1) -> dict:
    """The integer reference: S_r exactly, then est_r, value and err_est by the stated formulas
    in fp64 (utils.lattice_rule.finish)."""
    n = 1 << m
    count = n - begin if count is None else count
    rows = np.asarray(words, dtype=np.uint32).reshape(-1, case.d)
    sums = []
    for row in rows:
        numer = lr.numerators(lr.fractions_u32(m, z, row, begin, count), periodic)
        s_int = int(sample_ints(case, coordinate_ints(case, numer, periodic), periodic).sum())
        assert abs(s_int) < 1 << 53
        sums.append(float(s_int) if case.indicator
                    else math.ldexp(float(s_int), -E) / lr.denominator(periodic))
    vol = 1.0
    for lo, hi in case.box:
        vol *= hi - lo
    out = lr.finish(sums, vol * scale, n)
    out["sums"] = sums
    return out


def words_for(rows: int, d: int, salt: int = 7) -> np.ndarray:
    """Explicit shift words for the exact tests: splitmix64 of another seed, with the first
    row's leading words pinned to the corners 0, 2^31 - 1, 2^31 and 2^32 - 1 of the tent."""
    w = lr.lattice_shifts(0xC0FFEE + salt, rows, d).copy()
    corners = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    for j in range(min(d, 4)):
        w[0, j] = corners[j]
    return w


def z_for(m: int, d: int) -> list:
    """An explicit generating vector for any m >= 2: odd entries below n, spread over the range."""
    n = 1 << m
    return [((0x9E3779B1 * (j + 1)) % n) | 1 for j in range(d)]


def rank_slices(n: int, world: int):
    """(begin, count) of every rank, as the CLI and integrate_to split the points."""
    from cuda_v_mpi_amd.parallel.decomposition import rank_slice

    return [rank_slice(n, r, world) for r in range(world)]
