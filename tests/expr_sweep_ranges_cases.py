"""Cases of the per-row-range and curve tests (test_expr_sweep_ranges_cpu.py, _gpu.py,
test_expr_curve_gpu.py): the families of expr_adaptive_sweep_cases.py with a range per row, the
exact-arithmetic integrands of expr_adaptive_exact_cases.py on per-row ranges, and the curves'
grids with their closed forms. The references are computed once per process and shared: read
them, do not change them."""
from __future__ import annotations

import functools
import struct

import numpy as np

import expr_adaptive_exact_cases as ec
import expr_adaptive_sweep_cases as sc

U = 2.0 ** -52
F64 = ("value", "err_est", "resabs", "tol")
COUNTS = ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite", "capped",
          "converged")


def bits(v) -> str:
    return struct.pack(">d", float(v)).hex()


def row(r, k: int) -> tuple:
    """Everything a result (native, dataclass or dict of arrays) says about row k: the doubles
    as bits, then the counters."""
    g = (lambda key: r[key]) if isinstance(r, dict) else (lambda key: getattr(r, key))
    return tuple(bits(g(f)[k]) for f in F64) + tuple(int(g(f)[k]) for f in COUNTS)


def negated(rw: tuple) -> tuple:
    """The row with its value negated (a > b against b < a)."""
    v = struct.unpack(">d", bytes.fromhex(rw[0]))[0]
    return (bits(-v),) + rw[1:]


class Ranged:
    """A family with one range per row and the options it is always run with (panels and
    max_intervals explicit, so a one-row call resolves to the same numbers)."""

    def __init__(self, name, fam, a, b, args):
        self.name, self.fam = name, fam
        self.a, self.b = [float(v) for v in a], [float(v) for v in b]
        self.args = dict(args)
        assert len(self.a) == len(self.b) == len(fam.rows)
        assert "panels" in self.args and "max_intervals" in self.args

    def __repr__(self):
        return self.name


# every row on its own window: around its peak, beside it, far wider than it, from its peak
_LW = [(-0.25, 0.5), (0.0, 1.0), (-1.0, -0.5), (-2.0, 3.0), (0.123, 0.623)]
LORENTZ16 = Ranged("lorentz-16", sc.LORENTZ, [w[0] for w in _LW], [w[1] for w in _LW],
                   dict(panels=16, max_intervals=256))
# three panels put the rows' boundaries inside waves
LORENTZ3P = Ranged("lorentz-3", sc.LORENTZ, LORENTZ16.a, LORENTZ16.b,
                   dict(panels=3, max_intervals=256))
# 100 rows of 3 panels, each on a window of its own width around its own centre
LORENTZ100 = Ranged("lorentz100x3", sc.LORENTZ100,
                    [p0 - 0.05 - 0.01 * (i % 7) for i, (p0, _) in enumerate(sc.LORENTZ100.rows)],
                    [p0 + 0.02 + 0.03 * (i % 5) for i, (p0, _) in enumerate(sc.LORENTZ100.rows)],
                    dict(panels=3, max_intervals=256))
LORENTZ257 = Ranged("lorentz3x257", sc.LORENTZ3, [-1.0, 0.25, -0.75], [1.0, 0.5, 2.0],
                    dict(panels=257, max_intervals=1024))
# ~1000-interval segments beside 1-interval ones, across workgroups; row 5 runs backwards
COS7 = Ranged("cos7", sc.COS7, [0.0, 0.0, 0.5, 0.25, -1.0, 2.0, 1.0],
              [1.0, 2.0, 1.0, 1.0, 1.0, 0.0, 0.0], sc.COS7_ARGS)
# row 1 runs backwards, row 2 is empty
MIXED = Ranged("lorentz-reversed-and-empty", sc.LORENTZ, [-0.25, 1.0, 0.4, -2.0, 0.123],
               [0.5, 0.0, 0.4, 3.0, 0.623], dict(panels=16, max_intervals=256))
# cos(2000 x) on [0, 1] from one panel takes about 1000 intervals: capped at 256, alone
_CAP_FAM = sc.COS.with_rows("cos-cap", [(1.0,), (2000.0,), (200.0,), (37.5,)])
CAPPED = Ranged("cos-one-row-capped", _CAP_FAM, [0.0, 0.0, 0.5, -1.0], [2.0, 1.0, 1.0, 1.0],
                dict(panels=1, rtol=1e-9, max_intervals=256))
CAPPED_ROW = 1
BITWISE = [LORENTZ16, LORENTZ3P, LORENTZ100, LORENTZ257, COS7, MIXED, CAPPED]


@functools.lru_cache(maxsize=None)
def _model(name):
    from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_sweep_ranges_model

    c = {c.name: c for c in BITWISE}[name]
    return adaptive_sweep_ranges_model(c.fam.f, c.fam.params, c.a, c.b,
                                       **{**c.fam.args, **c.args})


def model(case: Ranged) -> dict:
    """The numpy model's run of the case; shared, so leave it unchanged."""
    return _model(case.name)


# ------------------------------------------------------------------ exact arithmetic
class ExactRanged:
    """An exact-arithmetic integrand on per-row ranges, 150 panels: the ragged 64/64/22 chain."""

    def __init__(self, name, expr, params, a, b, opts):
        self.name, self.expr = name, expr
        self.params = np.asarray(params, dtype=np.float64).reshape(len(a), -1)
        self.a, self.b, self.opts = list(a), list(b), dict(opts)

    def __repr__(self):
        return self.name


_EXACT = dict(panels=ec.SWEEP_PANELS, rtol=1e-10, max_intervals=1 << 10)
# rows of the sweep's own kink family (a linear one, easy ones, the hard one, a repeat), each on
# a range of its own; row 4 backwards, row 5 empty
_KROWS = [ec.SWEEP.params[k] for k in (0, 1, 10, ec.HARD_ROW, 40, 5, 71)]
EXACT_CASES = [
    ExactRanged("kink-ranges", ec.KINK, _KROWS,
                [0.0, 0.0, 0.0, 0.25, 1.0, 0.5, -1.0], [1.0, 0.5, 2.0, 0.75, 0.0, 0.5, 3.0],
                _EXACT),
    ExactRanged("box-ranges", ec.BOX, [[]] * 4, [-1.0, -0.21, 0.0, 2.0], [1.01, 0.83, 5.0, -3.0],
                dict(_EXACT, rtol=1e-6)),
    ExactRanged("zig-ranges", ec.ZIG, [[]] * 3, [0.0, 0.25, 1.0], [1.0, 0.5, 0.5],
                dict(_EXACT, rtol=1e-7, max_intervals=1 << 12)),
]


@functools.lru_cache(maxsize=None)
def _exact(name):
    from cuda_v_mpi_amd.utils.adaptive_curve import sweep_ranges_exact

    c = {c.name: c for c in EXACT_CASES}[name]
    return sweep_ranges_exact(ec.F[c.expr], c.params, c.a, c.b, **c.opts)


def exact(case: ExactRanged) -> dict:
    """The bit-exact reference of the case; shared, so leave it unchanged."""
    return _exact(case.name)


# ------------------------------------------------------------------ curves
# The rounding slack of a curve's point, in units of U * resabs_j. With u = 2^-53 and R_c the
# rule's integral of |f| over cell c (resabs_j is their sum up to the point):
#   * a cell's value is a sweep row's: K_i to 12 u R_i, the round's sum of the row's accepted K
#     (a lane's chain of at most 16 elements, then the butterfly's 6) 21 u, the rounds added in
#     order onto S_acc, at most max_depth + 1 = 61 of them, 61 u: 94 u R_c, as
#     test_expr_adaptive_sweep_gpu.py derives it (without the truth's own rounding);
#   * miint_acurve_prefix: with M <= 256 cells per = 1 and point j is the chain ((0 + I_0) +
#     I_1) + ... + I_{j-1}: at most M additions, each u of a partial sum that |f|'s integral
#     bounds: M u resabs_j;
#   * the truth, rounded to a double: u |truth| <= u resabs_j.
# Together (94 + M + 1) u: for the largest grid here, M = 100, 195 u = 97.5 * 2^-52.
CURVE_SLACK_UNITS = 98.0
CURVE_MAX_CELLS_FOR_SLACK = 100


def curve_bound(r, j: int) -> float:
    return (max(float(r.tol[j]), float(r.err_est[j]))
            + CURVE_SLACK_UNITS * U * float(r.resabs[j]))


ERF_GRID = np.linspace(0.0, 3.0, 101)
ERF_TRUTH = [float(sc.mp.sqrt(sc.mp.pi) / 2 * sc.mp.erf(sc.mp.mpf(float(v)))) for v in ERF_GRID]
RSQRT_GRID = np.array([0.0, 0.01, 0.05, 0.1, 0.25, 0.4, 0.6, 0.8, 1.0])
KINK_GRID = np.array([0.0, 0.25, 0.5, 1.0])  # |x - 0.3| has its kink inside cell 1


def kink_truth(x: float) -> float:
    """The integral of |t - 0.3| from 0 to x, 0.3 being the double the device compiles."""
    x, k = sc.mp.mpf(float(x)), sc.mp.mpf(0.3)
    return float(k * x - x * x / 2 if x <= k else k * k / 2 + (x - k) ** 2 / 2)


def prefix_grid(m: int) -> np.ndarray:
    """M cells of unequal length on [0, 3]."""
    return 3.0 * (np.arange(m + 1) / m) ** 1.5
