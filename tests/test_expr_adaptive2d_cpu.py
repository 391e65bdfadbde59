"""CPU tests of adaptive double integrals (ExprAdaptive2D, csrc/runtime/expr_adaptive2d.cpp):
the numpy model of the rule against a direct loop, against mpmath truths on every case the GPU
tests use and against the 1-D model, the generated source and its gfx950 compile, every
refusal, the CLIs' conflicts and the cpu backend. No device needed."""
from __future__ import annotations

import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive2d_cases as ac
from cuda_v_mpi_amd import Adaptive2DResult, integrate_expr2d_adaptive, native
from cuda_v_mpi_amd.utils import adaptive_quad as aq
from cuda_v_mpi_amd.utils import adaptive_quad2d as aq2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the rule
def _direct(f, x0, x1, y0, y1):
    """The rule of miint/expr.hpp on one rectangle, operation by operation, with math.fma where
    the kernels use it (Python 3.13) or a product and an add."""
    fma = getattr(math, "fma", lambda a, b, c: a * b + c)
    m = native()
    t, wk, wg = (list(map(float, v)) for v in (m.gk15_nodes()[7:], m.gk15_weights()[7:],
                                               m.gk7_weights()[3:]))
    hx = 0.5 * (x1 - x0)
    cx = x0 + hx
    hy = 0.5 * (y1 - y0)
    cy = y0 + hy

    def row(y):
        f0 = f(cx, y)
        rk, rg, ra = wk[0] * f0, wg[0] * f0, wk[0] * abs(f0)
        for i in range(1, 8):
            f1, f2 = f(fma(hx, -t[i], cx), y), f(fma(hx, t[i], cx), y)
            rk = fma(wk[i], f1 + f2, rk)
            ra = fma(wk[i], abs(f1) + abs(f2), ra)
            if i % 2 == 0:
                rg = fma(wg[i // 2], f1 + f2, rg)
        return rk, rg, ra

    rk, rg, ra = row(cy)
    kk, gk, aa, gg, kg = wk[0] * rk, wk[0] * rg, wk[0] * ra, wg[0] * rg, wg[0] * rk
    for j in range(1, 8):
        (k1, g1, a1), (k2, g2, a2) = row(fma(hy, -t[j], cy)), row(fma(hy, t[j], cy))
        kk = fma(wk[j], k1 + k2, kk)
        gk = fma(wk[j], g1 + g2, gk)
        aa = fma(wk[j], a1 + a2, aa)
        if j % 2 == 0:
            gg = fma(wg[j // 2], g1 + g2, gg)
            kg = fma(wg[j // 2], k1 + k2, kg)
    s = hx * hy
    return s * kk, abs(s * kk - s * gg), abs(s * kk - s * gk), abs(s * kk - s * kg), s * aa


RECTS = [(0.0, 1.0, 0.0, 1.0), (-1.0, 0.25, 0.5, 0.5 + 2.0 ** -20), (0.1, 0.3, -2.0, 5.0)]


@pytest.mark.parametrize("f", [lambda x, y: math.exp(-(x * x + y * y)),
                               lambda x, y: 1.0 / ((x - 0.3) ** 2 + (y + 0.2) ** 2 + 1e-2),
                               lambda x, y: abs(x - y) - 0.25],
                         ids=["gauss", "peak", "kink"])
def test_model_rule_is_the_direct_loop(f):
    """The vectorised rule against the loop, rectangle by rectangle: the same sums in the same
    order, so they differ by the fma's single rounding at most: 38 u of R (the cases file)."""
    r = np.array(RECTS)
    got = aq2.gk15x15(np.vectorize(f), r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(),
                      r[:, 3].copy())
    for i, rect in enumerate(RECTS):
        k, err, ex, ey, ra = _direct(f, *rect)
        noise = 40 * 2.0 ** -53 * ra
        assert abs(got[0][i] - k) <= noise and abs(got[4][i] - ra) <= noise
        for q, want in ((1, err), (2, ex), (3, ey)):
            assert abs(got[q][i] - want) <= 2 * noise
        assert ra > 0 and got[1][i] <= ra


def test_rule_is_exact_on_the_polynomials_both_rules_integrate():
    """x^12 y^10 lies in both product rules' exactness range: all three errors are rounding;
    x^14 y^2 is past the Gauss rule along x only, x^2 y^14 along y only."""
    one = (np.array([0.0]), np.array([1.0]), np.array([0.0]), np.array([2.0]))
    k, err, ex, ey, r = aq2.gk15x15(lambda x, y: x ** 12 * y ** 10, *one)
    assert abs(k[0] - 2.0 ** 11 / (13 * 11)) <= 64 * ac.U * r[0]
    assert max(err[0], ex[0], ey[0]) <= 64 * ac.U * r[0]
    k, err, ex, ey, r = aq2.gk15x15(lambda x, y: x ** 14 * y ** 2, *one)
    assert ex[0] > 1e-9 * r[0] and ey[0] <= 64 * ac.U * r[0] and err[0] > 1e-9 * r[0]
    k, err, ex, ey, r = aq2.gk15x15(lambda x, y: x ** 2 * y ** 14, *one)
    assert ey[0] > 1e-9 * r[0] and ex[0] <= 64 * ac.U * r[0]


def test_first_rectangles_run_x_fastest_with_the_1d_edges():
    x0, x1, y0, y1 = aq2.first_rectangles(-1.0, 2.0, 0.0, 0.7, 3, 5)
    assert x0.shape == (15,) and list(x0[:3]) == [-1.0, -1.0 + 3.0 / 3.0, -1.0 + 6.0 / 3.0]
    assert np.array_equal(x0[:3], x0[3:6]) and x1[2] == 2.0 and y1[-1] == 0.7
    assert np.all(y0[:3] == 0.0) and np.all(y0[3:6] == 0.0 + (0.7 * 1.0) / 5.0)
    assert np.array_equal(x1[:2], x0[1:3]) and np.array_equal(y1[:12], y0[3:])


# ------------------------------------------------------------------ the model's runs
def _identities(r, panels):
    assert r["splits"] == r["splits_x"] + r["splits_y"]
    assert r["intervals"] == panels + r["splits"]
    assert r["evals"] == 225 * (r["intervals"] + r["splits"])
    assert r["rects"].shape == (r["intervals"], 4)
    assert r["converged"] == (r["err_est"] <= r["tol"] and not r["capped"]
                              and r["nonfinite"] == 0)


def _tiles(rects, box):
    x0, x1, y0, y1 = rects.T
    assert np.all(x1 > x0) and np.all(y1 > y0)
    assert (x0.min(), x1.max(), y0.min(), y1.max()) == box
    assert np.array_equal(np.lexsort((x0, y0)), np.arange(len(rects)))


@pytest.mark.parametrize("run", ac.RUNS, ids=ac.run_id)
def test_model_meets_the_truth(run):
    case, rtol, (px, py) = run
    r = ac.run_model(run)
    _identities(r, px * py)
    _tiles(r["rects"], case.box)
    assert r["converged"] == (run not in ac.NOT_CONVERGED)
    assert not r["capped"] and r["nonfinite"] == 0 and r["rounds"] <= 121
    assert abs(r["value"] - case.truth) <= ac.value_bound(r)
    assert r["peak"] <= 4096 and r["evals"] < 2 * 10 ** 7


def test_model_figures_the_gpu_tests_rely_on():
    r = ac.model(ac.KINK, **ac.KINK_ARGS)   # 16 workgroups, splits and acceptances in each
    assert r["peak"] == 4096 and r["rounds"] >= 20 and r["converged"]
    rects = r["rects"]
    assert math.fsum((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])) == 1.0
    r = ac.model(ac.RIDGE, rtol=1e-10, panels_x=64, panels_y=32)
    t = ac.model(ac.RIDGE_T, rtol=1e-10, panels_x=32, panels_y=64)
    assert r["converged"] and t["converged"]
    assert r["splits_y"] == 0 and t["splits_x"] == 0 and r["splits_x"] == t["splits_y"] > 0
    assert abs(r["value"] - t["value"]) <= ac.value_bound(r)
    for shape in ac.SHAPES:
        e = ac.model(ac.EDGE, rtol=1e-10, panels_x=shape[0], panels_y=shape[1])
        assert e["splits_y"] == 0 and e["splits_x"] > 0 and e["rounds"] == 61
    r = ac.model(ac.SQRT_NEG)               # NaN on half of the box: accepted, counted
    assert r["rounds"] == 1 and r["nonfinite"] > 0 and np.isnan(r["value"]) and not r["converged"]
    r = ac.model(ac.DISC, **ac.DISC_ARGS)   # the indicator runs to the cap
    assert r["capped"] and not r["converged"] and r["intervals"] <= 4096
    assert abs(r["value"] - math.pi) <= 1e-3
    _tiles(r["rects"], ac.DISC.box)
    r = ac.model(ac.PEAK, max_depth=0, panels_x=17, panels_y=16)
    assert r["rounds"] == 1 and r["splits"] == 0 and r["forced"] >= 1 and not r["converged"]
    r = ac.model(ac.DIAGONAL, rtol=1e-6, panels_x=1, panels_y=1)   # the reproducibility run
    assert r["intervals"] >= 400 and r["rounds"] >= 10 and r["intervals"] <= 4096


def test_a_y_independent_integrand_follows_the_1d_model():
    """f(x, y) = g(x) on [a, b] x [0, 1]: nothing is ever split along y (ey is rounding), and the
    value is the 1-D model's to both runs' bounds."""
    def g(x):
        return 1.0 / (x * x + 1e-4)

    for px, py in ((1, 1), (16, 3)):
        r2 = aq2.adaptive2d_model(lambda x, y: g(x) + 0.0 * y, -1.0, 1.0, 0.0, 1.0, rtol=1e-9,
                                  panels_x=px, panels_y=py)
        r1 = aq.adaptive_model(g, -1.0, 1.0, rtol=1e-9, panels=px)
        assert r2["converged"] and r1["converged"] and r2["splits_y"] == 0 and r2["splits_x"] > 0
        assert abs(r2["value"] - r1["value"]) <= ac.value_bound(r2) + r1["tol"]
        truth = 2 * math.atan(100.0) * 100.0
        assert abs(r2["value"] - truth) <= ac.value_bound(r2)


def test_model_reversed_and_empty_sides():
    f = ac.PEAK.f
    args = dict(rtol=1e-8, panels_x=5, panels_y=3)
    fwd = aq2.adaptive2d_model(f, -1.0, 0.5, -0.75, 1.0, **args)
    for box, sign in (((0.5, -1.0, -0.75, 1.0), -1.0), ((-1.0, 0.5, 1.0, -0.75), -1.0),
                      ((0.5, -1.0, 1.0, -0.75), 1.0)):
        rev = aq2.adaptive2d_model(f, *box, **args)
        assert rev["value"] == sign * fwd["value"] and rev["err_est"] == fwd["err_est"]
        assert np.array_equal(rev["rects"], fwd["rects"])
    for box in ((0.25, 0.25, 0.0, 1.0), (0.0, 1.0, -0.5, -0.5)):
        z = aq2.adaptive2d_model(f, *box)
        assert z["value"] == 0.0 and z["evals"] == 0 and z["rounds"] == 0 and z["converged"]


# ------------------------------------------------------------------ the source
KERNELS = ("miint_adapt2d_init", "miint_adapt2d_eval", "miint_adapt2d_close",
           "miint_adapt2d_decide", "miint_adapt2d_prefix", "miint_adapt2d_scatter")


def test_source_prints_the_table_as_hex_floats_and_keeps_the_rows_rolled():
    m = native()
    src = m.expr_adapt2d_source("1.0/(x*x+y*y+1e-8)")
    printed = {float.fromhex(h) for h in re.findall(r"0x[01]\.[0-9a-f]*p[+-]\d+", src)}
    table = list(m.gk15_nodes()[8:]) + list(m.gk15_weights()[7:]) + list(m.gk7_weights()[3:])
    assert printed == {float(v) for v in table + [50 * 2.0 ** -52]}   # the centre prints as 0x0p+0
    assert not re.search(r"\d\.\d{6,}", src.replace("1e-8", ""))   # no typed decimal constants
    assert "return (1.0/(x*x+y*y+1e-8));" in src
    for kernel in KERNELS:
        assert f"void {kernel}(" in src
    # fifteen evaluations are written out (one row), not 225: the loop over the rows is rolled
    body = src[src.index("void miint_gk15x15("):src.index("#define MIINT_ST_D")]
    assert body.count("MIINT_ROW_") == 8 and "#pragma unroll 1" in body
    assert "asm" not in src
    with pytest.raises(RuntimeError, match="rejected"):
        m.expr_adapt2d_source("x; y")


def test_compiles_for_gfx950():
    m = native()
    code = m.expr_adapt2d_compile("(x*x+y*y<1.0)?1.0:0.0")
    assert code[:4] == b"\x7fELF" and len(code) > 4096
    for kernel in KERNELS:
        assert kernel.encode() in code
    with pytest.raises(RuntimeError, match="does not compile"):
        m.expr_adapt2d_compile("nosuchfunction(x, y)")


def test_the_1d_sources_do_not_move():
    """Generating and compiling the 2-D kernels leaves the 1-D families' sources as they were."""
    m = native()
    expr = "exp(-x*x)"
    before = (m.expr_adapt_source(expr), m.expr_adapt_unbounded_source(expr),
              m.expr_adapt_sweep_source("exp(-p0*x*x)", 1))
    m.expr_adapt2d_compile("exp(-(x*x+y*y))")
    m.expr_adapt2d_source(expr)
    after = (m.expr_adapt_source(expr), m.expr_adapt_unbounded_source(expr),
             m.expr_adapt_sweep_source("exp(-p0*x*x)", 1))
    assert before == after
    assert "adapt2d" not in before[0] and "miint_gk15x15" not in before[0]


# ------------------------------------------------------------------ refusals
BAD_OPTIONS = [
    (dict(rtol=0.0, atol=0.0), "rtol = 0 and atol = 0"),
    (dict(rtol=-1e-6), "rtol = -"),
    (dict(atol=-1.0), "atol = -1"),
    (dict(rtol=float("nan")), "rtol = nan"),
    (dict(panels_x=0), "panels_x * panels_y = 0 * 64"),
    (dict(panels_y=0), "panels_x * panels_y = 64 * 0"),
    (dict(panels_x=9, panels_y=8, max_intervals=71),
     "panels_x * panels_y = 9 * 8 must be 1..max_intervals = 71"),
    (dict(max_intervals=0), "max_intervals = 0"),
    (dict(max_intervals=(1 << 26) + 1), "max_intervals = 67108865"),
    (dict(max_depth=-1), "max_depth = -1"),
    (dict(max_depth=201), "max_depth = 201"),
]


@pytest.mark.parametrize("opts,message", BAD_OPTIONS, ids=[m for _, m in BAD_OPTIONS])
def test_refusals_name_the_numbers(opts, message):
    m = native()
    full = dict(aq2.DEFAULTS, **opts)
    with pytest.raises(RuntimeError) as e:
        m.adapt2d_check(0.0, 1.0, 0.0, 1.0, m.Adapt2DOptions(**full))
    assert message in str(e.value) and "adaptive 2-D: " in str(e.value)
    with pytest.raises(ValueError) as e:   # the model refuses the same, in the same words
        aq2.adaptive2d_model(lambda x, y: x + y, 0.0, 1.0, 0.0, 1.0, **full)
    assert message in str(e.value)
    from cuda_v_mpi_amd.ops import kernels
    kw = {k: v for k, v in full.items() if k not in ("panels_x", "panels_y")}
    with pytest.raises(RuntimeError) as e:  # before any device call
        kernels.quad_expr2d("x+y", 0.0, 1.0, 0.0, 1.0, panels=(full["panels_x"],
                                                               full["panels_y"]), **kw)
    assert message in str(e.value)


BAD_BOXES = [
    ((0.0, float("inf"), 0.0, 1.0), "ax = 0 and bx = inf must be finite"),
    ((float("nan"), 1.0, 0.0, 1.0), "ax = nan and bx = 1 must be finite"),
    ((0.0, 1.0, float("-inf"), 1.0), "ay = -inf and by = 1 must be finite"),
    ((0.0, 1.0, -1e308, 1e308), "ay = -1e+308 and by = 1e+308 must be finite, and by - ay too"),
    ((-8e307, 8e307, -8e307, 8e307), "the area (bx - ax) * (by - ay) = inf must be finite"),
]


@pytest.mark.parametrize("box,message", BAD_BOXES, ids=[m for _, m in BAD_BOXES])
def test_refuses_an_unbounded_rectangle(box, message):
    m = native()
    with pytest.raises(RuntimeError) as e:
        m.adapt2d_check(*box, m.Adapt2DOptions())
    assert message in str(e.value)
    with pytest.raises(ValueError) as e:
        aq2.adaptive2d_model(lambda x, y: x + y, *box)
    assert message in str(e.value)


def test_options_and_defaults():
    m = native()
    o = m.Adapt2DOptions()
    assert (o.rtol, o.atol, o.panels_x, o.panels_y, o.max_depth, o.max_intervals) == (
        1e-10, 0.0, 64, 64, 60, 1 << 22)
    assert aq2.DEFAULTS == dict(rtol=1e-10, atol=0.0, panels_x=64, panels_y=64, max_depth=60,
                                max_intervals=1 << 22)
    assert m.ADAPT2D_DEFAULT_PANELS == 64
    m.adapt2d_check(1.0, 0.0, 1.0, 0.0, o)     # reversed and empty sides are rectangles
    m.adapt2d_check(1.0, 1.0, 0.0, 1.0, o)
    r = m.Adapt2DResult()
    assert r.as_dict()["splits_x"] == 0 and "splits_y" in r.as_dict()


# ------------------------------------------------------------------ the cpu backend
def test_cpu_backend_runs_the_model_on_expr_torch():
    r = integrate_expr2d_adaptive(ac.PEAK.expr, *ac.PEAK.box, rtol=1e-8, panels_x=4, panels_y=4,
                                  backend="cpu")
    assert isinstance(r, Adaptive2DResult) and r.backend == "cpu" and r.converged
    want = ac.model(ac.PEAK, rtol=1e-8, panels_x=4, panels_y=4)
    assert r.evals == want["evals"] and r.rounds == want["rounds"]
    assert (r.splits_x, r.splits_y) == (want["splits_x"], want["splits_y"])
    assert abs(r.value - want["value"]) <= ac.SLACK_UNITS * ac.U * r.resabs
    assert abs(r.value - ac.PEAK.truth) <= ac.value_bound(r)
    assert r.as_dict()["expr"] == ac.PEAK.expr and r.as_dict()["ay"] == -1.0
    r = integrate_expr2d_adaptive("exp(-(x*x+y*y))", 3.0, 0.0, 0.0, 3.0, atol=1e-12, rtol=0.0,
                                  panels_x=8, panels_y=8, backend="cpu")
    assert r.converged and abs(r.value + ac.GAUSS.truth) <= 1e-12
    with pytest.raises(ValueError, match="backend must be"):
        integrate_expr2d_adaptive("x*y", 0.0, 1.0, 0.0, 1.0, backend="host")
    with pytest.raises(ValueError, match="cpu backend"):
        integrate_expr2d_adaptive(ac.DISC.expr, *ac.DISC.box, backend="cpu")


# ------------------------------------------------------------------ the CLIs
def _riemann(*args, env=None):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def _py(*args, env=None):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300, env=env)


WHO = "--area-rtol / --area-atol"
XY = ("--expr", "x*y", "--a", "0", "--b", "1")
BASE = (*XY, "--ya", "0", "--yb", "1", "--area-rtol", "1e-8")
CONFLICTS = [
    (("--n", "1e6"), "--n"),
    (("--ny", "100"), "--ny"),
    (("--rule", "mid"), "--rule"),
    (("--running",), "--running"),
    (("--params", "rows.txt"), "--params"),
    (("--linspace", "p0=0:1:4"), "--linspace"),
    (("--box", "0:1,0:1"), "--box"),
    (("--rtol", "1e-8"), "--rtol / --atol"),
    (("--atol", "1e-8"), "--rtol / --atol"),
    (("--row-rtol", "1e-8"), "--row-rtol / --row-atol"),
    (("--row-atol", "1e-8"), "--row-rtol / --row-atol"),
    (("--gpus", "2"), "--gpus 2"),
    (("--loopback", "2"), "--loopback"),
    (("--device", "cpu"), "--device cpu"),
]


@pytest.mark.parametrize("extra,named", CONFLICTS, ids=[" ".join(e) for e, _ in CONFLICTS])
def test_native_cli_names_the_conflict(extra, named):
    for tol in (("--area-rtol", "1e-8"), ("--area-atol", "1e-8")):
        p = _riemann(*XY, "--ya", "0", "--yb", "1", *tol, *extra)
        assert p.returncode == 1 and WHO in p.stderr and named in p.stderr, p.stderr


def test_native_cli_refuses_ranks_bad_numbers_stray_flags_and_infinite_sides():
    p = _riemann(*BASE, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode == 1 and "WORLD_SIZE = 2" in p.stderr and WHO in p.stderr
    p = _riemann(*XY, "--area-rtol", "1e-8")
    assert p.returncode == 1 and WHO in p.stderr and "--ya AY --yb BY" in p.stderr
    for flag, value, word in (("--area-rtol", "1e-8x", "--area-rtol must be a number"),
                              ("--area-atol", "small", "--area-atol must be a number"),
                              ("--panels", "12.5", "--panels must be a whole number"),
                              ("--panels-y", "1e2.", "--panels-y must be a whole number"),
                              ("--max-depth", "deep", "--max-depth must be a whole number"),
                              ("--max-intervals", "1e7.", "--max-intervals must be")):
        p = _riemann(*BASE, flag, value)
        assert p.returncode == 1 and word in p.stderr, (flag, p.stderr)
    p = _riemann(*XY, "--ya", "0", "--yb", "1", "--area-rtol", "0")
    assert p.returncode == 1 and "rtol = 0 and atol = 0" in p.stderr
    p = _riemann(*BASE, "--panels", "9", "--panels-y", "8", "--max-intervals", "71")
    assert p.returncode == 1 and "panels_x * panels_y = 9 * 8" in p.stderr
    p = _riemann(*BASE, "--panels", "300", "--max-intervals", "80000")   # --panels-y follows
    assert p.returncode == 1 and "panels_x * panels_y = 300 * 300" in p.stderr
    p = _riemann(*BASE, "--max-depth", "300")
    assert p.returncode == 1 and "max_depth = 300" in p.stderr
    p = _riemann(*XY, "--ya", "0", "--yb", "inf", "--area-rtol", "1e-8")
    assert p.returncode == 1 and "by = inf must be finite" in p.stderr
    p = _riemann("--expr", "x*y", "--a", "-inf", "--b", "1", "--ya", "0", "--yb", "1",
                 "--area-rtol", "1e-8")
    assert p.returncode == 1 and "infinite range" in p.stderr
    p = _riemann(*XY, "--ya", "0", "--yb", "1", "--panels-y", "8", "--n", "100", "--device", "cpu")
    assert p.returncode == 1 and "--panels-y belongs to --area-rtol / --area-atol" in p.stderr
    p = _riemann("--area-rtol", "1e-8", "--device", "cpu", "--n", "1e4")
    assert p.returncode == 1 and "--expr" in p.stderr
    # what was refused before is refused in the same words
    p = _riemann(*XY, "--ya", "0", "--yb", "1", "--rtol", "1e-8")
    assert p.returncode == 1 and "--rtol / --atol choose the samples themselves: --ya" in p.stderr
    p = _riemann("--help")
    assert p.returncode == 0 and "--area-rtol R" in p.stdout and "--panels-y Q" in p.stdout
    assert "splits_x" in p.stdout


def test_python_cli_names_the_conflict():
    for extra, named in ((("--n", "1e6"), "--n"), (("--ny", "100"), "--ny"),
                         (("--rule", "mid"), "--rule"), (("--params", "rows.txt"), "--params"),
                         (("--linspace", "p0=0:1:4"), "--linspace"),
                         (("--box", "0:1,0:1"), "--box"), (("--rtol", "1e-8"), "--rtol / --atol"),
                         (("--row-atol", "1e-8"), "--row-rtol / --row-atol"),
                         (("--device", "cpu"), "--device cpu"),
                         (("--backend", "host"), "--backend host")):
        p = _py(*BASE, *extra)
        assert p.returncode != 0 and WHO in p.stderr and named in p.stderr, p.stderr
    p = _py(*BASE, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode != 0 and "WORLD_SIZE = 2" in p.stderr
    p = _py(*XY, "--area-atol", "1e-8")
    assert p.returncode != 0 and WHO in p.stderr and "--ya AY --yb BY" in p.stderr
    p = _py(*XY, "--ya", "0", "--yb=inf", "--area-rtol", "1e-8")
    assert p.returncode != 0 and "--yb inf" in p.stderr and "finite rectangle" in p.stderr
    p = _py(*XY, "--ya", "0", "--yb", "1", "--panels-y", "8")
    assert p.returncode != 0 and "--panels-y belongs to --area-rtol / --area-atol" in p.stderr
    p = _py("--area-rtol", "1e-8")
    assert p.returncode != 0 and "--expr" in p.stderr
    p = _py(*XY, "--ya", "0", "--yb", "1", "--area-rtol", "0")
    assert p.returncode != 0 and "rtol = 0 and atol = 0" in p.stderr
    p = _py(*XY, "--ya", "0", "--yb", "1", "--rtol", "1e-8")   # as before
    assert p.returncode != 0 and "--rtol / --atol choose the samples themselves: --ya" in p.stderr
    p = _py("--help")
    assert p.returncode == 0 and "--area-rtol" in p.stdout and "--panels-y" in p.stdout
