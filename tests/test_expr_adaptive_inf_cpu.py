"""Infinite and half-infinite ranges of the adaptive integrators, without a device: the map's
host function against exact rationals, the numpy model on the cases of expr_adaptive_inf_cases.py
(whose docstring derives the value's bound), the sweep model, every refusal natively and in
numpy, the defaults, the generated sources and their gfx950 compile, and the CLIs' conflicts."""
from __future__ import annotations

import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive_cases as ac
import expr_adaptive_inf_cases as ic
from cuda_v_mpi_amd import (AdaptiveResult, integrate_expr_adaptive,
                            integrate_expr_adaptive_sweep, native)
from cuda_v_mpi_amd.utils import adaptive_quad as aq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
COUNTS = ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite", "capped",
          "converged")


# ------------------------------------------------------------------ the map, operation by operation
def _ts():
    rng = np.random.default_rng(7)
    t = np.concatenate([
        rng.uniform(0.0, 1.0, 400), rng.uniform(0.0, 0.5, 200), 10.0 ** rng.uniform(-300, -1, 200),
        [1.0, 0.5, 0.25, 0.75, np.nextafter(1.0, 0.0), np.nextafter(0.5, 0.0),
         np.nextafter(0.5, 1.0), 2.0 ** -60, 1.0 / 3.0, 0.1, 3e-16, 5e-324 * 2 ** 600]])
    return t[(t > 0.0) & (t <= 1.0)]


def _rn(v: Fraction) -> float:
    """The double nearest to v (ties to even): int / int is correctly rounded; beyond the
    largest double Python raises, where the device gives inf."""
    try:
        return v.numerator / v.denominator
    except OverflowError:
        return math.copysign(INF, v)


@pytest.mark.parametrize("a,b,kind", [(2.5, INF, "upper"), (-1e-3, INF, "upper"),
                                      (-INF, 0.7, "lower"), (-INF, -3e5, "lower"),
                                      (-INF, INF, "both"), (INF, 2.5, "upper"),
                                      (0.7, -INF, "lower"), (INF, -INF, "both")])
def test_range_map_rounds_every_operation_to_half_an_ulp(a, b, kind):
    """q = (1.0 - t) / t, x = end +- q and t * t, each the correctly rounded result of the exact
    operation on its (rounded) operands: no contraction, no reassociation. Half of the t lie
    below 0.5, where 1.0 - t is not exact."""
    m = native()
    assert m.adapt_range(a, b) == kind == aq.range_kind(a, b)
    t = _ts()
    assert (t < 0.5).sum() >= 300
    x, jac, x2 = m.adapt_range_map(a, b, t)
    end = b if math.isinf(a) else a
    inexact = 0
    for i, ti in enumerate(t):
        ft = Fraction(float(ti))
        s = _rn(1 - ft)
        inexact += Fraction(s) != 1 - ft
        q = _rn(Fraction(s) / ft)
        assert jac[i] == _rn(ft * ft)
        if kind == "both":
            assert x[i] == q and x2[i] == -q
        elif math.isinf(q):
            assert x[i] == (q if kind == "upper" else -q)
        else:
            want = Fraction(end) + Fraction(q) if kind == "upper" else Fraction(end) - Fraction(q)
            assert x[i] == _rn(want) and x2[i] == x[i]
    assert inexact >= 100
    assert np.array_equal(aq.t_to_x(a, b, t), x)


def test_range_map_of_a_finite_range_is_the_identity():
    m = native()
    t = _ts()
    x, jac, x2 = m.adapt_range_map(0.0, 3.0, t)
    assert np.array_equal(x, t) and np.array_equal(x2, t) and np.all(jac == 1.0)
    for a, b in ((1.0, 1.0), (INF, INF), (-INF, -INF), (0.0, 3.0), (float("nan"), INF)):
        assert m.adapt_range(a, b) == "finite" == aq.range_kind(a, b)


# ------------------------------------------------------------------ the model on the table
@pytest.mark.parametrize("panels", [ic.FEW_PANELS, ic.PANELS])
@pytest.mark.parametrize("rtol", ic.RTOLS)
@pytest.mark.parametrize("case", ic.TABLE, ids=repr)
def test_model_meets_the_truth_within_the_bound(case, rtol, panels):
    r = ic.model(case, rtol=rtol, panels=panels)
    err, bound = abs(r["value"] - case.truth), ic.value_bound(r, case)
    print(case, rtol, panels, {k: r[k] for k in COUNTS}, "err", err, "bound", bound,
          "measured/bound", err / bound, "C", case.conditioning)
    assert r["converged"] and not r["capped"] and r["nonfinite"] == 0
    assert err <= bound
    assert r["intervals"] == panels + r["splits"]
    assert r["evals"] == 15 * (r["intervals"] + r["splits"])
    assert r["range"] == aq.range_kind(case.a, case.b)
    if case is not ic.POWER:
        assert r["floor"] == 0 and r["forced"] == 0
    lo, hi = r["lo"], r["hi"]   # the partition of [0, 1] in t
    assert lo[0] == 0.0 and hi[-1] == 1.0 and np.array_equal(hi[:-1], lo[1:])


def test_model_figures_of_the_table():
    """Rounds and evaluations from 16 panels at rtol = 1e-10, on the project's node bits."""
    got = {c.name: (ic.model(c, rtol=1e-10, panels=16)["rounds"],
                    ic.model(c, rtol=1e-10, panels=16)["evals"]) for c in ic.TABLE}
    print(got)
    assert got["gauss"] == got["exp_upper"] == got["exp_lower"] == got["cauchy"] == (1, 240)
    assert got["cauchy_from_1"] == (1, 240) and got["gamma3"] == (2, 270)
    assert got["planck"] == (2, 300) and got["gauss_from_minus_2"] == (2, 300)
    assert got["gauss_at_50"] == (9, 780) and got["resonance_at_3"] == (13, 1380)
    assert got["x_to_minus_1.5"] == (61, 3600)
    p = ic.model(ic.POWER, rtol=1e-10, panels=16)
    assert p["floor"] >= 30 and p["forced"] == 2 and abs(p["value"] - 2.0) <= 2e-11
    big = max(ic.model(c, rtol=1e-10, panels=4096)["evals"] for c in ic.TABLE)
    assert big <= 70000


def test_model_honest_failures():
    r = ic.model(ic.DIVERGES, rtol=1e-10, panels=16)
    print({k: r[k] for k in COUNTS}, r["err_est"])
    assert not r["converged"] and r["rounds"] == 61 and 2 <= r["forced"] <= 3
    assert 1.0 <= r["err_est"] <= 3.0 and r["nonfinite"] == 0 and not r["capped"]
    r = ic.model(ic.END_SINGULAR, rtol=1e-6, panels=16)
    print({k: r[k] for k in COUNTS}, r["err_est"])
    assert not r["converged"] and r["nonfinite"] >= 1 and not r["capped"]
    assert 1e5 <= r["evals"] <= 1e6


def test_model_swapped_empty_and_finite_ranges():
    case = ic.EXP_UP
    fwd = ic.model(case, rtol=1e-10, panels=16)
    rev = ic.model(case, a=INF, b=0.0, rtol=1e-10, panels=16)
    assert rev["value"] == -fwd["value"] and rev["range"] == "upper"
    assert all(rev[k] == fwd[k] for k in COUNTS + ("err_est", "resabs", "tol"))
    both = ic.model(ic.GAUSS, a=INF, b=-INF, rtol=1e-10, panels=16)
    assert both["value"] == -ic.model(ic.GAUSS, rtol=1e-10, panels=16)["value"]
    for a in (INF, -INF, 2.0):
        z = aq.adaptive_model(case.f, a, a, unbounded=True)
        assert z["value"] == 0.0 and z["evals"] == 0 and z["converged"] and z["range"] == "finite"
    # unbounded = True with finite ends is the finite model, exactly
    for c in (ac.RESONANCE, ac.GAUSS3):
        one = aq.adaptive_model(c.f, c.a, c.b, rtol=1e-9, panels=32)
        two = aq.adaptive_model(c.f, c.a, c.b, rtol=1e-9, panels=32, unbounded=True)
        assert set(one) == set(two)
        for k in one:
            assert np.array_equal(one[k], two[k]), k


def test_t_to_x_gives_the_partition_in_x():
    r = ic.model(ic.GAUSS_M2, rtol=1e-10, panels=16)
    x = aq.t_to_x(-2.0, INF, r["hi"])
    assert x[-1] == -2.0 and np.all(np.diff(x) < 0)          # t = 1 is the finite end
    assert aq.t_to_x(-2.0, INF, r["lo"])[0] == INF           # t = 0 is infinity
    assert aq.t_to_x(-INF, 5.0, np.array([1.0, 0.5]))[1] == 4.0
    assert aq.t_to_x(-INF, INF, np.array([0.25]))[0] == 3.0


# ------------------------------------------------------------------ the sweep model
@pytest.mark.parametrize("fam", [ic.GAUSS_WIDTHS, ic.DECAYS], ids=repr)
def test_sweep_model_is_a_loop_of_the_one_integral_model(fam):
    sw = ic.sweep_model(fam, panels=16)
    assert sw["range"] == aq.range_kind(fam.a, fam.b)
    for k, row in enumerate(fam.rows):
        one = aq.adaptive_model(lambda x, row=row: fam.f(x, *row), fam.a, fam.b, panels=16,
                                max_intervals=sw["max_intervals"], unbounded=True)
        for key in aq.SWEEP_ROW_FIELDS:
            assert sw[key][k] == one[key], (k, key)
        assert sw["peak_row"][k] == one["peak"]
        err = abs(sw["value"][k] - fam.truths[k])
        print(fam, row, "err", err, "bound", ic.row_bound(sw, k, fam))
        assert sw["converged"][k] and err <= ic.row_bound(sw, k, fam)
    assert sw["call_rounds"] == int(sw["rounds"].max())
    assert sw["call_evals"] == int(sw["evals"].sum())
    rev = aq.adaptive_sweep_model(fam.f, fam.params, fam.b, fam.a, panels=16, unbounded=True)
    assert np.array_equal(rev["value"], -sw["value"])
    assert np.array_equal(rev["evals"], sw["evals"]) and rev["peak"] == sw["peak"]


# ------------------------------------------------------------------ refusals and defaults
def test_an_infinite_end_without_unbounded_is_refused_in_todays_words():
    m = native()
    full = dict(rtol=1e-10, atol=0.0, panels=16, max_depth=60, max_intervals=64)
    for a, b in ((0.0, INF), (-INF, 0.0), (-INF, INF), (INF, 0.0)):
        with pytest.raises(RuntimeError) as e:
            m.adapt_check(a, b, m.AdaptOptions(**full))
        with pytest.raises(ValueError) as v:
            aq.check_options(a, b, **full)
        tail = str(v.value)
        assert tail == f"adaptive: a = {a:.17g} and b = {b:.17g} must be finite, and b - a too"
        assert str(e.value).endswith(tail)
        m.adapt_check(a, b, m.AdaptOptions(unbounded=True, **full))
        aq.check_options(a, b, unbounded=True, **full)
        with pytest.raises(RuntimeError) as e:
            m.adapt_sweep_check(2, 1, 2, a, b, m.AdaptSweepOptions())
        with pytest.raises(ValueError) as v:
            aq.check_sweep_options(2, 1, 2, a, b)
        assert str(e.value).endswith(str(v.value)) and "must be finite" in str(v.value)
        used = m.adapt_sweep_check(2, 1, 2, a, b, m.AdaptSweepOptions(unbounded=True))
        assert used.unbounded and used.panels == 32768
        assert aq.check_sweep_options(2, 1, 2, a, b, unbounded=True)["panels"] == 32768
        with pytest.raises(ValueError, match="must be finite"):
            aq.adaptive_model(np.exp, a, b)
        with pytest.raises(ValueError, match="must be finite"):
            aq.adaptive_sweep_model(lambda x, p: p * x, [[1.0]], a, b)


def test_nan_and_overflowing_ends_are_refused_with_unbounded_too():
    m = native()
    nan = float("nan")
    for a, b in ((nan, 1.0), (0.0, nan), (nan, INF), (-INF, nan), (-1e308, 1e308)):
        with pytest.raises(RuntimeError) as e:
            m.adapt_check(a, b, m.AdaptOptions(unbounded=True))
        with pytest.raises(ValueError) as v:
            aq.check_options(a, b, **aq.DEFAULTS, unbounded=True)
        assert "must not be NaN, and b - a must be finite when both are" in str(v.value)
        assert str(e.value).replace("-nan", "nan").endswith(str(v.value))
        with pytest.raises(RuntimeError, match="must be finite"):
            m.adapt_check(a, b, m.AdaptOptions())
    # the other refusals are unchanged by the flag
    with pytest.raises(RuntimeError, match="rtol = 0 and atol = 0"):
        m.adapt_check(0.0, INF, m.AdaptOptions(rtol=0.0, unbounded=True))
    with pytest.raises(ValueError, match="panels = 65"):
        aq.check_options(0.0, INF, 1e-10, 0.0, 65, 60, 64, unbounded=True)


def test_the_low_layers_refuse_before_any_device_call_and_the_top_layer_sets_the_flag():
    from cuda_v_mpi_amd.ops import kernels

    with pytest.raises(RuntimeError, match="must be finite"):
        kernels.quad_expr("exp(-x)", 0.0, INF)
    with pytest.raises(RuntimeError, match="must be finite"):
        kernels.quad_expr_sweep("exp(-p0*x)", [[1.0]], 0.0, INF)
    with pytest.raises(RuntimeError, match="must not be NaN"):
        kernels.quad_expr("exp(-x)", 0.0, float("nan"), unbounded=True)
    with pytest.raises(RuntimeError, match="must not be NaN"):
        kernels.quad_expr_sweep("exp(-p0*x)", [[1.0]], float("nan"), INF, unbounded=True)


def test_defaults():
    m = native()
    assert m.AdaptOptions().unbounded is False and m.AdaptSweepOptions().unbounded is False
    o = m.AdaptOptions(1e-8, 0.0, 16, 60, 64, True)    # the flag is the last positional
    assert o.unbounded and o.max_intervals == 64
    s = m.AdaptSweepOptions(1e-8, 0.0, 16, 60, 64, 128, True)
    assert s.unbounded and s.max_total == 128
    assert m.AdaptSweepResult().range == "finite"
    import inspect

    for fn in (aq.adaptive_model, aq.adaptive_sweep_model, aq.check_options,
               aq.check_sweep_options):
        assert inspect.signature(fn).parameters["unbounded"].default is False
    from cuda_v_mpi_amd.ops import kernels

    for fn in (kernels.quad_expr, kernels.quad_expr_sweep):
        assert inspect.signature(fn).parameters["unbounded"].default is False


# ------------------------------------------------------------------ sources and compiles
def test_unbounded_sources_wrap_f_share_the_rule_and_compile_for_gfx950():
    m = native()
    expr = "x*x*x/expm1(x)"
    src = m.expr_adapt_unbounded_source(expr)
    for name in ("miint_adapt_eval_upper", "miint_adapt_eval_lower", "miint_adapt_eval_both"):
        assert f"void {name}(" in src
    assert f"double miint_user_f(double x) {{ return ({expr}); }}" in src
    assert "const double q = (1.0 - t) / t;" in src and "/ (t * t)" in src
    assert "end + q : end - q" in src and "miint_user_f(q) + miint_user_f(-q)" in src
    assert src.count("#pragma clang fp contract(off)") == 2     # the map and the rule
    rule = [l for l in m.expr_adapt_source(expr).splitlines() if l.lstrip().startswith("MIINT_GK_")]
    assert len(rule) == 8 and all(l in src for l in rule)       # the same table, the same order
    assert "atomic" not in src.lower() and "miint_adapt_init" not in src
    assert m.expr_adapt_unbounded_compile(expr)[:4] == b"\x7fELF"
    sw = m.expr_adapt_sweep_unbounded_source("1.0/((x-p0)*(x-p0)+p1)", 2)
    for name in ("miint_asweep_eval_upper", "miint_asweep_eval_lower", "miint_asweep_eval_both"):
        assert f"void {name}(" in sw
    assert "double miint_user_f(double x, double p0, double p1)" in sw
    assert "miint_user_f(q, p0, p1) + miint_user_f(-q, p0, p1)" in sw
    assert all(l in sw for l in rule) and "miint_asweep_row" not in sw
    assert m.expr_adapt_sweep_unbounded_compile("1.0/((x-p0)*(x-p0)+p1)", 2)[:4] == b"\x7fELF"
    assert m.expr_adapt_sweep_unbounded_compile("exp(-x*x)", 0)[:4] == b"\x7fELF"
    with pytest.raises(RuntimeError, match="p3"):
        m.expr_adapt_sweep_unbounded_compile("p3*x", 2)
    with pytest.raises(RuntimeError, match="rejected"):
        m.expr_adapt_unbounded_source("x; 1")
    with pytest.raises(RuntimeError, match="nparams = 9"):
        m.expr_adapt_sweep_unbounded_source("x", 9)


def test_the_finite_sources_do_not_know_the_map():
    """Finite calls compile and run the code they did: the existing sources carry none of the
    new text (their own tests hold the rest of them)."""
    m = native()
    for src in (m.expr_adapt_source("exp(-x*x)"), m.expr_adapt_sweep_source("exp(-p0*x*x)", 1)):
        for word in ("miint_user_f", "miint_g(", "miint_kind", "_upper", "_lower", "_both"):
            assert word not in src, word
        assert src.count("#pragma clang fp contract(off)") == 1
    one = m.expr_adapt_source("exp(-x*x)")
    assert "double miint_f(double x) { return (exp(-x*x)); }" in one
    assert one.count("extern \"C\" __global__") == 6


# ------------------------------------------------------------------ the cpu backend
def test_cpu_backend_runs_the_model_and_needs_no_flag():
    r = integrate_expr_adaptive("exp(-x*x)", -INF, INF, rtol=1e-10, panels=16, backend="cpu")
    want = ic.model(ic.GAUSS, rtol=1e-10, panels=16, max_intervals=1 << 22)
    assert isinstance(r, AdaptiveResult) and r.range == "both" and r.converged
    assert r.evals == want["evals"] and abs(r.value - math.sqrt(math.pi)) <= r.tol
    assert r.as_dict()["range"] == "both"
    assert integrate_expr_adaptive("exp(-x*x)", 0.0, 1.0, panels=16, backend="cpu").range == "finite"
    fam = ic.DECAYS
    s = integrate_expr_adaptive_sweep(fam.expr, fam.params, INF, 0.0, panels=16, backend="cpu")
    assert s.range == "upper" and s.converged.all()
    assert np.array_equal(s.value, -ic.sweep_model(fam, panels=16)["value"])


# ------------------------------------------------------------------ the CLIs
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def _py(*args):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300)


SPELLINGS = ["inf", "+inf", "-inf", "infinity", "INF", "-Infinity", "+INFINITY"]
NO_TOLERANCE = [
    (),
    ("--n", "1e6"),
    ("--rule", "mid"),
    ("--running", "--n", "1000"),
    ("--ya", "0", "--yb", "1"),
    ("--linspace", "p0=0:1:4"),
    ("--device", "cpu"),
]


@pytest.mark.parametrize("extra", NO_TOLERANCE, ids=[" ".join(e) or "plain" for e in NO_TOLERANCE])
def test_native_cli_refuses_an_infinite_end_without_a_tolerance(extra):
    for spelling in SPELLINGS:
        for ends in (("--a", "0", "--b", spelling), ("--a", spelling, "--b", "0")):
            p = _riemann("--expr", "exp(-x*x)", *ends, *extra)
            assert p.returncode == 1, (spelling, p.stdout, p.stderr)
            assert "an infinite range needs" in p.stderr and "--rtol / --atol" in p.stderr
            assert "--row-rtol / --row-atol" in p.stderr and spelling in p.stderr
    p = _riemann("--a", "0", "--b", "inf", "--rtol", "1e-8")     # a built-in integrand
    assert p.returncode == 1 and "--expr" in p.stderr


def test_native_cli_takes_an_infinite_end_with_a_tolerance_up_to_the_device():
    """Past every refusal: what stops the run here is the missing device, or nothing."""
    for tol in (("--rtol", "1e-8"), ("--atol", "1e-8"),
                ("--row-rtol", "1e-8", "--linspace", "p0=1:2:2")):
        p = _riemann("--expr", "exp(-x*x)", "--a", "-inf", "--b", "Infinity", *tol, "--json")
        assert "infinite range" not in p.stderr and "must be finite" not in p.stderr, p.stderr
        assert p.returncode == 0 or "HIP device" in p.stderr or "hip" in p.stderr.lower()
    p = _riemann("--expr", "exp(-x*x)", "--a", "nan", "--b", "inf", "--rtol", "1e-8")
    assert p.returncode == 1 and "must not be NaN" in p.stderr
    p = _riemann("--expr", "x", "--a", "-inf", "--b", "inf", "--rtol", "1e-8", "--n", "100")
    assert p.returncode == 1 and "--n does not go with them" in p.stderr
    p = _riemann("--help")
    assert p.returncode == 0
    for word in ("inf, +inf, -inf or infinity", "range: finite, upper, lower or both",
                 "|f(x) + f(-x)|", "split it at 1", "does not converge"):
        assert word in p.stdout, word


def test_python_cli_refuses_an_infinite_end_without_a_tolerance():
    for spelling in ("inf", "-inf", "+inf", "Infinity", "-INFINITY"):
        for extra in ((), ("--n", "1e6"), ("--linspace", "p0=0:1:4"), ("--ya", "0", "--yb", "1")):
            p = _py("--expr", "exp(-x*x)", "--a", "0", "--b", spelling, *extra)
            assert p.returncode != 0 and "an infinite range needs" in p.stderr, p.stderr
            assert "--rtol / --atol" in p.stderr and "--b" in p.stderr
    p = _py("--expr", "exp(-x*x)", "--a", "-inf", "--b", "0", "--box", "0:1", "--rtol", "1e-3")
    assert p.returncode != 0 and "infinite range" in p.stderr
    p = _py("--a", "-inf", "--rtol", "1e-8")                      # a built-in integrand
    assert p.returncode != 0 and "infinite range" in p.stderr
    p = _py("--expr", "x", "--a", "-inf", "--b", "inf", "--rtol", "1e-8", "--n", "100")
    assert p.returncode != 0 and "--n does not go with them" in p.stderr
    p = _py("--expr", "x", "--a", "nan", "--b", "inf", "--rtol", "1e-8")
    assert p.returncode != 0 and "must not be NaN" in p.stderr
    p = _py("--help")
    assert p.returncode == 0
    text = " ".join(p.stdout.split())
    for word in ("inf, +inf, -inf or infinity", "finite, upper, lower or both",
                 "|f(x) + f(-x)|", "split the range there", "does not converge"):
        assert word in text, word


def test_python_cli_json_spells_an_infinite_end():
    """--a -inf reaches argparse as a value, and the record stays json."""
    from cuda_v_mpi_amd.__main__ import _join_infinities, _json_ends

    assert _join_infinities(["integrate", "--a", "-inf", "--b", "+Infinity", "--n", "-3"]) == [
        "integrate", "--a=-inf", "--b=+Infinity", "--n", "-3"]
    rec = _json_ends(dict(a=-INF, b=INF, value=1.0))
    assert json.loads(json.dumps(rec, allow_nan=False)) == dict(a="-inf", b="inf", value=1.0)
