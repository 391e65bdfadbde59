"""CPU tests of adaptive sweeps (ExprAdaptiveSweep, csrc/runtime/expr_adaptive_sweep.cpp): the
numpy model against a loop of the one-integral model, every refusal with its wording (native and
numpy), the derived defaults, the generated source and its gfx950 compile, the cpu backend and
both CLIs' conflict tables. No device is touched."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive_sweep_cases as sc
from cuda_v_mpi_amd import AdaptiveSweepResult, integrate_expr_adaptive_sweep, native
from cuda_v_mpi_amd.utils import adaptive_quad as aq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("fam", [sc.LORENTZ, sc.KINK, sc.STEP, sc.COS], ids=repr)
def test_model_is_a_loop_of_the_one_integral_model(fam):
    args = {**dict(panels=16), **fam.args}
    got = sc.model(fam, **args)
    for k, row in enumerate(fam.rows):
        one = aq.adaptive_model(lambda x, row=row: fam.f(x, *row), fam.a, fam.b,
                                rtol=args.get("rtol", 1e-10), panels=args["panels"],
                                max_intervals=got["max_intervals"])
        for key in aq.SWEEP_ROW_FIELDS:
            assert got[key][k] == one[key], (key, k)
        assert got["peak_row"][k] == one["peak"]
        assert abs(got["value"][k] - fam.truths[k]) <= sc.value_bound(got, k)
    assert got["call_rounds"] == got["rounds"].max()
    assert got["call_evals"] == got["evals"].sum()
    assert got["peak_row"].max() <= got["peak"] <= got["peak_row"].sum()


def test_model_reproduces_the_table_of_the_cases():
    """The intervals / rounds every row was laid out for (rtol = 1e-10 from 16 panels; the
    cosine rows from one panel at 1e-9)."""
    m = sc.model(sc.LORENTZ, panels=16)
    assert list(m["intervals"]) == sc.LORENTZ_MODEL_INTERVALS
    assert list(m["rounds"]) == [13, 19, 2, 1, 9]
    m = sc.model(sc.KINK, panels=16)
    assert list(m["intervals"]) == [38, 16, 40, 32] and list(m["rounds"]) == [23, 1, 25, 17]
    m = sc.model(sc.STEP, panels=16)
    assert list(m["intervals"]) == [66, 16, 65] and list(m["rounds"]) == [51, 1, 50]
    m = sc.model(sc.COS)
    assert list(m["intervals"]) == [1, 16, 64, 1011] and list(m["rounds"]) == [1, 5, 7, 11]
    assert m["peak_row"][3] == 998 and m["converged"].all() and not m["capped"].any()
    m = sc.model(sc.SQRT_SHIFT, panels=16)
    assert list(m["nonfinite"]) == sc.SQRT_SHIFT_NONFINITE and list(m["rounds"]) == [1, 1, 1]
    assert m["converged"].tolist() == [True, False, False]


def test_model_empty_cases_and_reversed_range():
    fam = sc.LORENTZ
    z = aq.adaptive_sweep_model(fam.f, fam.params, 0.25, 0.25)
    assert z["value"].tolist() == [0.0] * 5 and z["converged"].all() and z["call_evals"] == 0
    e = aq.adaptive_sweep_model(fam.f, [], -1.0, 1.0)
    assert e["value"].shape == (0,) and e["call_rounds"] == 0 and e["peak"] == 0
    fwd = aq.adaptive_sweep_model(fam.f, fam.params, -1.0, 0.5, rtol=1e-8, panels=16)
    rev = aq.adaptive_sweep_model(fam.f, fam.params, 0.5, -1.0, rtol=1e-8, panels=16)
    assert np.array_equal(rev["value"], -fwd["value"])
    assert np.array_equal(rev["err_est"], fwd["err_est"])


def test_model_caps_a_row_alone():
    wide = sc.model(sc.LORENTZ, panels=16, max_intervals=256)
    capped = sc.model(sc.LORENTZ, panels=16, max_intervals=32)
    assert capped["capped"].tolist() == [n > 32 for n in sc.LORENTZ_MODEL_INTERVALS]
    assert (capped["intervals"] <= 32).all()
    for k in (2, 3):
        for key in aq.SWEEP_ROW_FIELDS:
            assert capped[key][k] == wide[key][k]


# ------------------------------------------------------------------ defaults
DEFAULT_PANELS = {1: 65536, 2: 32768, 3: 16384, 4096: 16, 4097: 16, 1 << 20: 16}


def test_derived_defaults_at_the_row_counts_where_they_change():
    m = native()
    assert m.adapt_sweep_default_panels(2048) == 32 and aq.sweep_default_panels(2048) == 32
    for rows, panels in DEFAULT_PANELS.items():
        assert m.adapt_sweep_default_panels(rows) == panels == aq.sweep_default_panels(rows)
        max_total = 1 << 24 if rows > 4096 else 1 << 22
        opt = m.AdaptSweepOptions(max_total=max_total)
        used = m.adapt_sweep_check(rows, 1, rows, 0.0, 1.0, opt)
        assert used.panels == panels and used.max_intervals == max_total // rows
        res = aq.check_sweep_options(rows, 1, rows, 0.0, 1.0, max_total=max_total)
        assert res == dict(panels=panels, max_intervals=max_total // rows)
    o = m.AdaptSweepOptions()
    assert (o.rtol, o.atol, o.panels, o.max_depth, o.max_intervals, o.max_total) == (
        1e-10, 0.0, 0, 60, 0, 1 << 22)
    assert aq.SWEEP_DEFAULTS == dict(rtol=1e-10, atol=0.0, panels=0, max_depth=60,
                                     max_intervals=0, max_total=1 << 22)
    assert m.ADAPT_SWEEP_MAX_TOTAL_LIMIT == 1 << 26 and m.ADAPT_SWEEP_INITIAL_TOTAL == 65536
    assert m.ADAPT_SWEEP_MIN_PANELS == 16
    # 2^20 rows of 16 panels do not fit the default capacity: said up front, with the numbers
    with pytest.raises(RuntimeError, match=r"panels = 16 must be 1\.\.max_intervals = 4 \(per"):
        m.adapt_sweep_check(1 << 20, 0, 0, 0.0, 1.0, m.AdaptSweepOptions())


# ------------------------------------------------------------------ refusals
# (rows, nparams, param_count, options) -> the words both checks use
BAD = [
    ((1 << 20) + 1, 0, 0, {}, "rows = 1048577 must be 0..2^20"),
    (4, 9, 36, {}, "nparams = 9 must be 0..8"),
    (4, 2, 7, {}, "7 parameter values for 4 rows of 2"),
    (4, 1, 4, dict(max_total=0), "max_total = 0 must be 1..2^26"),
    (4, 1, 4, dict(max_total=(1 << 26) + 1), "max_total = 67108865 must be 1..2^26"),
    (4, 1, 4, dict(panels=65, max_intervals=64),
     "panels = 65 must be 1..max_intervals = 64 (per row)"),
    (4, 1, 4, dict(max_total=32), "panels = 16384 must be 1..max_intervals = 8 (per row)"),
    (4, 1, 4, dict(max_intervals=1 << 21),
     "rows * max_intervals = 4 * 2097152 passes max_total = 4194304"),
    (3, 1, 3, dict(panels=4, max_intervals=6, max_total=17),
     "rows * max_intervals = 3 * 6 passes max_total = 17"),
    (4, 1, 4, dict(rtol=0.0, atol=0.0), "rtol = 0 and atol = 0"),
    (4, 1, 4, dict(rtol=-1e-6), "rtol = -"),
    (4, 1, 4, dict(atol=float("nan")), "atol = nan"),
    (4, 1, 4, dict(max_depth=-1), "max_depth = -1"),
    (4, 1, 4, dict(max_depth=201), "max_depth = 201"),
]


@pytest.mark.parametrize("rows,nparams,count,opts,message", BAD, ids=[b[-1] for b in BAD])
def test_refusals_name_the_numbers(rows, nparams, count, opts, message):
    m = native()
    full = dict(aq.SWEEP_DEFAULTS, **opts)
    o = m.AdaptSweepOptions(full["rtol"], full["atol"], full["panels"], full["max_depth"],
                            full["max_intervals"], full["max_total"])
    with pytest.raises(RuntimeError) as e:
        m.adapt_sweep_check(rows, nparams, count, 0.0, 1.0, o)
    assert message in str(e.value) and "adaptive" in str(e.value)
    with pytest.raises(ValueError) as e:   # the model's check refuses the same, in the same words
        aq.check_sweep_options(rows, nparams, count, 0.0, 1.0, **full)
    assert message in str(e.value)


def test_refusals_reach_the_python_entry_points_before_any_device_call():
    from cuda_v_mpi_amd.ops import kernels

    params = sc.LORENTZ.params
    for opts, message in ((dict(panels=65, max_intervals=64), "panels = 65"),
                          (dict(max_intervals=1 << 21), "passes max_total"),
                          (dict(rtol=0.0), "rtol = 0 and atol = 0")):
        with pytest.raises(RuntimeError, match=message):
            kernels.quad_expr_sweep(sc.LORENTZ.expr, params, -1.0, 1.0, **opts)
        with pytest.raises(ValueError, match=message):
            aq.adaptive_sweep_model(sc.LORENTZ.f, params, -1.0, 1.0, **opts)
    with pytest.raises(RuntimeError, match="must be finite"):
        kernels.quad_expr_sweep(sc.LORENTZ.expr, params, 0.0, float("inf"))
    with pytest.raises(ValueError, match="2-D"):
        kernels.quad_expr_sweep(sc.LORENTZ.expr, [1.0, 2.0], -1.0, 1.0)
    m = native()
    m.adapt_sweep_check(5, 2, 10, 1.0, 0.0, m.AdaptSweepOptions())   # a > b and a == b are ranges
    m.adapt_sweep_check(0, 2, 0, 1.0, 1.0, m.AdaptSweepOptions())    # no rows is a sweep


# ------------------------------------------------------------------ source and compile
def test_source_shares_the_rule_and_compiles_for_gfx950_without_a_device():
    m = native()
    src = m.expr_adapt_sweep_source(sc.LORENTZ.expr, 2)
    for name in ("miint_asweep_init", "miint_asweep_eval", "miint_asweep_row",
                 "miint_asweep_prefix", "miint_asweep_scatter"):
        assert f"void {name}(" in src
    one = m.expr_adapt_source("exp(-x*x)")
    rule = [l for l in one.splitlines() if l.lstrip().startswith("MIINT_GK_")]
    assert len(rule) == 8 and all(l in src for l in rule)       # the same table, the same order
    assert "double miint_f(double x, double p0, double p1)" in src
    assert "atomic" not in src.lower()
    code = m.expr_adapt_sweep_compile(sc.LORENTZ.expr, 2)
    assert isinstance(code, bytes) and code[:4] == b"\x7fELF"
    assert m.expr_adapt_sweep_compile("exp(-x*x)", 0)[:4] == b"\x7fELF"
    with pytest.raises(RuntimeError, match="p3"):
        m.expr_adapt_sweep_compile("p3*x", 2)
    with pytest.raises(RuntimeError, match="nparams = 9"):
        m.expr_adapt_sweep_source("x", 9)
    with pytest.raises(RuntimeError, match="rejected"):
        m.expr_adapt_sweep_source("x; p0", 1)


# ------------------------------------------------------------------ the cpu backend
def test_cpu_backend_runs_the_model_on_expr_torch():
    fam = sc.LORENTZ
    r = integrate_expr_adaptive_sweep(fam.expr, fam.params, fam.a, fam.b, panels=16,
                                      backend="cpu")
    assert isinstance(r, AdaptiveSweepResult) and r.backend == "cpu" and r.converged.all()
    want = sc.model(fam, panels=16)
    assert r.evals.tolist() == want["evals"].tolist() and r.call_rounds == want["call_rounds"]
    assert r.peak == want["peak"] and r.call_evals == want["call_evals"]
    for k in range(5):
        assert abs(r.value[k] - fam.truths[k]) <= sc.value_bound(r, k)
    assert r.as_dict()["expr"] == fam.expr
    r = integrate_expr_adaptive_sweep("p0*exp(-x*x)", [[1.0], [-2.0]], 3.0, 0.0, atol=1e-12,
                                      rtol=0.0, panels=8, backend="cpu")
    assert r.converged.all() and abs(r.value[1] / r.value[0] + 2.0) <= 4e-12   # 3 atol / |value|
    with pytest.raises(ValueError, match="backend must be"):
        integrate_expr_adaptive_sweep("x*p0", [[1.0]], 0.0, 1.0, backend="host")
    with pytest.raises(ValueError, match="cpu backend"):
        integrate_expr_adaptive_sweep("(x<p0)?1.0:0.0", [[0.3]], 0.0, 1.0, backend="cpu")


# ------------------------------------------------------------------ the CLIs
def _riemann(*args, env=None):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def _py(*args, env=None):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300, env=env)


BASE = ("--expr", "1.0/((x-p0)*(x-p0)+1e-6)", "--a", "-1", "--b", "1", "--linspace",
        "p0=-0.5:0.7:4")
WHO = "--row-rtol / --row-atol"
CONFLICTS = [
    (("--n", "1e6"), "--n"),
    (("--rule", "mid"), "--rule"),
    (("--running",), "--running"),
    (("--ya", "0", "--yb", "1"), "--ya"),
    (("--gpus", "2"), "--gpus 2"),
    (("--loopback", "2"), "--loopback"),
    (("--device", "cpu"), "--device cpu"),
    (("--box", "0:1,0:1"), "--box"),
    (("--rtol", "1e-8"), "--rtol / --atol do not go"),
    (("--atol", "1e-8"), "--rtol / --atol do not go"),
]


@pytest.mark.parametrize("extra,named", CONFLICTS, ids=[n for _, n in CONFLICTS])
def test_native_cli_names_the_conflict(extra, named):
    for tol in (("--row-rtol", "1e-8"), ("--row-atol", "1e-8")):
        p = _riemann(*BASE, *tol, *extra)
        assert p.returncode == 1 and WHO in p.stderr and named in p.stderr, p.stderr


def test_native_cli_refuses_ranks_missing_rows_bad_numbers_and_stray_bounds():
    tol = ("--row-rtol", "1e-8")
    p = _riemann(*BASE, *tol, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode == 1 and "WORLD_SIZE = 2" in p.stderr and WHO in p.stderr
    p = _riemann("--expr", "x", "--a", "0", "--b", "1", *tol)
    assert p.returncode == 1 and "need the rows of --params FILE or --linspace" in p.stderr
    p = _riemann("--row-rtol", "1e-8", "--device", "cpu", "--n", "1e4")
    assert p.returncode == 1 and "--expr" in p.stderr
    for flag, value, word in (("--row-rtol", "1e-8x", "--row-rtol must be a number"),
                              ("--row-atol", "small", "--row-atol must be a number"),
                              ("--panels", "12.5", "--panels must be a whole number"),
                              ("--max-total", "1e7.", "--max-total must be")):
        other = ("--row-atol", "1e-3") if flag == "--row-rtol" else ("--row-rtol", "1e-8")
        p = _riemann(*BASE, *other, flag, value)
        assert p.returncode == 1 and word in p.stderr, (flag, p.stderr)
    p = _riemann(*BASE, "--row-rtol", "0")
    assert p.returncode == 1 and "rtol = 0 and atol = 0" in p.stderr
    p = _riemann(*BASE, *tol, "--panels", "65", "--max-intervals", "64")
    assert p.returncode == 1 and "panels = 65 must be 1..max_intervals = 64" in p.stderr
    p = _riemann(*BASE, *tol, "--max-intervals", "2097152")
    assert p.returncode == 1 and "passes max_total = 4194304" in p.stderr
    # the knobs without a tolerance do not run the fixed-n sweep instead
    p = _riemann(*BASE, "--max-total", "4096")
    assert p.returncode == 1 and "--max-total belongs to --row-rtol / --row-atol" in p.stderr
    p = _riemann(*BASE, "--panels", "64")
    assert p.returncode == 1 and "belong to --rtol / --atol" in p.stderr
    p = _riemann("--help")
    assert p.returncode == 0 and "--row-rtol R" in p.stdout and "--max-total N" in p.stdout


def test_the_old_refusal_of_rtol_with_rows_is_unchanged():
    for extra, named in ((("--params", "rows.txt"), "--params"),
                         (("--linspace", "p0=0:1:4"), "--linspace")):
        p = _riemann("--expr", "x", "--a", "0", "--b", "1", "--rtol", "1e-8", *extra)
        assert p.returncode == 1 and named in p.stderr
        assert "--rtol / --atol choose the samples themselves" in p.stderr
        p = _py("--expr", "x", "--a", "0", "--b", "1", "--rtol", "1e-8", *extra)
        assert p.returncode != 0 and named in p.stderr
        assert "--rtol / --atol choose the samples themselves" in p.stderr


def test_python_cli_names_the_conflict():
    tol = ("--row-rtol", "1e-8")
    for extra, named in ((("--n", "1e6"), "--n"), (("--rule", "mid"), "--rule"),
                         (("--ya", "0", "--yb", "1"), "--ya"),
                         (("--box", "0:1,0:1"), "--box"),
                         (("--device", "cpu"), "--device cpu"),
                         (("--backend", "host"), "--backend host"),
                         (("--rtol", "1e-8"), "--rtol / --atol do not go"),
                         (("--atol", "1e-8"), "--rtol / --atol do not go")):
        p = _py(*BASE, *tol, *extra)
        assert p.returncode != 0 and WHO in p.stderr and named in p.stderr, p.stderr
    p = _py(*BASE, *tol, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode != 0 and "WORLD_SIZE = 2" in p.stderr
    p = _py("--expr", "x", *tol)
    assert p.returncode != 0 and "need the rows of --params FILE or --linspace" in p.stderr
    p = _py(*tol)
    assert p.returncode != 0 and "--expr" in p.stderr
    p = _py(*BASE, "--max-total", "4096")
    assert p.returncode != 0 and "--max-total belongs to --row-rtol / --row-atol" in p.stderr
    p = _py(*BASE, "--panels", "64")
    assert p.returncode != 0 and "belong to --rtol / --atol" in p.stderr
    p = _py(*BASE, "--row-rtol", "0")
    assert p.returncode != 0 and "rtol = 0 and atol = 0" in p.stderr
    p = _py(*BASE, *tol, "--panels", "65", "--max-intervals", "64")
    assert p.returncode != 0 and "panels = 65 must be 1..max_intervals = 64" in p.stderr
