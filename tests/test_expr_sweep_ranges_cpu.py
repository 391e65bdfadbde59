"""CPU tests of per-row ranges in adaptive sweeps and of the running integral to a tolerance
(no GPU): the refusals of the checks and of the Python CLI with their messages, the ranges
source and its hipRTC compile for gfx950, the sources that must not move, the numpy models
against closed forms, the exact reference's prefix order against a plain loop, and
``backend="cpu"`` end to end. tests/test_riemann_ranges_cli_cpu.py has the native CLI."""
from __future__ import annotations

import hashlib
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_sweep_ranges_cases as rc
from cuda_v_mpi_amd import (CurveResult, integrate_expr_adaptive_sweep, integrate_expr_curve,
                            native)
from cuda_v_mpi_amd import __main__ as cli
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import adaptive_curve as acv
from cuda_v_mpi_amd.utils import adaptive_quad as aq

sc = rc.sc


# ------------------------------------------------------------------ the ranged check
def _opts(**kw):
    return native().AdaptSweepOptions(**kw)


RANGED_REFUSALS = [
    (dict(a=[0.0], b=[1.0, 2.0]), {}, "1 lower and 2 upper ends for 2 rows"),
    (dict(a=[0.0, 0.0, 0.0], b=[1.0, 1.0, 1.0]), {}, "3 lower and 3 upper ends for 2 rows"),
    ({}, dict(unbounded=True), "per-row ranges are finite: unbounded takes one shared range"),
    (dict(b=[1.0, float("inf")]), {}, "row 1: a = 0 and b = inf must be finite, and b - a too"),
    (dict(a=[float("nan"), 0.0]), {}, "row 0: a = nan and b = 1 must be finite"),
    (dict(a=[0.0, -1.5e308], b=[1.0, 1.5e308]), {}, "row 1: a = -1.5e\\+308 and b = 1.5e\\+308"),
    ({}, dict(rtol=0.0), "rtol = 0 and atol = 0 must be finite and >= 0, and not both 0"),
    ({}, dict(panels=65, max_intervals=64), "panels = 65 must be 1..max_intervals = 64"),
    ({}, dict(max_intervals=1 << 22), "rows \\* max_intervals = 2 \\* 4194304 passes max_total"),
    ({}, dict(max_total=0), "max_total = 0 must be 1..2\\^26"),
    ({}, dict(max_depth=201), "max_depth = 201 must be 0..200"),
]


@pytest.mark.parametrize("ends,opts,message", RANGED_REFUSALS, ids=[m[:24] for *_, m in
                                                                   RANGED_REFUSALS])
def test_the_ranged_check_refuses_in_the_shared_checks_words(ends, opts, message):
    m = native()
    a, b = ends.get("a", [0.0, 0.0]), ends.get("b", [1.0, 1.0])
    with pytest.raises(RuntimeError, match="adaptive( sweep)?: .*" + message):
        m.adapt_sweep_ranges_check(2, 1, 2, a, b, _opts(**opts))
    if len(a) == len(b) == 2:   # the numpy model words it alike, and nothing reaches a device
        with pytest.raises(ValueError, match="adaptive( sweep)?: .*" + message):
            aq.check_sweep_ranges(2, 1, 2, a, b, **opts)
        if "unbounded" not in opts:
            with pytest.raises(RuntimeError, match=message):
                kernels.quad_expr_sweep("x*p0", [[1.0], [2.0]], a, b, **opts)


def test_the_ranged_check_resolves_like_the_shared_one_and_takes_every_order_of_ends():
    m = native()
    o = m.adapt_sweep_ranges_check(5, 2, 10, [1.0, 0.0, 0.5, -1.0, 0.0], [0.0, 1.0, 0.5, 1.0, 2.0],
                                   _opts())
    s = m.adapt_sweep_check(5, 2, 10, 0.0, 1.0, _opts())
    assert (o.panels, o.max_intervals) == (s.panels, s.max_intervals) == (8192, (1 << 22) // 5)
    assert m.adapt_sweep_ranges_check(0, 2, 0, [], [], _opts()).panels == 65536
    with pytest.raises(RuntimeError, match="rows = 1048577 must be 0..2\\^20"):
        m.adapt_sweep_ranges_check(1048577, 0, 0, [0.0] * 1048577, [1.0] * 1048577, _opts())
    with pytest.raises(RuntimeError, match="3 parameter values for 2 rows of 1"):
        m.adapt_sweep_ranges_check(2, 1, 3, [0.0, 0.0], [1.0, 1.0], _opts())


# ------------------------------------------------------------------ the curve's check
CURVE_REFUSALS = [
    ([0.0], {}, "1 points: the grid must hold 2..2\\^20 \\+ 1"),
    ([0.0, 1.0, 1.0, 0.5], {}, "x\\[2\\] = 1 after x\\[1\\] = 1: the grid must be strictly"),
    ([0.0, 1.0, 0.5, 2.0], {}, "x\\[2\\] = 0.5 after x\\[1\\] = 1"),
    ([1.0, 0.5, 0.75], {}, "x\\[2\\] = 0.75 after x\\[1\\] = 0.5"),
    ([0.0, 0.0], {}, "x\\[1\\] = 0 after x\\[0\\] = 0"),
    ([0.0, float("nan"), 1.0], {}, "x\\[1\\] = nan must be finite"),
    ([0.0, 1.0, float("inf")], {}, "x\\[2\\] = inf must be finite"),
    ([-1.5e308, 1.5e308], {}, "x\\[M\\] - x\\[0\\] must be finite"),
    ([0.0, 1.0], dict(unbounded=True), "the grid is finite: unbounded is refused"),
]


@pytest.mark.parametrize("x,opts,message", CURVE_REFUSALS, ids=[m[:20] for *_, m in
                                                               CURVE_REFUSALS])
def test_the_curves_check_names_the_first_offending_index(x, opts, message):
    with pytest.raises(RuntimeError, match="adaptive curve: .*" + message):
        native().adapt_curve_check(x, _opts(**opts))
    if not opts:
        with pytest.raises(ValueError, match="adaptive curve: .*" + message):
            aq.check_curve(x)
        with pytest.raises(RuntimeError, match=message):    # before any device call
            kernels.quad_expr_curve("x", x)


def test_the_curves_defaults_and_its_capacity_check():
    m = native()
    for cells, panels in ((1, 65536), (2, 32768), (100, 512), (65536, 1), (65537, 1),
                          (1 << 20, 1)):
        x = np.arange(cells + 1, dtype=np.float64)
        o = m.adapt_curve_check(x, _opts())
        assert (o.panels, o.max_intervals) == (panels, (1 << 22) // cells), cells
        assert aq.check_curve(x) == dict(panels=panels, max_intervals=(1 << 22) // cells)
    x = np.arange(1001, dtype=np.float64)
    with pytest.raises(RuntimeError, match="rows \\* max_intervals = 1000 \\* 5000 passes"):
        m.adapt_curve_check(x, _opts(max_intervals=5000))
    with pytest.raises(RuntimeError, match="max_total = 134217728 must be 1..2\\^26"):
        m.adapt_curve_check(x, _opts(max_total=1 << 27))
    with pytest.raises(RuntimeError, match="panels = 64 must be 1..max_intervals = 32"):
        m.adapt_curve_check(x, _opts(max_total=32000))
    with pytest.raises(ValueError, match="1-D"):
        kernels.quad_expr_curve("x", [[0.0, 1.0]])
    assert m.ADAPT_CURVE_MAX_CELLS == 1 << 20


def test_atol_is_dealt_by_length_in_the_documented_order():
    x = rc.prefix_grid(40)
    want = [(1e-9 * abs(float(x[c + 1]) - float(x[c]))) / abs(float(x[-1]) - float(x[0]))
            for c in range(40)]
    for got in (native().adapt_curve_atol(x, 1e-9), acv.curve_atol(x, 1e-9),
                aq.curve_atol(x, 1e-9), native().adapt_curve_atol(x[::-1].copy(), 1e-9)[::-1]):
        assert [rc.bits(v) for v in got] == [rc.bits(v) for v in want]
    assert abs(sum(want) - 1e-9) <= 1e-23


# ------------------------------------------------------------------ source and compile
# sha256 of the generated sources at the parent commit
PINNED = {
    ("expr_adapt_sweep_source", ("1.0/((x-p0)*(x-p0)+p1)", 2)):
        "5ae2f0a2ad7f83bbddbd8eae6d47239de8064a8decd6a5a103b72e23b62ee44e",
    ("expr_adapt_sweep_source", ("x", 0)):
        "94ac2e607c5af8641f0301f4ef2d45f17f7eceefaf74a91ad15404014282769d",
    ("expr_adapt_sweep_source", ("exp(-p0*x*x)", 1)):
        "ff2693cc56f57013e151fd0141417a6e502594342321f59f1827cab82dd1f2d7",
    ("expr_adapt_sweep_unbounded_source", ("exp(-p0*x*x)", 1)):
        "26f2b540feef7a854b5fb97719ba5f6770f78456e60acfc9b141b3f629f052cd",
    ("expr_adapt_source", ("exp(-x*x)",)):
        "e3078d7ab02b908a8f7aae72496f04e48ee9c3d49ba8b9c1c482e018c275e74a",
}


def test_the_ranges_source_compiles_for_gfx950_and_the_pinned_sources_do_not_move():
    m = native()
    src = m.expr_adapt_sweep_ranges_source()
    names = ("miint_asweep_init_ranges", "miint_asweep_row_ranges", "miint_acurve_prefix")
    for name in names:
        assert f"void {name}(" in src
    assert "atomic" not in src.lower() and "miint_f" not in src
    code = m.expr_adapt_sweep_ranges_compile()
    assert isinstance(code, bytes) and code[:4] == b"\x7fELF"
    for name in names:
        assert name.encode() in code
    for (fn, args), want in PINNED.items():
        assert hashlib.sha256(getattr(m, fn)(*args).encode()).hexdigest() == want, (fn, args)


def test_the_twin_row_kernel_is_the_row_kernels_text():
    """Between its parameters and its end the twin differs from miint_asweep_row in one line:
    the loads of the row's width and atol."""
    m = native()

    def body(src, name):
        text = src[src.index(f"void {name}("):]
        text = text[text.index(") {\n") + 4:]
        return text[:text.index("\n}\n")].splitlines()

    one = body(m.expr_adapt_sweep_source("x", 0), "miint_asweep_row")
    twin = body(m.expr_adapt_sweep_ranges_source(), "miint_asweep_row_ranges")
    extra = [l for l in twin if l not in one]
    assert extra == ["  const double width = width_of[row], atol = atol_of[row];"]
    assert [l for l in twin if l in one] == one
    init = body(m.expr_adapt_sweep_source("x", 0), "miint_asweep_init")
    twin = body(m.expr_adapt_sweep_ranges_source(), "miint_asweep_init_ranges")
    assert [l for l in twin if l not in init] == ["  const double a = lo_of[r], b = hi_of[r];"]
    assert [l for l in twin if l in init] == init


# ------------------------------------------------------------------ the numpy models
def test_the_ranged_model_meets_the_closed_forms_row_by_row():
    case = rc.LORENTZ16
    r = rc.model(case)
    for k, (p0, p1) in enumerate(case.fam.rows):
        s = math.sqrt(p1)
        truth = (math.atan((case.b[k] - p0) / s) - math.atan((case.a[k] - p0) / s)) / s
        assert r["converged"][k] and abs(r["value"][k] - truth) <= 4e-10 * abs(truth), k
    one = aq.adaptive_sweep_model(case.fam.f, case.fam.params[[1]], case.a[1], case.b[1],
                                  **case.args)
    for key in aq.SWEEP_ROW_FIELDS:   # a row is the shared-range model of that row alone
        assert r[key][1] == one[key][0], key
    mixed = rc.model(rc.MIXED)
    assert mixed["value"][2] == 0.0 and mixed["evals"][2] == 0 and mixed["converged"][2]
    assert mixed["value"][1] == -rc.model(rc.LORENTZ16)["value"][1] or mixed["value"][1] < 0
    assert mixed["call_rounds"] == int(mixed["rounds"].max())
    assert mixed["call_evals"] == int(mixed["evals"].sum())


def test_the_curve_model_meets_erf_a_kink_and_an_endpoint_singularity():
    r = aq.adaptive_curve_model(lambda t: np.exp(-t * t), rc.ERF_GRID)
    assert r["converged"].all() and r["value"][0] == 0.0
    for j, t in enumerate(rc.ERF_TRUTH):
        assert abs(r["value"][j] - t) <= max(r["tol"][j], r["err_est"][j]) + 98 * rc.U * \
            r["resabs"][j], j
    assert np.all(r["tol"][1:] <= 1.0000001e-10 * r["resabs"][1:])
    r = aq.adaptive_curve_model(lambda t: np.abs(t - 0.3), rc.KINK_GRID, panels=4)
    assert [abs(v - rc.kink_truth(x)) <= 1e-15 for x, v in zip(rc.KINK_GRID, r["value"])]
    assert r["cells"]["rounds"].tolist()[0] == 1 < r["cells"]["rounds"][1]
    r = aq.adaptive_curve_model(lambda t: 1.0 / np.sqrt(t), rc.RSQRT_GRID, panels=16)
    assert np.abs(r["value"] - 2.0 * np.sqrt(rc.RSQRT_GRID)).max() <= 2e-10
    assert r["cells"]["rounds"][0] == 61 and (r["cells"]["rounds"][1:] == 1).all()
    down = aq.adaptive_curve_model(lambda t: np.exp(-t * t), rc.ERF_GRID[::-1].copy())
    assert (down["value"][1:] < 0).all() and abs(down["total"] + r["total"] * 0
                                                  + rc.ERF_TRUTH[-1]) <= 1e-10
    bad = aq.adaptive_curve_model(lambda t: 1.0 / (t - 0.5), [0.0, 0.125, 0.25, 0.75, 1.0],
                                  panels=1, max_intervals=64)
    assert bad["converged"].tolist() == [True, True, True, False, False]


# ------------------------------------------------------------------ the exact reference
def test_the_prefix_order_against_a_plain_loop():
    rng = np.random.default_rng(7)
    for m in (1, 2, 255, 256, 257, 513, 1000):
        v = rng.standard_normal(m) * 10.0 ** rng.integers(-8, 8, m)
        per = (m + 255) // 256
        want, prefix = [0.0], 0.0
        for t in range(256):
            chain = 0.0
            for c in range(min(t * per, m), min((t + 1) * per, m)):
                chain += float(v[c])
                want.append(prefix + chain)
            prefix += chain
        got = acv.curve_prefix_exact(v)
        assert [rc.bits(g) for g in got] == [rc.bits(w) for w in want], m
        if per == 1:   # one chain
            assert [rc.bits(g) for g in got[1:]] == [rc.bits(w) for w in np.cumsum(v)]
    v = rng.standard_normal(513)
    assert [rc.bits(g) for g in acv.curve_prefix_exact(v, per_of=lambda n: 4)] != \
        [rc.bits(g) for g in acv.curve_prefix_exact(v)]
    nan = v.copy()
    nan[300] = np.nan
    got = acv.curve_prefix_exact(nan)
    assert np.isnan(got[301:]).all() and [rc.bits(g) for g in got[:301]] == \
        [rc.bits(g) for g in acv.curve_prefix_exact(v)[:301]]
    assert acv.curve_unconverged_exact([True, False, True]).tolist() == [0, 0, 1, 1]


def test_the_exact_reference_composes_the_call_from_the_rows():
    case = rc.EXACT_CASES[0]
    want = rc.exact(case)
    ec = rc.ec
    for k in (1, 4):   # a row is adaptive_sweep_exact of that row alone on its range
        one = ec.ax.adaptive_sweep_exact(ec.F[case.expr], case.params[k:k + 1], case.a[k],
                                         case.b[k], **case.opts)
        assert rc.row(want, k) == rc.row(one, 0)
        assert want["row_lengths"][k] == one["lengths"]
    assert case.a[4] > case.b[4] and want["value"][4] == -acv.sweep_ranges_exact(
        ec.F[case.expr], case.params[4:5], [case.b[4]], [case.a[4]], **case.opts)["value"][0]
    assert want["row_lengths"][5] == [] and want["evals"][5] == 0
    assert want["lengths"][0] == 6 * 150 and want["peak"] == max(want["lengths"])
    assert want["call_rounds"] == int(want["rounds"].max()) == len(want["lengths"])
    assert want["call_evals"] == int(want["evals"].sum())
    # the shared range given per row is the shared-range reference
    shared = ec.reference(ec.SWEEP)
    rows = [3, 10, ec.HARD_ROW]
    per_row = acv.sweep_ranges_exact(ec.F[ec.KINK], np.array(ec.SWEEP.params)[rows],
                                     [0.0] * 3, [1.0] * 3, **ec.SWEEP.opts)
    for i, k in enumerate(rows):
        assert rc.row(per_row, i) == rc.row(shared, k)
    cv = acv.curve_exact(ec.F[ec.ZIG], [0.0, 0.25, 0.5, 1.0], rtol=1e-7, atol=1e-9, panels=3,
                         max_intervals=1 << 12)
    assert [rc.bits(v) for v in cv["value"]] == \
        [rc.bits(v) for v in acv.curve_prefix_exact(cv["cells"]["value"])]
    assert [rc.bits(v) for v in cv["atol_cell"]] == [rc.bits(v) for v in (2.5e-10, 2.5e-10, 5e-10)]


# ------------------------------------------------------------------ the cpu backend
def test_cpu_backend_end_to_end():
    case = rc.LORENTZ16
    r = integrate_expr_adaptive_sweep(case.fam.expr, case.fam.params, case.a, case.b,
                                      backend="cpu", **case.args)
    want = rc.model(case)
    assert r.backend == "cpu" and r.converged.all() and r.range == "finite"
    assert r.evals.tolist() == want["evals"].tolist() and r.peak == want["peak"]
    assert r.a.tolist() == case.a and r.b.tolist() == case.b
    same = integrate_expr_adaptive_sweep(case.fam.expr, case.fam.params, -1.0,
                                         np.full(5, 1.0), backend="cpu", panels=16)
    shared = integrate_expr_adaptive_sweep(case.fam.expr, case.fam.params, -1.0, 1.0,
                                           backend="cpu", panels=16)
    assert same.value.tolist() == shared.value.tolist()
    c = integrate_expr_curve("exp(-x*x)", rc.ERF_GRID, backend="cpu")
    assert isinstance(c, CurveResult) and c.backend == "cpu" and c.converged.all()
    assert abs(c.total - rc.ERF_TRUTH[-1]) <= 1e-10 and c.value.shape == (101,)
    assert c.cells["evals"].shape == (100,) and c.call_evals == int(c.cells["evals"].sum())
    assert c.as_dict()["expr"] == "exp(-x*x)"
    with pytest.raises(ValueError, match="backend must be"):
        integrate_expr_curve("x", [0.0, 1.0], backend="host")
    with pytest.raises(ValueError, match="strictly increasing or strictly decreasing"):
        integrate_expr_curve("x", [0.0, 1.0, 1.0], backend="cpu")


# ------------------------------------------------------------------ the Python CLI
def _py(*args, env=None):
    """``python -m cuda_v_mpi_amd integrate`` in this process: the exit code or message, and
    nothing has run when it is a message."""
    old = dict(os.environ)
    os.environ.update(env or {})
    try:
        return cli.main(["integrate", *args])
    except SystemExit as e:
        return e.code
    finally:
        os.environ.clear()
        os.environ.update(old)


CURVE = ("--expr", "exp(-x*x)", "--curve-rtol", "1e-9", "--a", "0", "--b", "3", "--points", "10")
CURVE_WHO = "--curve-rtol / --curve-atol"
CURVE_CONFLICTS = [
    (("--n", "1e6"), "--n"), (("--rule", "mid"), "--rule"), (("--rtol", "1e-8"), "--rtol"),
    (("--atol", "1e-8"), "--atol"), (("--row-rtol", "1e-8"), "--row-rtol"),
    (("--row-atol", "1e-8"), "--row-atol"), (("--area-rtol", "1e-8"), "--area-rtol"),
    (("--ya", "0", "--yb", "1"), "--ya"), (("--box", "0:1,0:1"), "--box"),
    (("--osc", "cos", "--omega", "3"), "--osc"), (("--params", "rows.txt"), "--params"),
    (("--linspace", "p0=0:1:4"), "--linspace"), (("--ranges", "r.txt"), "--ranges"),
    (("--device", "cpu"), "--device cpu"), (("--backend", "host"), "--backend host"),
    (("--m", "12"), "--m"),
]


@pytest.mark.parametrize("extra,named", CURVE_CONFLICTS, ids=[n for _, n in CURVE_CONFLICTS])
def test_python_cli_refuses_the_curve_flags_with_another_modes(extra, named):
    msg = _py(*CURVE, *extra)
    assert isinstance(msg, str) and named in msg, msg
    assert CURVE_WHO in msg or "--box" in msg, msg


def test_python_cli_refuses_bad_grids_ranks_and_infinite_ends(tmp_path):
    msg = _py(*CURVE, env=dict(WORLD_SIZE="2", RANK="0"))
    assert "WORLD_SIZE = 2" in msg and CURVE_WHO in msg
    assert "--expr" in _py("--curve-rtol", "1e-9", "--a", "0", "--b", "1", "--points", "4")
    assert "need a grid" in _py("--expr", "x", "--curve-rtol", "1e-9", "--a", "0", "--b", "1")
    assert "need a grid" in _py("--expr", "x", "--curve-atol", "1e-9", "--points", "4")
    assert "infinite end" in _py("--expr", "x", "--curve-rtol", "1e-9", "--a", "0", "--b", "inf",
                                 "--points", "4")
    assert "infinite end" in _py("--expr", "x", "--curve-rtol", "1e-9", "--a", "-inf", "--b",
                                 "0", "--points", "4")
    assert "--points 0 must be at least 1" in _py("--expr", "x", "--curve-rtol", "1e-9", "--a",
                                                  "0", "--b", "1", "--points", "0")
    assert "they need --curve-rtol / --curve-atol" in _py("--expr", "x", "--a", "0", "--b", "1",
                                                          "--points", "4")
    grid = tmp_path / "grid.txt"
    grid.write_text("# a grid\n0\n0.5\n\n0.25\n1\n")
    at = ("--expr", "x", "--curve-rtol", "1e-9", "--at", str(grid))
    assert "x[2] = 0.25 after x[1] = 0.5" in _py(*at)
    assert "--at FILE is the whole grid" in _py(*at, "--a", "0")
    assert "--at FILE is the whole grid" in _py(*at, "--points", "3")
    grid.write_text("0\n0.5 0.75\n")
    assert "line 2: expected `x`" in _py(*at)
    grid.write_text("0\ninf\n")
    assert "x[1] = inf must be finite" in _py(*at)
    assert "No such file" in _py("--expr", "x", "--curve-rtol", "1e-9", "--at",
                                 str(tmp_path / "none.txt"))
    assert "rtol = 0 and atol = 0" in _py("--expr", "x", "--curve-rtol", "0", "--a", "0", "--b",
                                          "1", "--points", "4")
    msg = _py("--expr", "x", "--curve-rtol", "1e-9", "--a", "1", "--b", "1", "--points", "4")
    assert "x[1] = 1 after x[0] = 1" in msg


SWEEP = ("--expr", "1.0/((x-p0)*(x-p0)+1e-6)", "--linspace", "p0=-0.5:0.7:4")


def test_python_cli_refuses_ranges_with_a_shared_range_or_without_a_row_tolerance(tmp_path):
    ranges = tmp_path / "ranges.txt"
    ranges.write_text("-1 0\n-0.5 0.5\n# the third\n0 1\n1 0.25\n")
    tol = ("--row-rtol", "1e-8")
    for ends in (("--a", "-1"), ("--b", "1"), ("--a", "-1", "--b", "1")):
        msg = _py(*SWEEP, *tol, "--ranges", str(ranges), *ends)
        assert "--ranges gives every row its own a and b: --a / --b do not go with it" in msg
    for other in ((), ("--rtol", "1e-8"), ("--n", "1e6")):
        msg = _py(*SWEEP, "--ranges", str(ranges), *other)
        assert "--ranges" in msg and "it needs --row-rtol R / --row-atol T" in msg
    ranges.write_text("-1 0\n-0.5 0.5\n0 1\n")
    assert "3 ranges for 4 rows" in _py(*SWEEP, *tol, "--ranges", str(ranges))
    ranges.write_text("-1 0\n-0.5 0.5\n0 1 2\n1 0\n")
    assert "line 3: expected `a b`" in _py(*SWEEP, *tol, "--ranges", str(ranges))
    ranges.write_text("-1 0\n-0.5 0.5\n0 inf\n1 0\n")
    assert "row 2: a = 0 and b = inf must be finite" in _py(*SWEEP, *tol, "--ranges", str(ranges))
    assert "No such file" in _py(*SWEEP, *tol, "--ranges", str(tmp_path / "none.txt"))


def test_python_cli_keeps_its_old_refusals():
    msg = _py("--expr", "x", "--a", "0", "--b", "1", "--rtol", "1e-8", "--linspace", "p0=0:1:4")
    assert "--rtol / --atol choose the samples themselves" in msg and "--linspace" in msg
    msg = _py(*SWEEP, "--a", "-1", "--b", "1", "--row-rtol", "1e-8", "--n", "1e6")
    assert "--row-rtol / --row-atol choose the samples themselves: --n" in msg
    msg = _py(*SWEEP, "--a", "-1", "--b", "1", "--max-total", "4096")
    assert "--max-total belongs to --row-rtol / --row-atol" in msg
    msg = _py("--expr", "x", "--a", "0", "--b", "inf")
    assert "an infinite range needs --expr with --rtol" in msg
