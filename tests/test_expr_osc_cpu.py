"""CPU tests of the oscillatory integrator (ExprAdaptiveOsc, csrc/runtime/expr_adaptive_osc.cpp):
the Filon-Clenshaw-Curtis weights against 50-digit values, the rule's exactness, the numpy model
(utils/adaptive_osc.py) against mpmath truths on every case the GPU tests use, what the rule
buys over Gauss-Kronrod on the typed product, the Fourier tail, every refusal of the Python
layer and of both CLIs, and the generated sources. No device needed."""
from __future__ import annotations

import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_osc_cases as oc
from cuda_v_mpi_amd import OscillatoryResult, integrate_expr_oscillatory, native
from cuda_v_mpi_amd.utils import adaptive_osc as ao
from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest absolute error of osc_weights measured on the development host over
# oc.WEIGHT_PARS and their negatives was 2.64e-17 (at par = 1e-8; half an ulp of the largest
# weights). The bound is 4 x that, for another host's libm, and must stay below 2^-48.
WEIGHT_ERR_MEASURED = 2.64e-17
WEIGHT_BOUND = 4.0 * WEIGHT_ERR_MEASURED


# ------------------------------------------------------------------ the weights
@pytest.mark.parametrize("par", oc.WEIGHT_PARS, ids=lambda p: f"{p:g}")
def test_weights_against_mpmath(par):
    """osc_weights(par) and osc_weights(-par) against 50-digit integrals of the Lagrange basis
    times cos and sin. Measured largest absolute error: 2.64e-17; the bound is 4 x that (1.06e-16)
    and, as a condition, never above 2^-48 = 3.55e-15. Mirror symmetry is exact."""
    import mpmath as mp

    assert WEIGHT_BOUND <= 2.0 ** -48
    m = native()
    worst = 0.0
    for sign in (1.0, -1.0):
        got = m.osc_weights(sign * par)
        for n, gc, gs in ((24, got[0], got[1]), (12, got[2], got[3])):
            wc, ws = oc.weights_mp(par, n)
            assert gc.shape == gs.shape == (n + 1,)
            for j in range(n + 1):
                worst = max(worst, float(abs(mp.mpf(float(gc[j])) - wc[j])),
                            float(abs(mp.mpf(float(gs[j])) - sign * ws[j])))
            assert np.array_equal(gc, gc[::-1])             # Wc_j == Wc_{n-j}, exactly
            assert np.array_equal(gs, -gs[::-1]) and gs[n // 2] == 0.0
    print(f"par {par:g}: largest absolute error {worst:.3e}")
    assert worst <= WEIGHT_BOUND


def test_weights_par_zero_are_clenshaw_curtis():
    import mpmath as mp

    m = native()
    wc24, ws24, wc12, ws12 = m.osc_weights(0.0)
    assert not ws24.any() and not ws12.any()
    for n, got in ((24, wc24), (12, wc12)):
        want = oc.weights_mp(0.0, n)[0]
        for j in range(n + 1):
            assert abs(float(got[j]) - float(want[j])) <= 2 * np.spacing(float(want[j]))
    # the printed table: the correctly rounded doubles
    with mp.workdps(60):
        assert [float(mp.cos(j * mp.pi / 24)) for j in range(12)] == list(m.osc_nodes()[:12])
        assert m.osc_nodes()[12] == 0.0 and np.array_equal(m.osc_nodes(), -m.osc_nodes()[::-1])
        assert [float(w) for w in oc.weights_mp(0.0, 24)[0]] == list(m.osc_cc_weights())
    row = m.osc_table_row(0.5)
    w = m.osc_weights(0.5)
    assert row.shape == (m.OSC_ROW,)
    assert np.array_equal(row[:13], w[0][:13]) and np.array_equal(row[13:25], w[1][:12])
    assert np.array_equal(row[25:32], w[2][:7]) and np.array_equal(row[32:38], w[3][:6])
    with pytest.raises(RuntimeError, match="par = nan must be finite"):
        m.osc_weights(float("nan"))


def test_abscissae_are_the_fma_nodes():
    m = native()
    lo, hi = np.array([0.3, -2.0, 1e-9]), np.array([1.7, 5.0, 3.0])
    x = m.osc_abscissae(lo, hi)
    hw = 0.5 * (hi - lo)
    c = lo + hw
    t = m.osc_nodes()
    for j in range(25):
        assert np.array_equal(x[:, j], m.fma(hw, t[j], c))


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize("omega", [0.0, 3.0, 300.0])
@pytest.mark.parametrize("kind", ["cos", "sin"])
def test_polynomials_to_degree_12_are_exact(omega, kind):
    """For f of degree <= 12 both interpolants are f, so K == G up to rounding: 25 products a
    sum, each weight within 2^-54 of its value and each fma within 2^-53 of the sum so far, in
    two rules: |K - G| <= 64 * 2^-53 * hw * max |f(x_j)| with room. Degree 14 misses it by
    orders of magnitude, so the bound is not vacuous."""
    lo, hi = np.array([0.3]), np.array([1.7])
    table = ao._Table(omega * 0.5 * (hi[0] - lo[0]))
    depth = np.zeros(1, dtype=np.int64)

    def run(f):
        k, err, r = ao.osc_rule(f, lo, hi, depth, omega, kind, table)
        x = native().osc_abscissae(lo, hi)
        return float(err[0]), 0.5 * (hi[0] - lo[0]) * float(np.abs(f(x)).max())

    for deg in range(13):
        err, scale = run(lambda x, d=deg: (x - 0.8) ** d + 0.25 * x)
        assert err <= 64 * 2.0 ** -53 * scale, (deg, err, scale)
    err, scale = run(lambda x: (x - 0.8) ** 14)
    if not (kind == "sin" and omega == 0.0):     # sin at omega 0 is 0 whatever f is
        assert err > 1e4 * 64 * 2.0 ** -53 * scale


# ------------------------------------------------------------------ the model against truth
# The one combination that does not end `converged`: from 4 panels, par is 12500 and the rule's
# |K25 - K13| of about 1.5e-17 an interval is below the floor 50 * 2^-52 * R (R, the integral of
# |f|, does not shrink with omega), so four intervals are accepted as rounding noise and err_est
# 5.96e-17 stays above tol = 1e-10 * 3.5e-8 = 3.5e-18. The value is right all the same: true
# error 4.0e-21. From 64 panels the same case converges in one round.
FLOOR_BOUND = {("lorentz-cos-w10000", 4)}


@pytest.mark.parametrize("panels", oc.PANELS)
@pytest.mark.parametrize("case", oc.FINITE, ids=lambda c: c.id)
def test_model_against_truth(case, panels):
    r = ao.osc_model(oc.f_numpy(case.expr), case.a, case.b, case.omega, case.kind,
                     rtol=case.rtol, atol=case.atol, panels=panels)
    truth = oc.truth(case)
    print(f"{case.id} from {panels}: error {abs(r['value'] - truth):.3e} tol {r['tol']:.3e} "
          f"err_est {r['err_est']:.3e} rounds {r['rounds']} evals {r['evals']} {r['reason']}")
    assert abs(r["value"] - truth) <= r["tol"]
    assert r["evals"] == 25 * sum(r["lengths"]) and r["omega"] == case.omega
    if (case.id, panels) in FLOOR_BOUND:
        assert not r["converged"] and r["floor"] > 0
        assert r["reason"].startswith("the rounding floor was reached on")
    else:
        assert r["converged"] and r["reason"] == ""


def test_lorentz_closed_form_against_quadrature():
    import mpmath as mp

    for w in (1.0, 50.0):
        for kind, osc in (("cos", mp.cos), ("sin", mp.sin)):
            with mp.workdps(30):
                q = mp.quad(lambda x: osc(w * x) / (1 + x * x), mp.linspace(0, 10, int(10 * w) + 9))
            assert abs(oc.lorentz_truth(10.0, w, kind) - float(q)) <= 1e-15 * abs(float(q))


def test_gpu_cases_are_clear_of_their_thresholds():
    """What the GPU tests compare structurally must not hang on a rounding: every decision of
    every omega != 0 case, with the options used on the device, is further than 1e-6 relative
    from its threshold. A kink and an end root run past depth 20 of the weight table (the peak
    stops at depth 7 from 4 panels)."""
    deepest = 0
    for case in oc.FINITE:
        for panels in oc.PANELS:
            r = ao.osc_model(oc.f_numpy(case.expr), case.a, case.b, case.omega, case.kind,
                             rtol=case.rtol, atol=case.atol, panels=panels, max_intervals=4096)
            assert not r["capped"]
            if case.omega != 0.0:
                assert r["margin"] > 1e-6, (case.id, panels, r["margin"])
            deepest = max(deepest, r["max_depth_seen"])
    assert deepest > 20


@pytest.mark.parametrize("kind", ["cos", "sin"])
@pytest.mark.parametrize("panels", oc.PANELS)
def test_what_the_rule_buys(kind, panels):
    """omega = 1e4 on [0, 10]: at most 1/50 of the evaluations the model of ExprAdaptive spends
    on the typed product with the same options. Measured: cos 475 636 x from 4 panels and
    59 454 x from 64; sin 94 685 x and 8 876 x."""
    osc = np.cos if kind == "cos" else np.sin
    gk = adaptive_model(lambda x: osc(1e4 * x) / (1.0 + x * x), 0.0, 10.0, rtol=1e-10,
                        panels=panels)
    r = ao.osc_model(oc.f_numpy(oc.LORENTZ), 0.0, 10.0, 1e4, kind, rtol=1e-10, panels=panels)
    print(f"{kind} from {panels}: Gauss-Kronrod {gk['evals']} evals, oscillatory {r['evals']}: "
          f"{gk['evals'] / r['evals']:.0f} x")
    assert 50 * r["evals"] <= gk["evals"]


def test_model_small_properties():
    f = oc.f_numpy(oc.LORENTZ)
    up = ao.osc_model(f, 0.0, 10.0, 50.0, "sin", panels=4)
    down = ao.osc_model(f, 10.0, 0.0, 50.0, "sin", panels=4)
    assert down["value"] == -up["value"] and down["err_est"] == up["err_est"]
    assert np.array_equal(down["partition"], up["partition"][::-1, ::-1])
    assert up["partition"][0, 0] == 0.0 and up["partition"][-1, 1] == 10.0
    assert np.array_equal(up["partition"][1:, 0], up["partition"][:-1, 1])
    same = ao.osc_model(f, 2.0, 2.0, 50.0, "cos")
    assert same["value"] == 0.0 and same["rounds"] == 0 and same["converged"]
    minus = ao.osc_model(f, 0.0, 10.0, -50.0, "sin", panels=4)      # sin is odd in omega
    assert minus["value"] == pytest.approx(-up["value"], rel=1e-13)
    end = ao.osc_model(lambda x: 1.0 / np.sqrt(x), 0.0, 1.0, 10.0, "cos", panels=4)
    assert end["nonfinite"] == 1 and not end["converged"]
    assert end["reason"].startswith("f was not finite on 1 intervals")


# ------------------------------------------------------------------ the Fourier tail
@pytest.mark.parametrize("case", oc.TAILS, ids=lambda c: c.id)
def test_tail_model_against_truth(case):
    r = ao.osc_tail_model(oc.f_numpy(case.expr), case.a, case.omega, case.kind, atol=case.atol)
    truth = oc.tail_truth(case)
    print(f"{case.id}: error {abs(r['value'] - truth):.3e} err_est {r['err_est']:.3e} cycles "
          f"{r['cycles']} extrapolated {r['extrapolated']}")
    assert r["converged"] and r["reason"] == "" and r["range"] == "upper"
    assert abs(r["value"] - truth) <= case.atol
    assert r["err_est"] <= case.atol and 3 <= r["cycles"] <= 50


def test_tail_of_a_constant_says_it_does_not_converge():
    c = oc.DIVERGENT
    r = ao.osc_tail_model(oc.f_numpy(c.expr), c.a, c.omega, c.kind, atol=c.atol)
    assert not r["converged"] and r["reason"].startswith("no decay")
    short = ao.osc_tail_model(oc.f_numpy("1.0/x"), 1.0, 1.0, "sin", atol=1e-10, max_cycles=6)
    assert not short["converged"] and short["cycles"] == 6
    assert short["reason"].startswith("max_cycles = 6")


def test_epsilon_algorithm():
    m = native()
    s = np.cumsum([(-1.0) ** k / (k + 1) for k in range(12)])       # log 2
    # the twelfth partial sum is 4e-2 off; the extrapolation a million times closer
    assert abs(m.osc_epsilon(s) - math.log(2.0)) < 1e-6 * abs(s[-1] - math.log(2.0))
    assert m.osc_epsilon(np.array([1.0, 1.0, 1.0])) == 1.0
    with pytest.raises(RuntimeError, match="at least 3"):
        m.osc_epsilon(np.array([1.0, 2.0]))


# ------------------------------------------------------------------ refusals, Python
def _osc(*args, **kw):
    return integrate_expr_oscillatory(*args, backend="cpu", **kw)


@pytest.mark.parametrize("args, kw, message", [
    (("x", 0.0, 1.0, float("nan")), {}, "omega = nan must be finite"),
    (("x", 0.0, 1.0, float("inf")), {}, "omega = inf must be finite"),
    (("x", 0.0, float("inf"), 1.0), {"rtol": 1e-8}, "the Fourier tail needs atol > 0"),
    (("x", 0.0, float("inf"), 0.0), {"atol": 1e-8}, "omega = 0 with an infinite end"),
    (("x", float("-inf"), 1.0, 1.0), {"atol": 1e-8}, "only (a, +inf) with a finite is supported"),
    (("x", 0.0, float("-inf"), 1.0), {"atol": 1e-8}, "only (a, +inf) with a finite is supported"),
    (("x", 0.0, float("inf"), 1.0), {"atol": 1e-8, "max_cycles": 0}, "max_cycles = 0 must be"),
    (("x", 0.0, 1.0, 1.0), {"rtol": 0.0}, "must be finite and >= 0, and not both 0"),
    (("x", 0.0, float("nan"), 1.0), {}, "must be finite, and b - a too"),
    (("x", 0.0, 1.0, 1.0), {"panels": 0}, "panels = 0 must be 1..max_intervals"),
    (("x", 0.0, 1.0, 1.0, "tan"), {}, "kind 'tan' must be cos or sin"),
])
def test_python_refusals(args, kw, message):
    with pytest.raises(ValueError) as e:
        _osc(*args, **kw)
    assert message in str(e.value)
    with pytest.raises(ValueError, match="backend must be 'hip' or 'cpu'"):
        integrate_expr_oscillatory("x", 0.0, 1.0, 1.0, backend="host")


def test_native_refusals_need_no_device():
    m = native()
    opt = m.AdaptOptions(rtol=1e-8)
    with pytest.raises(RuntimeError, match="omega = nan must be finite"):
        m.osc_check(0.0, 1.0, float("nan"), opt)
    with pytest.raises(RuntimeError, match="b = inf is the Fourier tail"):
        m.osc_check(0.0, float("inf"), 1.0, opt)
    with pytest.raises(RuntimeError, match="needs atol > 0"):
        m.osc_check(0.0, float("inf"), 1.0, opt, True)
    m.osc_check(0.0, float("inf"), 1.0, m.AdaptOptions(rtol=0.0, atol=1e-9), True)
    with pytest.raises(RuntimeError, match="rejected|not allowed|expression"):
        m.expr_osc_source("x; y")


def test_cpu_backend_result():
    r = _osc(oc.LORENTZ, 0.0, 10.0, 1e4, "sin", panels=64)
    assert isinstance(r, OscillatoryResult) and r.backend == "cpu" and r.converged
    assert abs(r.value - oc.lorentz_truth(10.0, 1e4, "sin")) <= r.tol
    assert (r.omega, r.kind, r.cycles, r.extrapolated, r.reason) == (1e4, "sin", 0, False, "")
    assert r.evals == 1600 and set(r.as_dict()) >= {"omega", "kind", "cycles", "reason"}
    t = _osc("exp(-x)", 0.0, float("inf"), 10.0, "cos", atol=1e-10, rtol=0.0)
    assert t.converged and t.range == "upper" and t.cycles >= 3
    assert abs(t.value - 1.0 / 101.0) <= 1e-10


# ------------------------------------------------------------------ the CLIs
def _riemann(*args, env=None):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def _py(*args, env=None):
    """``python -m cuda_v_mpi_amd integrate`` in this process: (exit status or message, stdout)."""
    import contextlib
    import io

    from cuda_v_mpi_amd.__main__ import main

    old = dict(os.environ)
    os.environ.update(env or {})
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            status = main(["integrate", *args])
    except SystemExit as e:
        status = e.code
    finally:
        os.environ.clear()
        os.environ.update(old)
    return status, out.getvalue()


WHO = "--osc / --omega"
X = ("--expr", "1.0/(1.0+x*x)", "--a", "0", "--b", "10")
OSC = X + ("--osc", "cos", "--omega", "50", "--rtol", "1e-10")
CONFLICTS = [(("--n", "1000"), "--n"), (("--rule", "mid"), "--rule"), (("--ya", "0"), "--ya"),
             (("--y-lo", "0.0"), "--y-lo"), (("--box", "0:1"), "--box"),
             (("--params", "rows.txt"), "--params"), (("--linspace", "p0=0:1:3"), "--linspace"),
             (("--row-rtol", "1e-8"), "--row-rtol"), (("--area-rtol", "1e-8"), "--area-rtol")]


@pytest.mark.parametrize("extra, flag", CONFLICTS + [(("--running",), "--running"),
                                                     (("--loopback", "2"), "--loopback")],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_riemann_refuses_what_belongs_elsewhere(extra, flag):
    r = _riemann(*OSC, *extra)
    assert r.returncode != 0
    assert f"{WHO} integrate one f(x) against one weight to a tolerance: {flag} does not go" \
        in r.stderr


def test_riemann_refusals():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    for args, message, e in [
            (X + ("--osc", "cos", "--rtol", "1e-8"), "--osc needs --omega W", None),
            (X + ("--omega", "3", "--rtol", "1e-8"), "--omega belongs to --osc cos|sin", None),
            (X + ("--osc", "cos", "--omega", "3"), f"{WHO} integrate to a tolerance: they need "
             "--rtol R / --atol T", None),
            (OSC + ("--gpus", "2"), f"{WHO} run on one GPU: --gpus 2", None),
            (OSC, "a rank environment (WORLD_SIZE = 2)", env),
            (OSC + ("--device", "cpu"), f"{WHO} have no host engine: --device cpu", None),
            (("--expr", "x", "--a", "-inf", "--b", "1", "--osc", "cos", "--omega", "1", "--atol",
              "1e-8"), "(-inf, b) and two-sided Fourier integrals are not supported", None),
            (("--expr", "x", "--a", "0", "--b", "inf", "--osc", "cos", "--omega", "1", "--rtol",
              "1e-8"), "the Fourier tail (--b inf) needs --atol T", None),
            (("--expr", "x", "--a", "0", "--b", "inf", "--osc", "cos", "--omega", "0", "--atol",
              "1e-8"), "omega = 0 with an infinite end is not supported", None),
            (OSC + ("--max-cycles", "9"), "--max-cycles bounds the Fourier tail", None),
            (X + ("--osc", "cos", "--omega", "nan", "--rtol", "1e-8"),
             "--omega must be a number", None),
            (X + ("--osc", "tan", "--omega", "1", "--rtol", "1e-8"),
             "kind 'tan' must be cos or sin", None),
            (("--osc", "cos", "--omega", "1", "--rtol", "1e-8"), "--expr is missing", None)]:
        r = _riemann(*args, env=e)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert "--osc cos|sin --omega W" in _riemann("--help").stdout


@pytest.mark.parametrize("extra, flag", CONFLICTS, ids=lambda v: v if isinstance(v, str) else "")
def test_python_cli_refuses_what_belongs_elsewhere(extra, flag):
    status, _ = _py(*OSC, *extra)
    assert f"{WHO} integrate one f(x) against one weight to a tolerance: {flag} does not go" \
        in str(status)


def test_python_cli_refusals():
    for args, message, env in [
            (X + ("--osc", "cos", "--rtol", "1e-8"), "--osc needs --omega W", None),
            (X + ("--omega", "3", "--rtol", "1e-8"), "--omega belongs to --osc cos|sin", None),
            (X + ("--osc", "cos", "--omega", "3"), f"{WHO} integrate to a tolerance: they need "
             "--rtol R / --atol T", None),
            (OSC, "a rank environment (WORLD_SIZE = 2)", {"WORLD_SIZE": "2"}),
            (OSC + ("--device", "cpu"), f"{WHO} have no host engine: --device cpu", None),
            (("--expr", "x", "--a=-inf", "--b", "1", "--osc", "cos", "--omega", "1", "--atol",
              "1e-8"), "(-inf, b) and two-sided Fourier integrals are not supported", None),
            (("--expr", "x", "--a", "0", "--b", "inf", "--osc", "cos", "--omega", "1", "--rtol",
              "1e-8"), "the Fourier tail (--b inf) needs --atol T", None),
            (("--expr", "x", "--a", "0", "--b", "inf", "--osc", "cos", "--omega", "0", "--atol",
              "1e-8", "--backend", "cpu"), "omega = 0 with an infinite end is not supported",
             None),
            (X + ("--osc", "cos", "--omega", "nan", "--rtol", "1e-8", "--backend", "cpu"),
             "omega = nan must be finite", None),
            (OSC + ("--max-cycles", "9"), "--max-cycles bounds the Fourier tail", None),
            (("--osc", "cos", "--omega", "1", "--rtol", "1e-8"), "--expr is missing", None)]:
        status, _ = _py(*args, env=env)
        assert message in str(status), (args, status)


def test_python_cli_runs_the_model():
    status, out = _py(*X, "--osc", "sin", "--omega", "1e4", "--rtol", "1e-10", "--panels", "64",
                      "--backend", "cpu", "--json")
    rec = json.loads(out)
    assert status == 0 and rec["converged"] and rec["kind"] == "sin" and rec["omega"] == 1e4
    assert abs(rec["value"] - oc.lorentz_truth(10.0, 1e4, "sin")) <= rec["tol"]
    assert {"cycles", "extrapolated", "reason", "value_bits", "evals"} <= set(rec)
    status, out = _py("--expr", "exp(-x)", "--a", "0", "--b", "inf", "--osc", "cos", "--omega",
                      "10", "--atol", "1e-10", "--backend", "cpu", "--json")
    rec = json.loads(out)
    assert status == 0 and rec["converged"] and rec["b"] == "inf" and rec["cycles"] >= 3
    assert abs(rec["value"] - 1.0 / 101.0) <= 1e-10


# ------------------------------------------------------------------ the generated sources
# sha256 of expr_adapt_source(expr) at the parent commit
PARENT_SOURCE = {
    "x*x": "ca26d41f87ad937687b5f0459894980042bfd95db481c7b76134ba18b1300ed9",
    "1.0/(1.0+x*x)": "ef736b23c68839fe1639946e0eb79de34faa3626fdb8c049747a6f372c2cb6d3",
    "exp(-x*x)": "e3078d7ab02b908a8f7aae72496f04e48ee9c3d49ba8b9c1c482e018c275e74a",
}


def test_finite_sources_are_the_parents():
    m = native()
    for expr, want in PARENT_SOURCE.items():
        m.expr_osc_source(expr)
        assert hashlib.sha256(m.expr_adapt_source(expr).encode()).hexdigest() == want
    src = m.expr_osc_source("exp(-x*x)")
    assert "miint_osc_eval_cos" in src and "miint_osc_eval_sin" in src
    assert "fp contract(off)" in src and "miint_adapt_decide" not in src
    assert "osc" not in m.expr_adapt_source("exp(-x*x)")


def test_twins_compile_without_scratch():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from expr_adaptive2d_probe import kernel_resources

    code = native().expr_osc_compile(oc.PEAK)
    for name in ("miint_osc_eval_cos", "miint_osc_eval_sin"):
        res = kernel_resources(code, name)
        print(name, res)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0
        assert res["vgpr_count"] <= 128
