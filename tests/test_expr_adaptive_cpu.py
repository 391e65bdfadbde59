"""CPU tests of adaptive integration (ExprAdaptive, csrc/runtime/expr_adaptive.cpp): the rule's
constants against a 70-digit derivation, the numpy model of the rule on every case the GPU
tests use, the generated source and its gfx950 compile, every refusal, the CLIs' conflicts and
the cpu backend. No device needed."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive_cases as ac
from cuda_v_mpi_amd import AdaptiveResult, integrate_expr_adaptive, native
from cuda_v_mpi_amd.utils import adaptive_quad as aq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the constants
def _moment(k):
    return mp.mpf(0) if k % 2 else mp.mpf(2) / (k + 1)


def _weights(nodes):
    """The weights that integrate x^0 .. x^(len - 1) exactly on these nodes."""
    n = len(nodes)
    v, rhs = mp.matrix(n, n), mp.matrix(n, 1)
    for k in range(n):
        for j in range(n):
            v[k, j] = nodes[j] ** k
        rhs[k] = _moment(k)
    w = mp.lu_solve(v, rhs)
    return [w[j] for j in range(n)]


@pytest.fixture(scope="module")
def derived():
    """(K15 nodes, K15 weights, G7 nodes, G7 weights) at 70 digits. G7 nodes: the roots of P7.
    Kronrod nodes: the roots of the monic degree-8 Stieltjes polynomial E, the one with
    int P7 E x^k = 0 for k = 0..7 (a linear system in the monomial basis). Weights: exactness on
    the monomials below the node count."""
    with mp.workdps(70):
        p7 = mp.taylor(lambda t: mp.legendre(7, t), 0, 7)            # low -> high
        gauss = sorted(r.real for r in mp.polyroots(p7[::-1], maxsteps=200, extraprec=400))
        a, rhs = mp.matrix(8, 8), mp.matrix(8, 1)
        for k in range(8):
            for j in range(8):
                a[k, j] = sum(p7[i] * _moment(i + j + k) for i in range(8))
            rhs[k] = -sum(p7[i] * _moment(i + 8 + k) for i in range(8))
        e = mp.lu_solve(a, rhs)
        stieltjes = [mp.mpf(1)] + [e[j] for j in range(7, -1, -1)]    # high -> low
        kronrod = [r.real for r in mp.polyroots(stieltjes, maxsteps=200, extraprec=400)]
        nodes = sorted(gauss + kronrod)
        return nodes, _weights(nodes), gauss, _weights(gauss)


def test_derivation_is_the_gauss_kronrod_pair(derived):
    """K15 is exact on the monomials up to degree 22, G7 up to 13 and not at 14; the figures
    quoted for orientation come out."""
    nodes, wk, gauss, wg = derived
    with mp.workdps(70):
        for k in range(23):
            assert abs(sum(w * t ** k for w, t in zip(wk, nodes)) - _moment(k)) < mp.mpf(10) ** -60
        for k in range(14):
            assert abs(sum(w * t ** k for w, t in zip(wg, gauss)) - _moment(k)) < mp.mpf(10) ** -60
        assert abs(sum(w * t ** 14 for w, t in zip(wg, gauss)) - _moment(14)) > mp.mpf(10) ** -5
        assert mp.nstr(nodes[14], 33) == "0.991455371120812639206854697526329"
        assert mp.nstr(wk[14], 33) == "0.0229353220105292249637320080589696"
        assert mp.nstr(wk[7], 33) == "0.209482141084727828012999174891714"
        assert mp.nstr(wg[3], 33) == "0.417959183673469387755102040816327"
        assert all(abs(nodes[2 * j + 1] - gauss[j]) < mp.mpf(10) ** -60 for j in range(7))


def test_table_holds_the_correctly_rounded_doubles(derived):
    nodes, wk, gauss, wg = derived
    m = native()
    t, w15, w7 = m.gk15_nodes(), m.gk15_weights(), m.gk7_weights()
    assert t.shape == (15,) and w15.shape == (15,) and w7.shape == (7,)
    with mp.workdps(70):
        want_t = [float(v) for v in nodes]       # mpf -> float rounds to nearest
        want_t[7] = 0.0                          # the root of an odd polynomial
        assert [float(v) for v in t] == want_t
        assert [float(v) for v in w15] == [float(v) for v in wk]
        assert [float(v) for v in w7] == [float(v) for v in wg]
    assert list(t) == sorted(t) and list(t[:7]) == [-v for v in t[:7:-1]]


def test_source_prints_the_table_as_hex_floats():
    m = native()
    src = m.expr_adapt_source("1.0/(x*x+1e-8)")
    import re

    printed = [float.fromhex(h) for h in re.findall(r"0x[01]\.[0-9a-f]*p[+-]\d+", src)]
    table = list(m.gk15_nodes()[8:]) + list(m.gk15_weights()[7:]) + list(m.gk7_weights()[3:])
    assert sorted(printed) == sorted(float(v) for v in table + [50 * 2.0 ** -52])
    assert not re.search(r"\d\.\d{6,}", src.replace("1e-8", ""))   # no typed decimal constants
    assert "return (1.0/(x*x+1e-8));" in src
    for kernel in ("miint_adapt_init", "miint_adapt_eval", "miint_adapt_close",
                   "miint_adapt_decide", "miint_adapt_prefix", "miint_adapt_scatter"):
        assert f"void {kernel}(" in src
    with pytest.raises(RuntimeError, match="rejected"):
        m.expr_adapt_source("x; x")


def test_compiles_for_gfx950():
    m = native()
    code = m.expr_adapt_compile("(x<0.3)?1.0:0.0")
    assert code[:4] == b"\x7fELF" and len(code) > 4096
    with pytest.raises(RuntimeError, match="does not compile"):
        m.expr_adapt_compile("nosuchfunction(x)")


def test_abscissae_are_the_fused_nodes():
    m = native()
    lo, hi = np.array([0.0, -1.0, 0.1]), np.array([1.0, 1.0, 0.1 + 2.0 ** -40])
    x = m.gk15_abscissae(lo, hi)
    t = m.gk15_nodes()
    assert x.shape == (3, 15)
    for i in range(3):
        hw = 0.5 * (hi[i] - lo[i])
        c = lo[i] + hw
        with mp.workdps(60):
            assert [float(v) for v in x[i]] == [float(mp.mpf(hw) * mp.mpf(tj) + mp.mpf(c))
                                                for tj in t]
        assert lo[i] < x[i, 0] and x[i, 14] < hi[i]


# ------------------------------------------------------------------ the model
def _model_runs():
    runs = []
    for case in ac.SMOOTH:
        for panels in (1, 3, 64, 257):
            runs.append((case, dict(panels=panels)))
    for case in ac.TOLERANCE:
        for rtol in ac.RTOLS:
            runs.append((case, dict(rtol=rtol, panels=ac.PANELS)))
            runs.append((case, dict(rtol=rtol, panels=ac.FEW_PANELS)))
    runs.append((ac.COS2000, ac.COS2000_ARGS))
    runs.append((ac.INV_SQRT, dict(rtol=1e-13, panels=ac.PANELS)))
    runs.append((ac.SQRT_NEG, dict(panels=ac.PANELS)))
    runs.append((ac.RESONANCE, dict(panels=64, max_intervals=64)))
    runs.append((ac.RESONANCE, dict(max_depth=0, panels=ac.PANELS)))
    return runs


@pytest.mark.parametrize("case,args", _model_runs(),
                         ids=lambda v: v.name if isinstance(v, ac.Case) else
                         ",".join(f"{k}={x}" for k, x in v.items()) or "defaults")
def test_model_identities_and_truth(case, args):
    r = ac.model(case, **args)
    panels = args["panels"]
    assert r["intervals"] == panels + r["splits"]
    assert r["evals"] == 15 * (r["intervals"] + r["splits"])
    assert r["lo"].shape == r["hi"].shape == (r["intervals"],)
    assert r["lo"][0] == case.a and r["hi"][-1] == case.b
    assert np.array_equal(r["hi"][:-1], r["lo"][1:])
    assert np.all(r["hi"] >= r["lo"])
    assert r["evals"] < 10 ** 5 and r["rounds"] <= 61
    assert r["converged"] == (r["err_est"] <= r["tol"] and not r["capped"]
                              and r["nonfinite"] == 0)
    if r["converged"]:
        assert abs(r["value"] - case.truth) <= r["tol"]


def test_model_figures_the_gpu_tests_rely_on():
    for case in ac.SMOOTH:             # smooth: one round, nothing split, at every panel count
        for panels in (3, 64, 257):
            r = ac.model(case, panels=panels)
            assert (r["rounds"], r["splits"], r["converged"]) == (1, 0, True), (case, panels)
    for case in ac.TOLERANCE:          # each converged; from 16 panels each one has to split
        for rtol in ac.RTOLS:
            assert ac.model(case, rtol=rtol, panels=ac.PANELS)["converged"], (case, rtol)
            r = ac.model(case, rtol=rtol, panels=ac.FEW_PANELS)
            assert r["converged"] and r["splits"] >= 4, (case, rtol, r["splits"])
    r = ac.model(ac.COS2000, **ac.COS2000_ARGS)   # four workgroups, splits in all of them
    assert (r["rounds"], r["intervals"], r["peak"]) == (11, 1011, 998) and r["peak"] >= 600
    r = ac.model(ac.INV_SQRT, rtol=1e-13, panels=ac.PANELS)   # an honest failure at the singular end
    assert not r["converged"] and r["forced"] >= 1 and r["rounds"] == 61
    assert abs(r["value"] - 2.0) < 1e-9
    r = ac.model(ac.SQRT_NEG, panels=ac.PANELS)   # NaN on half of the range: accepted, counted
    assert r["nonfinite"] >= 1 and np.isnan(r["value"]) and not r["converged"]
    assert r["rounds"] <= 3
    r = ac.model(ac.RESONANCE, panels=64, max_intervals=64)
    assert r["capped"] and not r["converged"] and np.isfinite(r["value"])
    assert r["intervals"] == 64 and abs(r["value"] - ac.RESONANCE.truth) <= 10 * r["err_est"]
    r = ac.model(ac.RESONANCE, max_depth=0, panels=ac.PANELS)
    assert r["rounds"] == 1 and r["intervals"] == ac.PANELS and r["splits"] == 0 and r["forced"] >= 1


def test_model_floor_branch_bounds_the_work():
    """1.0/(x*x+1e-8) at rtol 1e-13: the intervals whose |K - G| is rounding noise are accepted
    (`floor`), the list stays at a few thousand."""
    r = ac.model(ac.RESONANCE, rtol=1e-13, panels=ac.PANELS)
    assert r["floor"] >= 1 and r["intervals"] < 20000 and r["rounds"] <= 61


def test_model_reversed_and_empty_range():
    fwd = ac.model(ac.RESONANCE, -1.0, 0.5, rtol=1e-8)
    rev = ac.model(ac.RESONANCE, 0.5, -1.0, rtol=1e-8)
    assert rev["value"] == -fwd["value"] and rev["err_est"] == fwd["err_est"]
    assert rev["lo"][0] == 0.5 and rev["hi"][-1] == -1.0
    assert np.array_equal(rev["hi"][:-1], rev["lo"][1:])
    z = aq.adaptive_model(ac.RESONANCE.f, 0.25, 0.25)
    assert z["value"] == 0.0 and z["evals"] == 0 and z["rounds"] == 0 and z["converged"]


# ------------------------------------------------------------------ refusals
BAD_OPTIONS = [
    (dict(rtol=0.0, atol=0.0), "rtol = 0 and atol = 0"),
    (dict(rtol=-1e-6), "rtol = -"),
    (dict(atol=-1.0), "atol = -1"),
    (dict(rtol=float("nan")), "rtol = nan"),
    (dict(panels=0), "panels = 0"),
    (dict(panels=65, max_intervals=64), "panels = 65 must be 1..max_intervals = 64"),
    (dict(max_intervals=0), "max_intervals = 0"),
    (dict(max_intervals=(1 << 26) + 1), "max_intervals = 67108865"),
    (dict(max_depth=-1), "max_depth = -1"),
    (dict(max_depth=201), "max_depth = 201"),
]


@pytest.mark.parametrize("opts,message", BAD_OPTIONS, ids=[m for _, m in BAD_OPTIONS])
def test_refusals_name_the_numbers(opts, message):
    m = native()
    full = dict(aq.DEFAULTS, **opts)
    o = m.AdaptOptions(full["rtol"], full["atol"], full["panels"], full["max_depth"],
                       full["max_intervals"])
    with pytest.raises(RuntimeError) as e:
        m.adapt_check(0.0, 1.0, o)
    assert message in str(e.value)
    with pytest.raises(ValueError) as e:   # the model refuses the same, in the same words
        aq.adaptive_model(np.sin, 0.0, 1.0, **full)
    assert message in str(e.value)
    from cuda_v_mpi_amd.ops import kernels
    with pytest.raises(RuntimeError) as e:  # before any device call
        kernels.quad_expr("sin(x)", 0.0, 1.0, **full)
    assert message in str(e.value)


def test_refuses_an_unbounded_range():
    m = native()
    for a, b in ((0.0, float("inf")), (float("nan"), 1.0), (-1e308, 1e308)):
        with pytest.raises(RuntimeError, match="must be finite"):
            m.adapt_check(a, b, m.AdaptOptions())
    m.adapt_check(1.0, 0.0, m.AdaptOptions())     # a > b and a == b are ranges
    m.adapt_check(1.0, 1.0, m.AdaptOptions())
    m.adapt_check(0.0, 1.0, m.AdaptOptions(rtol=0.0, atol=1e-9))


def test_options_and_defaults():
    m = native()
    o = m.AdaptOptions()
    assert (o.rtol, o.atol, o.panels, o.max_depth, o.max_intervals) == (1e-10, 0.0, 65536, 60,
                                                                        1 << 22)
    assert aq.DEFAULTS == dict(rtol=1e-10, atol=0.0, panels=65536, max_depth=60,
                               max_intervals=1 << 22)
    assert m.ADAPT_MAX_INTERVALS_LIMIT == 1 << 26 and m.ADAPT_MAX_DEPTH_LIMIT == 200
    assert m.ADAPT_DEFAULT_PANELS == 65536


# ------------------------------------------------------------------ the cpu backend
def test_cpu_backend_runs_the_model_on_expr_torch():
    r = integrate_expr_adaptive("1.0/(x*x+1e-8)", -1.0, 1.0, rtol=1e-10, panels=ac.PANELS,
                                backend="cpu")
    assert isinstance(r, AdaptiveResult) and r.backend == "cpu" and r.converged
    want = ac.model(ac.RESONANCE, rtol=1e-10, panels=ac.PANELS)
    assert r.evals == want["evals"] and r.rounds == want["rounds"]
    assert abs(r.value - ac.RESONANCE.truth) <= r.tol
    assert r.intervals == ac.PANELS + r.splits and r.as_dict()["expr"] == "1.0/(x*x+1e-8)"
    r = integrate_expr_adaptive("exp(-x*x)", 3.0, 0.0, atol=1e-12, rtol=0.0, panels=8,
                                backend="cpu")
    assert r.converged and abs(r.value + ac.GAUSS3.truth) <= 1e-12
    with pytest.raises(ValueError, match="backend must be"):
        integrate_expr_adaptive("x", 0.0, 1.0, backend="host")
    with pytest.raises(ValueError, match="cpu backend"):
        integrate_expr_adaptive("(x<0.3)?1.0:0.0", 0.0, 1.0, backend="cpu")


# ------------------------------------------------------------------ the CLIs
def _riemann(*args, env=None):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def _py(*args, env=None):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300, env=env)


BASE = ("--expr", "1.0/(x*x+1e-8)", "--a", "-1", "--b", "1", "--rtol", "1e-8")
CONFLICTS = [
    (("--n", "1e6"), "--n"),
    (("--rule", "mid"), "--rule"),
    (("--running",), "--running"),
    (("--ya", "0", "--yb", "1"), "--ya"),
    (("--params", "rows.txt"), "--params"),
    (("--linspace", "p0=0:1:4"), "--linspace"),
    (("--gpus", "2"), "--gpus 2"),
    (("--loopback", "2"), "--loopback"),
    (("--device", "cpu"), "--device cpu"),
]


@pytest.mark.parametrize("extra,named", CONFLICTS, ids=[n for _, n in CONFLICTS])
def test_native_cli_names_the_conflict(extra, named):
    for tol in (("--rtol", "1e-8"), ("--atol", "1e-8")):
        p = _riemann("--expr", "x", "--a", "0", "--b", "1", *tol, *extra)
        assert p.returncode == 1 and "--rtol / --atol" in p.stderr and named in p.stderr, p.stderr


def test_native_cli_refuses_ranks_bad_numbers_and_stray_bounds():
    p = _riemann(*BASE, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode == 1 and "WORLD_SIZE = 2" in p.stderr
    for flag, value, word in (("--rtol", "1e-8x", "--rtol must be a number"),
                              ("--atol", "small", "--atol must be a number"),
                              ("--panels", "12.5", "--panels must be a whole number"),
                              ("--max-depth", "deep", "--max-depth must be a whole number"),
                              ("--max-intervals", "1e7.", "--max-intervals must be")):
        args = [a for a in BASE] + [flag, value]
        p = _riemann(*args)
        assert p.returncode == 1 and word in p.stderr, (flag, p.stderr)
    p = _riemann("--expr", "x", "--a", "0", "--b", "1", "--rtol", "0")
    assert p.returncode == 1 and "rtol = 0 and atol = 0" in p.stderr
    p = _riemann(*BASE, "--panels", "0")
    assert p.returncode == 1 and "panels = 0" in p.stderr
    p = _riemann(*BASE, "--max-depth", "300")
    assert p.returncode == 1 and "max_depth = 300" in p.stderr
    # a misspelt or orphaned knob does not run the fixed-n default instead
    p = _riemann("--expr", "x", "--a", "0", "--b", "1", "--panels", "64", "--device", "cpu")
    assert p.returncode == 1 and "belong to --rtol / --atol" in p.stderr
    p = _riemann("--rtol", "1e-8", "--device", "cpu", "--n", "1e4")
    assert p.returncode == 1 and "--expr" in p.stderr
    p = _riemann("--help")
    assert p.returncode == 0 and "--rtol R" in p.stdout and "--max-intervals M" in p.stdout


def test_python_cli_names_the_conflict():
    for extra, named in ((("--n", "1e6"), "--n"), (("--rule", "mid"), "--rule"),
                         (("--ya", "0", "--yb", "1"), "--ya"),
                         (("--params", "rows.txt"), "--params"),
                         (("--linspace", "p0=0:1:4"), "--linspace"),
                         (("--device", "cpu"), "--device cpu"),
                         (("--backend", "host"), "--backend host")):
        p = _py(*BASE, *extra)
        assert p.returncode != 0 and "--rtol / --atol" in p.stderr and named in p.stderr, p.stderr
    p = _py(*BASE, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode != 0 and "WORLD_SIZE = 2" in p.stderr
    p = _py(*BASE, "--rtoll", "1e-8")
    assert p.returncode == 2 and "unrecognized arguments" in p.stderr
    p = _py("--expr", "x", "--panels", "64")
    assert p.returncode != 0 and "belong to --rtol / --atol" in p.stderr
    p = _py("--rtol", "1e-8")
    assert p.returncode != 0 and "--expr" in p.stderr
    p = _py("--expr", "x", "--rtol", "0")
    assert p.returncode != 0 and "rtol = 0 and atol = 0" in p.stderr


def test_python_cli_fixed_n_defaults_are_unchanged():
    p = subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", "--backend", "cpu",
                        "--n", "1e5"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["n"] == 100000 and js["rule"] == "left" and js["integrand"] == "pi4"
