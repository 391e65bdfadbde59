"""CPU tests of double integrals between two curves (ExprAdaptiveRegion,
csrc/runtime/expr_adaptive_region.cpp): the numpy model of the rule against a direct loop, against
mpmath truths on every case the GPU tests use and against the rectangle's model, the mapped nodes
against exact rationals, the generated source and its gfx950 compile (no scratch, no spills),
every refusal, the CLIs' conflicts and the cpu backend. No device needed."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive2d_cases as ac
import expr_region_cases as rc
from cuda_v_mpi_amd import (Adaptive2DResult, AdaptiveRegionResult, integrate_expr2d_region,
                            native)
from cuda_v_mpi_amd.utils import adaptive_quad2d as aq2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the rule
def _direct(f, g, h, x0, x1, v0, v1):
    """The region rule of miint/expr.hpp on one rectangle of (x, v), operation by operation:
    the limits once per column, y by fma, the product by w, then the rectangle's sums."""
    m = native()
    fma = lambda a, b, c: float(m.fma(a, b, c))   # noqa: E731
    t, wk, wg = (list(map(float, v)) for v in (m.gk15_nodes()[7:], m.gk15_weights()[7:],
                                               m.gk7_weights()[3:]))
    hx = 0.5 * (x1 - x0)
    cx = x0 + hx
    hy = 0.5 * (v1 - v0)
    cy = v0 + hy
    xs = [cx] + [fma(hx, s * t[i], cx) for i in range(1, 8) for s in (-1.0, 1.0)]
    gs = [g(x) for x in xs]
    ws = [h(x) - gi for x, gi in zip(xs, gs)]

    def mapped(i, v):
        return f(xs[i], fma(ws[i], v, gs[i])) * ws[i]

    def row(v):
        f0 = mapped(0, v)
        rk, rg, ra = wk[0] * f0, wg[0] * f0, wk[0] * abs(f0)
        for i in range(1, 8):
            f1, f2 = mapped(2 * i - 1, v), mapped(2 * i, v)
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


RECTS = [(0.0, 1.0, 0.0, 1.0), (-0.75, 0.25, 0.5, 0.5 + 2.0 ** -20), (0.1, 0.3, 0.125, 0.875)]


@pytest.mark.parametrize("case", [rc.DISC_GAUSS, rc.PARABOLA, rc.PEAK_IN_DISC, rc.CROSSING],
                         ids=repr)
def test_model_rule_is_the_direct_loop(case):
    """The vectorised rule against the loop, rectangle by rectangle: the same values (bit for
    bit: the map's roundings are shared) in the same sums, which differ by the fma's single
    rounding at most: 38 u of R (the rectangle's cases file)."""
    r = np.array(RECTS)
    got = aq2.product_rule(aq2.region_values(case.f, case.g, case.h), r[:, 0].copy(),
                           r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy())
    scalar = [lambda *a, fn=fn: float(fn(*map(np.float64, a))) for fn in (case.f, case.g, case.h)]
    for i, rect in enumerate(RECTS):
        k, err, ex, ey, ra = _direct(*scalar, *rect)
        noise = 40 * 2.0 ** -53 * ra
        assert abs(got[0][i] - k) <= noise and abs(got[4][i] - ra) <= noise
        for q, want in ((1, err), (2, ex), (3, ey)):
            assert abs(got[q][i] - want) <= 2 * noise
        assert ra > 0 and got[1][i] <= ra


def test_mapped_nodes_and_heights_are_the_exact_ones_rounded_once():
    """Limits x and 2 x on dyadic rectangles: g_i = x_i and w_i = 2 x_i - x_i = x_i exactly, the
    x nodes are fma(hx, -+t_i, cx) and y_ij = fma(w_i, v_j, g_i), each the exact rational
    rounded once; the value summed is f * w_i."""
    m = native()
    t = [Fraction(float(v)) for v in m.gk15_nodes()]           # ascending, t[7] = 0
    rects = np.array([(0.25, 0.75, 0.0, 1.0), (-3.0, -2.5, 0.125, 0.375), (1.0, 1.0 + 2.0 ** -30,
                                                                           0.5, 1.0)])
    seen = {}

    def f(x, y):
        seen["x"], seen["y"] = np.array(x), np.array(y)
        return 1.0 + 0.0 * x

    values = aq2.region_values(f, lambda x: x, lambda x: 2.0 * x)
    x = m.gk15_abscissae(rects[:, 0].copy(), rects[:, 1].copy())
    v = m.gk15_abscissae(rects[:, 2].copy(), rects[:, 3].copy())
    out = values(x, v)
    for n, (x0, x1, v0, v1) in enumerate(rects):
        hx, hv = 0.5 * (x1 - x0), 0.5 * (v1 - v0)             # exact on dyadic ends
        cx, cv = x0 + hx, v0 + hv
        for i in range(15):
            xi = float(Fraction(hx) * t[i] + Fraction(cx))
            assert x[n, i] == xi
            w = float(Fraction(2.0 * xi) - Fraction(xi))
            assert w == xi
            for j in range(15):
                vj = float(Fraction(hv) * t[j] + Fraction(cv))
                assert v[n, j] == vj
                assert seen["x"][n, j, i] == xi
                assert seen["y"][n, j, i] == float(Fraction(w) * Fraction(vj) + Fraction(xi))
                assert out[n, j, i] == w
    corners = aq2.region_corners(rects, lambda x: x, lambda x: 2.0 * x)
    assert corners.shape == (3, 4, 2)
    assert corners[0].tolist() == [[0.25, 0.25], [0.75, 0.75], [0.75, 1.5], [0.25, 0.5]]


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


@pytest.mark.parametrize("run", rc.RUNS, ids=rc.run_id)
def test_model_meets_the_truth(run):
    case, (px, py) = run
    r = rc.run_model(run)
    _identities(r, px * py)
    _tiles(r["rects"], (*case.xrange, 0.0, 1.0))
    assert r["converged"] and not r["capped"] and r["nonfinite"] == 0 and r["forced"] == 0
    print(f"{rc.run_id(run)}: |value - truth| = {abs(r['value'] - case.truth):.3e}, bound "
          f"{rc.value_bound(r):.3e}, rounds {r['rounds']}, rectangles {r['intervals']}")
    assert abs(r["value"] - case.truth) <= rc.value_bound(r)
    assert r["peak"] <= 4096 and r["evals"] < 4 * 10 ** 6 and r["rounds"] <= 60


def test_model_figures_the_gpu_tests_rely_on():
    r = rc.model(rc.DISC, rtol=1e-10, panels_x=1, panels_y=1)     # the partition test's run
    assert (r["rounds"], r["intervals"]) == (46, 90) and r["splits_x"] > 0
    r = rc.model(rc.DISC, rtol=1e-10, panels_x=64, panels_y=64)
    assert (r["rounds"], r["intervals"]) == (40, 9088) and abs(r["value"] - np.pi) <= 1e-15
    for case in (rc.TRIANGLE, rc.PARABOLA, rc.DUFFY):            # the map leaves polynomials and
        for shape in rc.SHAPES[1:]:                              # a smooth 1 / sqrt(1 + v^2)
            assert rc.run_model((case, shape))["rounds"] == 1
    assert rc.run_model((rc.DUFFY, (1, 1)))["rounds"] == 2
    # the honest failures: a limit that is NaN outside [-1, 1], and the cap
    wide = aq2.region_model(rc.DISC.f, rc.DISC.g, rc.DISC.h, -2.0, 2.0, panels_x=4, panels_y=4)
    assert wide["nonfinite"] > 0 and not wide["converged"] and np.isnan(wide["value"])
    capped = rc.model(rc.DISC, rtol=1e-10, panels_x=4, panels_y=4, max_intervals=64)
    assert capped["capped"] and not capped["converged"] and capped["intervals"] <= 64
    # by indicator on the bounding box the rectangle's rounds cap within 1e-3 of pi
    r = ac.model(ac.DISC, **ac.DISC_ARGS)
    assert r["capped"] and 1e-6 < abs(r["value"] - np.pi) <= 1e-3


def test_crossing_limits_and_reversed_ends_negate():
    c = rc.CROSSING
    left = aq2.region_model(c.f, c.g, c.h, -1.0, 0.0, rtol=1e-10, panels_x=4, panels_y=4)
    right = aq2.region_model(c.f, c.g, c.h, 0.0, 1.0, rtol=1e-10, panels_x=4, panels_y=4)
    assert left["value"] == -right["value"] and abs(right["value"] - 0.5) <= 1e-15
    assert left["resabs"] == right["resabs"] > 0
    p = rc.PARABOLA
    fwd = aq2.region_model(p.f, p.g, p.h, 0.0, 1.0, panels_x=3, panels_y=5)
    rev = aq2.region_model(p.f, p.g, p.h, 1.0, 0.0, panels_x=3, panels_y=5)     # ax > bx
    swapped = aq2.region_model(p.f, p.h, p.g, 0.0, 1.0, panels_x=3, panels_y=5)  # h < g
    assert rev["value"] == -fwd["value"] and np.array_equal(rev["rects"], fwd["rects"])
    assert abs(swapped["value"] + fwd["value"]) <= rc.value_bound(fwd)
    assert swapped["resabs"] > 0 and swapped["value"] < 0
    z = aq2.region_model(p.f, p.g, p.h, 0.25, 0.25)
    assert z["value"] == 0.0 and z["evals"] == 0 and z["rounds"] == 0 and z["converged"]


# The rectangle's model at the parent commit, before its 225 values came from a callback:
# (case, arguments) -> value, err_est, resabs as hex floats, rounds, rectangles, splits_x,
# splits_y, peak. Both integrands are arithmetic only, so the bits do not depend on a library.
PARENT_MODEL = [
    (ac.PEAK, dict(rtol=1e-8, panels_x=3, panels_y=5),
     ("0x1.d479970e22cafp+4", "0x1.1d419cf800000p-25", "0x1.d479970e22cafp+4", 14, 101, 38, 48,
      20)),
    (ac.KINK, ac.KINK_ARGS,   # the cases file's own note: 23 rounds, 8188 rectangles, peak 4096
     ("0x1.5555555562eb9p-2", "0x1.0304a5789c89cp-32", "0x1.5555555562eb9p-2", 23, 8188, 4095,
      4092, 4096)),
]


@pytest.mark.parametrize("case,args,want", PARENT_MODEL, ids=["peak", "kink"])
def test_the_rectangle_model_is_unchanged(case, args, want):
    r = ac.model(case, **args)
    got = (r["value"].hex(), r["err_est"].hex(), r["resabs"].hex(), r["rounds"], r["intervals"],
           r["splits_x"], r["splits_y"], r["peak"])
    assert got == want
    assert abs(r["value"] - case.truth) <= ac.value_bound(r)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_constant_limits_follow_the_rectangle_model(shape):
    """Limits 0.0 .. 3.0: the mapped integrand is 3 f(x, 3 v) on [0, 3] x [0, 1]. The same rounds
    and the same rectangles (v = y / 3) as the rectangle's model on [0, 3] x [0, 3], the value
    the same to both bounds. The integrand and the square are symmetric in x and y, so from one
    square ex = ey but for rounding and which axis is bisected first is not held: the two orders
    end in the same rectangles after the same number of splits."""
    run = (rc.CONSTANT, shape)
    r = rc.run_model(run)
    want = ac.model(ac.GAUSS, rtol=1e-10, panels_x=shape[0], panels_y=shape[1])
    for k in ("rounds", "intervals", "splits", "evals", "peak", "converged"):
        assert r[k] == want[k], k
    assert abs(r["value"] - want["value"]) <= rc.value_bound(r) + ac.value_bound(want)
    assert np.array_equal(r["rects"][:, :2], want["rects"][:, :2])
    assert np.allclose(3.0 * r["rects"][:, 2:], want["rects"][:, 2:], rtol=4 * rc.U, atol=0.0)


# ------------------------------------------------------------------ the source
KERNELS = ("miint_adapt2d_init", "miint_region_eval", "miint_adapt2d_close",
           "miint_adapt2d_decide", "miint_adapt2d_prefix", "miint_adapt2d_scatter")
SHARED = tuple(k for k in KERNELS if k != "miint_region_eval")
# sha256 of expr_adapt2d_source(expr) at the parent commit
PARENT_SOURCE = {
    "x*y": "4ae97aa111d5f2abe2f39609413746f160b6162d3e7496ac13277f2095a91c27",
    "exp(-(x*x+y*y))": "98bf06490fe777aecf1ccd020a9ee4273f10040d8d56c91ad3acd4a5f24ac465",
}
# sha256 of the 1-D sources of "x*x" at the parent commit
PARENT_1D = {
    "expr_adapt_source": "ca26d41f87ad937687b5f0459894980042bfd95db481c7b76134ba18b1300ed9",
    "expr_adapt_unbounded_source":
        "5c36d56a3a2d51c24c3443d5f3c474f6ab72a19b69492f748c586edb73dc6959",
    "expr_source": "9c793345ed79d6a31cc6e24a17bb5da5eaa85829ec105ffe94f8cde6c7610c67",
}


def _kernel_text(src: str, kernel: str) -> str:
    """The kernel with the comment in front of it, up to its closing brace."""
    at = src.index(f"void {kernel}(")
    start = src.rindex("\n\n", 0, at)
    return src[start:src.index("\n}\n", at) + 3]


def test_source_prints_the_table_as_hex_floats_and_keeps_the_rows_rolled():
    m = native()
    src = m.expr_region_source("1.0/(x*x+y*y+1e-8)", "-sqrt(1.0-x*x)", "sqrt(1.0-x*x)")
    printed = {float.fromhex(h) for h in re.findall(r"0x[01]\.[0-9a-f]*p[+-]\d+", src)}
    table = list(m.gk15_nodes()[8:]) + list(m.gk15_weights()[7:]) + list(m.gk7_weights()[3:])
    assert printed == {float(v) for v in table + [50 * 2.0 ** -52]}
    assert not re.search(r"\d\.\d{6,}", src.replace("1e-8", ""))   # no typed decimal constants
    assert "return (1.0/(x*x+y*y+1e-8));" in src
    assert "return (-sqrt(1.0-x*x));" in src and "return (sqrt(1.0-x*x));" in src
    for name in ("miint_f(double x, double y)", "miint_ylo(double x)", "miint_yhi(double x)"):
        assert src.count(f"double {name} {{") == 1
    for kernel in KERNELS:
        assert f"void {kernel}(" in src
    assert "miint_adapt2d_eval" not in src.replace("miint_adapt2d_eval's", "")
    # fifteen evaluations are written out (one row), not 225: the loop over the rows is rolled
    body = src[src.index("void miint_region_gk15x15("):src.index("#define MIINT_ST_D")]
    assert body.count("MIINT_ROW_") == 8 and body.count("#pragma unroll 1") == 1
    # the limits: thirty calls in front of the loop, fifteen columns, none inside it
    head, loop = body.split("#pragma unroll 1")
    assert head.count("MIINT_LIMITS_CENTRE()") == 1 and head.count("MIINT_LIMITS_PAIR(") == 7
    assert "MIINT_LIMITS" not in loop and "miint_ylo" not in loop and "miint_yhi" not in loop
    assert "contract(off)" in head
    columns = sorted(int(c) for p in re.findall(r"MIINT_LIMITS_PAIR\([^,]+, (\d+), (\d+)\)", head)
                     for c in p)
    assert columns == list(range(1, 15))
    assert sorted(int(c) for p in re.findall(r"PAIR\(.*?, (\d+), (\d+)\)\n", loop)
                  for c in p) == list(range(1, 15))
    # miint_ylo / miint_yhi are called by the limits' macro alone
    calls = [ln for ln in src.splitlines() if re.search(r"miint_y(lo|hi)\(", ln)
             and "__device__" not in ln]
    assert len(calls) == 1 and "miint_ylo(xi)" in calls[0] and "miint_yhi(xi) - g##i" in calls[0]
    assert "asm" not in src


def test_the_five_shared_kernels_are_the_rectangle_sources_text():
    m = native()
    rect = m.expr_adapt2d_source("x*y")
    region = m.expr_region_source("x*y", "x*x", "x")
    for kernel in SHARED:
        text = _kernel_text(rect, kernel)
        assert len(text) > 400 and text == _kernel_text(region, kernel), kernel
    # and everything around them: the prelude, the table, the end of the rule
    for piece in (rect[:rect.index("__device__ __forceinline__ double miint_f(")],
                  rect[rect.index("// The y direction's table"):rect.index("// One row of")],
                  rect[rect.index("    if (row == 0) {"):rect.index("// One rectangle per lane")],
                  rect[rect.index("// sum_K over the nb"):]):
        assert len(piece) > 300 and piece in region
    assert rect.endswith(region[region.index("// sum_K over the nb"):])


def test_the_rectangle_and_1d_sources_are_the_parents():
    m = native()
    for expr, want in PARENT_SOURCE.items():
        m.expr_region_source(expr, "0.0", "x")
        assert hashlib.sha256(m.expr_adapt2d_source(expr).encode()).hexdigest() == want
    for name, want in PARENT_1D.items():
        assert hashlib.sha256(getattr(m, name)("x*x").encode()).hexdigest() == want
    sweep = m.expr_adapt_sweep_source("exp(-p0*x*x)", 1)
    m.expr_region_compile("x*y", "0.0", "x")
    assert m.expr_adapt_sweep_source("exp(-p0*x*x)", 1) == sweep
    assert "region" not in m.expr_adapt2d_source("x*y") and "miint_ylo" not in sweep


def kernel_resources(code: bytes, kernel: str) -> dict:
    """vgpr_count, sgpr_count, scratch bytes and spills of one kernel, from the code object's
    notes (llvm-readelf of the ROCm installation)."""
    exe = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        notes = subprocess.run([exe, "--notes", f.name], capture_output=True, text=True,
                               check=True).stdout
    for block in notes.split(".name:")[1:]:
        if block.split()[0] == kernel:
            found = dict(re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|"
                                    r"vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block))
            return {k: int(v) for k, v in found.items()}
    raise AssertionError(f"no kernel {kernel} in the code object")


@pytest.mark.parametrize("case", rc.ALL, ids=repr)
def test_compiles_for_gfx950_without_scratch(case):
    """The fifteen columns' limits stay in registers: no scratch and no spills for every case's
    (f, y_lo, y_hi); the register count is printed, not held to a figure."""
    code = native().expr_region_compile(*case.triple)
    assert code[:4] == b"\x7fELF" and len(code) > 4096
    for kernel in KERNELS:
        assert kernel.encode() in code
    res = kernel_resources(code, "miint_region_eval")
    print(f"{case.name}: miint_region_eval {res}")
    assert res["private_segment_fixed_size"] == 0
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert 0 < res["vgpr_count"] <= 256


def test_a_bad_expression_does_not_compile_and_names_all_three():
    with pytest.raises(RuntimeError, match="does not compile") as e:
        native().expr_region_compile("x*y", "nosuchfunction(x)", "x")
    assert "'x*y' between 'nosuchfunction(x)' and 'x'" in str(e.value)


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
    full = dict(aq2.DEFAULTS, **opts)
    p = rc.PARABOLA
    with pytest.raises(ValueError) as e:
        aq2.region_model(p.f, p.g, p.h, 0.0, 1.0, **full)
    assert message in str(e.value) and "adaptive 2-D: " in str(e.value)
    from cuda_v_mpi_amd.ops import kernels
    kw = {k: v for k, v in full.items() if k not in ("panels_x", "panels_y")}
    with pytest.raises(RuntimeError) as e:  # before any device call
        kernels.quad_expr2d_region(p.expr, 0.0, 1.0, p.y_lo, p.y_hi,
                                   panels=(full["panels_x"], full["panels_y"]), **kw)
    assert message in str(e.value)
    with pytest.raises(RuntimeError) as e:
        integrate_expr2d_region(p.expr, 0.0, 1.0, p.y_lo, p.y_hi, **full)
    assert message in str(e.value)


@pytest.mark.parametrize("xrange,message", [
    ((0.0, float("inf")), "ax = 0 and bx = inf must be finite"),
    ((float("nan"), 1.0), "ax = nan and bx = 1 must be finite"),
    ((-1e308, 1e308), "ax = -1e+308 and bx = 1e+308 must be finite, and bx - ax too"),
], ids=["inf", "nan", "width"])
def test_refuses_an_unbounded_x_range(xrange, message):
    from cuda_v_mpi_amd.ops import kernels
    p = rc.PARABOLA
    with pytest.raises(RuntimeError) as e:
        kernels.quad_expr2d_region(p.expr, *xrange, p.y_lo, p.y_hi)
    assert message in str(e.value)
    with pytest.raises(ValueError) as e:
        aq2.region_model(p.f, p.g, p.h, *xrange)
    assert message in str(e.value)


BAD_EXPRESSIONS = [
    (("x*y", "y", "x"), ("the lower limit y_lo 'y'", "may not mention y")),
    (("x*y", "0.0", "x+y*y"), ("the upper limit y_hi 'x+y*y'", "may not mention y")),
    (("x*y", "exp(y)", "x"), ("the lower limit y_lo 'exp(y)'", "may not mention y")),
    (("x*y", "0.0; x", "x"), ("the lower limit y_lo '0.0; x' is rejected",)),
    (("x*y", "0.0", "x; 1.0"), ("the upper limit y_hi 'x; 1.0' is rejected",)),
    (("x; y", "0.0", "x"), ("the integrand 'x; y' is rejected",)),
    (("x*y", "", "x"), ("the lower limit y_lo '' is rejected",)),
]


@pytest.mark.parametrize("triple,words", BAD_EXPRESSIONS, ids=[w[0] for _, w in BAD_EXPRESSIONS])
def test_a_refused_expression_names_which_of_the_three(triple, words):
    from cuda_v_mpi_amd.ops import kernels
    calls = (lambda: native().expr_region_source(*triple),
             lambda: native().expr_region_compile(*triple),
             lambda: kernels.quad_expr2d_region(triple[0], 0.0, 1.0, triple[1], triple[2]),
             lambda: integrate_expr2d_region(triple[0], 0.0, 1.0, triple[1], triple[2],
                                             backend="cpu"))
    for call in calls:
        with pytest.raises(RuntimeError) as e:
            call()
        for word in words:
            assert word in str(e.value)


def test_names_that_only_contain_a_y_are_limits():
    m = native()
    src = m.expr_region_source("x*y", "cyl_bessel_i0(x)", "hypot(x, 1.0)")
    assert "return (cyl_bessel_i0(x));" in src and "return (hypot(x, 1.0));" in src


# ------------------------------------------------------------------ the cpu backend
def test_cpu_backend_runs_the_model_on_expr_torch():
    c = rc.PEAK_IN_DISC
    r = integrate_expr2d_region(c.expr, *c.xrange, c.y_lo, c.y_hi, rtol=1e-10, panels_x=3,
                                panels_y=5, backend="cpu")
    assert isinstance(r, AdaptiveRegionResult) and isinstance(r, Adaptive2DResult)
    assert r.backend == "cpu" and r.converged
    want = rc.model(c, rtol=1e-10, panels_x=3, panels_y=5)
    assert r.evals == want["evals"] and r.rounds == want["rounds"]
    assert (r.splits_x, r.splits_y) == (want["splits_x"], want["splits_y"])
    assert abs(r.value - want["value"]) <= rc.SLACK_UNITS * rc.U * r.resabs
    assert abs(r.value - c.truth) <= rc.value_bound(r)
    d = r.as_dict()
    assert (d["expr"], d["y_lo"], d["y_hi"]) == c.triple and (d["ay"], d["by"]) == (0.0, 1.0)
    assert (d["ax"], d["bx"]) == c.xrange
    r = integrate_expr2d_region("x+y", 1.0, 0.0, "x*x", "x", atol=1e-12, rtol=0.0, panels_x=8,
                                panels_y=8, backend="cpu")
    assert r.converged and abs(r.value + 0.15) <= 1e-12
    r = integrate_expr2d_region("1.0", -1.0, 1.0, "0.0", "x", atol=1e-10, rtol=0.0, backend="cpu")
    assert r.converged and abs(r.value) <= 1e-10 and r.resabs > 0.99
    with pytest.raises(ValueError, match="backend must be"):
        integrate_expr2d_region("x*y", 0.0, 1.0, "0.0", "x", backend="host")
    with pytest.raises(ValueError, match="cpu backend"):
        integrate_expr2d_region("x*y", 0.0, 1.0, "(x<0.5)?0.0:x", "1.0", backend="cpu")


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
LIMITS = "--y-lo / --y-hi"
X = ("--expr", "x*y", "--a", "0", "--b", "1")
BASE = (*X, "--y-lo", "0.0", "--y-hi=x", "--area-rtol", "1e-8")
# (the flags after --expr / --a / --b, what the message names)
CONFLICTS = [
    (("--y-lo", "0.0", "--area-rtol", "1e-8"), ("--y-lo and --y-hi go together", "--y-hi is")),
    (("--y-hi", "x", "--area-atol", "1e-8"), ("--y-lo and --y-hi go together", "--y-lo is")),
    (("--y-lo", "0.0", "--y-hi", "x"), (LIMITS, "--area-rtol R / --area-atol T")),
    (("--y-lo", "0.0"), (LIMITS, "--area-rtol R / --area-atol T")),
    (("--y-lo", "0.0", "--y-hi", "x", "--n", "1000"), (LIMITS, "--area-rtol R / --area-atol T")),
    (("--y-lo", "0.0", "--y-hi", "x", "--area-rtol", "1e-8", "--ya", "0", "--yb", "1"),
     (LIMITS, "--ya / --yb")),
    (("--y-lo", "0.0", "--y-hi", "x", "--area-rtol", "1e-8", "--ya", "0"), (LIMITS, "--ya / --yb")),
    (("--y-lo", "0.0", "--y-hi", "x", "--area-atol", "1e-8", "--yb", "1"), (LIMITS, "--ya / --yb")),
]
# whatever the rectangle form refuses is refused with the limits too, in its words
REFUSED_BY_THE_RECTANGLE_FORM = [
    (("--n", "1e6"), "--n"),
    (("--ny", "100"), "--ny"),
    (("--rule", "mid"), "--rule"),
    (("--params", "rows.txt"), "--params"),
    (("--linspace", "p0=0:1:4"), "--linspace"),
    (("--box", "0:1,0:1"), "--box"),
    (("--rtol", "1e-8"), "--rtol / --atol"),
    (("--row-atol", "1e-8"), "--row-rtol / --row-atol"),
    (("--device", "cpu"), "--device cpu"),
]
NATIVE_ONLY = [(("--running",), "--running"), (("--gpus", "2"), "--gpus 2"),
               (("--loopback", "2"), "--loopback"), (("--atol", "1e-8"), "--rtol / --atol"),
               (("--row-rtol", "1e-8"), "--row-rtol / --row-atol")]


@pytest.mark.parametrize("flags,words", CONFLICTS, ids=[" ".join(f) for f, _ in CONFLICTS])
def test_both_clis_name_the_limits_conflict(flags, words):
    for run in (_riemann, _py):
        p = run(*X, *flags)
        assert p.returncode != 0 and p.stdout == "", p.stdout
        for word in words:
            assert word in p.stderr, (run.__name__, p.stderr)


@pytest.mark.parametrize("extra,named", REFUSED_BY_THE_RECTANGLE_FORM + NATIVE_ONLY,
                         ids=[" ".join(e) for e, _ in REFUSED_BY_THE_RECTANGLE_FORM + NATIVE_ONLY])
def test_native_cli_refuses_what_the_rectangle_form_refuses(extra, named):
    p = _riemann(*BASE, *extra)
    assert p.returncode == 1 and WHO in p.stderr and named in p.stderr, p.stderr


def test_python_cli_refuses_what_the_rectangle_form_refuses():
    for extra, named in REFUSED_BY_THE_RECTANGLE_FORM + [(("--backend", "host"),
                                                          "--backend host")]:
        p = _py(*BASE, *extra)
        assert p.returncode != 0 and WHO in p.stderr and named in p.stderr, p.stderr


def test_clis_refuse_ranks_bad_options_bad_limits_and_print_help():
    for run in (_riemann, _py):
        p = run(*BASE, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
        assert p.returncode != 0 and "WORLD_SIZE = 2" in p.stderr and WHO in p.stderr
        p = run(*X, "--y-lo", "0.0", "--y-hi", "x", "--area-rtol", "0")
        assert p.returncode != 0 and "rtol = 0 and atol = 0" in p.stderr
        p = run(*BASE, "--panels", "9", "--panels-y", "8", "--max-intervals", "71")
        assert p.returncode != 0 and "panels_x * panels_y = 9 * 8" in p.stderr
        p = run(*X, "--y-lo", "y", "--y-hi", "x", "--area-rtol", "1e-8")
        assert p.returncode != 0 and "the lower limit y_lo 'y'" in p.stderr
        assert "may not mention y" in p.stderr
        p = run(*X, "--y-lo", "0.0", "--y-hi", "x; 1", "--area-rtol", "1e-8")
        assert p.returncode != 0 and "the upper limit y_hi 'x; 1' is rejected" in p.stderr
        p = run("--expr", "x; y", "--a", "0", "--b", "1", "--y-lo", "0.0", "--y-hi", "x",
                "--area-rtol", "1e-8")
        assert p.returncode != 0 and "the integrand 'x; y' is rejected" in p.stderr
        p = run("--y-lo", "0.0", "--y-hi", "x", "--area-rtol", "1e-8")
        assert p.returncode != 0 and "--expr" in p.stderr
        p = run(*X, "--area-rtol", "1e-8")     # the rectangle form's words, and the new way out
        assert p.returncode != 0 and "--ya AY --yb BY" in p.stderr and "--y-lo EXPR" in p.stderr
        p = run("--help")
        assert p.returncode == 0 and "--y-lo" in p.stdout and "--y-hi" in p.stdout
    p = _riemann("--expr", "x*y", "--a", "0", "--b", "inf", "--y-lo", "0.0", "--y-hi", "x",
                 "--area-rtol", "1e-8")
    assert p.returncode == 1 and "infinite range" in p.stderr
    p = _py("--expr", "x*y", "--a", "0", "--b=inf", "--y-lo", "0.0", "--y-hi", "x", "--area-rtol",
            "1e-8")
    assert p.returncode != 0 and "--b inf" in p.stderr and "infinite range" in p.stderr
    p = _riemann("--help")
    assert "--y-lo EXPR --y-hi EXPR" in p.stdout and "--y-lo=-sqrt(1.0-x*x)" in p.stdout
    assert "y_lo, y_hi" in p.stdout
