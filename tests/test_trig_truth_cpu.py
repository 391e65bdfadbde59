"""What makes the truth-referenced sin / train cases meaningful, asserted on any box: the
closed form against a brute-force 200-bit sum, the representability the exact families
claim, the packed-fp32 tiles' sensitivity, the bound helpers' monotonicity and their
cross-check against the project's own figures, which division the dispatcher picks for every
case, and the host twins (fast_trig_host, host_riemann) against the same truth and bounds."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest

import trig_truth_cases as tc
from cuda_v_mpi_amd.utils import trig_truth as tt

MP = tt.MP
ULP1 = 2.0 ** -52


def _native_args(native, d, rule, i_begin, count):
    s = d.spec
    return (s.native_id, s.a, d.h, float(tt.RULE_OFF[rule]), i_begin, count, list(s.coef), s.p0,
            s.p1)


# ---------------------------------------------------------------------------- the truth
@pytest.mark.parametrize("dom", sorted(tc.DOMAINS))
def test_closed_form_equals_brute_force(dom):
    """Every family, reversed intervals and far angles included, at small m and odd starts:
    the closed form and the sample-by-sample 200-bit sum agree to 2**-150 of sum |f|."""
    d = tc.DOMAINS[dom]
    for rule, i0, m in (("left", 0, 257), ("mid", (d.n // 3) | 1, 193),
                        ("right", max(0, d.n - 131), min(131, d.n))):
        m = min(m, d.n - i0)
        a = tt.true_sum(d.spec, d.n, rule, i0, m)
        b = tt.brute_sum(d.spec, d.n, rule, i0, m)
        assert abs(a - b) <= MP.mpf(2) ** -150 * m * tt.geometry(d.spec, d.n, rule, i0, m).amp


def test_closed_form_refuses_an_ill_conditioned_step():
    with pytest.raises(ValueError):
        tt.trig_progression_sum(0, 2 * MP.pi, 10, cos=False)
    # and no case is anywhere near: every tile and slice sum evaluates
    for c in tc.SLICE_CASES:
        tc.truth_sum(c.dom, c.rule, c.i_begin, c.count)


def test_true_values_round_once():
    d = tc.DOMAINS["sin-3.4e9"]
    vals, exact = tt.true_values(d.spec, d.n, "mid", 5, 64)
    assert all(float(e) == v for e, v in zip(exact, vals))
    assert max(abs(MP.mpf(v) - e) / abs(e) for e, v in zip(exact, vals)) <= 2.0 ** -53


# ---------------------------------------------------------------------------- representability
@pytest.mark.parametrize("dom", sorted(tc.DOMAINS))
def test_exact_families_form_every_coordinate_exactly(dom):
    d = tc.DOMAINS[dom]
    g = tc.geom(dom, "mid", 0, d.n)
    assert tt.coords_exact(g) == d.exact
    if not d.exact:
        return
    assert tt.angle_exact(g)
    assert (d.spec.b - d.spec.a) / d.n == d.h and abs(d.h) == 2.0 ** round(math.log2(abs(d.h)))
    # first, last and a tile midpoint under every rule: the double is the exact value
    for rule in tc.RULES:
        gg = tc.geom(dom, rule, 0, d.n)
        for i in (0, d.n - 1, d.n // 3, d.n // 2 + 95.5):
            x = tt.Fraction(gg.a) + (tt.Fraction(i) + gg.off) * tt.Fraction(gg.h)
            assert tt.Fraction(float(x)) == x
    assert tt.angle_input_bound(g, 2) == 0.0


def test_angle_ranges_are_the_ones_named():
    q = lambda dom: tc.geom(dom, "left", 0, tc.DOMAINS[dom].n).quadrants  # noqa: E731
    lim = tt.TRIG_SERIES_MAX_N
    assert q("sin-near0") < 8 and q("sin-pm40") < 64
    for dom in ("sin-1e5", "train-1e5"):   # fast and library tiles in one launch
        d = tc.DOMAINS[dom]
        assert tc.geom(dom, "left", 0, 1).quadrants < tt.FAST_TRIG_MAX_N < q(dom)
    assert 2 ** 30 < q("sin-3.0e9") < lim and lim - 2 ** 17 < q("sin-3.373e9") < lim
    for dom in ("sin-3.4e9", "sin-m3.4e9", "sin-rev-3.4e9", "sin-1e12", "train-3.8e9",
                "train-1e12", "train-small-ts", "sin-3.4e9-coarse", "train-3.8e9-coarse"):
        assert q(dom) > 2.0 ** 31, dom
    assert tc.DOMAINS["train-neg-ts"].spec.p0 < 0
    assert any(c.i_begin > 2 ** 32 for c in tc.SLICE_CASES)
    assert any(c.i_begin > 2 ** 32 for c in tc.POINT_CASES)


def test_dispatcher_agrees_with_the_cases(native):
    """The tile lengths and the division every case runs, read from the extension (no
    launch): T is asserted from the code, and runs_series is the dispatcher's own choice."""
    assert native.TRIG_SERIES_MAX_N == tt.TRIG_SERIES_MAX_N
    assert native.FAST_TRIG_MAX_N == tt.FAST_TRIG_MAX_N
    D, V = native.DType, native.DivMode
    seen = set()
    for c in list(tc.TILE_CASES) + list(tc.SLICE_CASES):
        d = tc.DOMAINS[c.dom]
        count = getattr(c, "count", None) or tc.tile_of(d, c.div)
        g = tc.geom(c.dom, c.rule, c.i_begin, count)
        args = _native_args(native, d, c.rule, c.i_begin, count)
        dt = D.fp32 if c.dtype == "fp32" else D.fp64
        eff = native.riemann_effective_div(*args, dt, getattr(V, c.div))
        want = V.series if tc.runs_series(g, c.div) else V.ieee
        assert eff == want, c.id
        assert native.riemann_tile_len(*args, dt, getattr(V, c.div)) == \
            (tt.SERIES_TILE[d.name] if eff == V.series else tt.IEEE_TILE), c.id
        seen.add((d.name, c.dtype, c.div, eff == V.series))
    # both outcomes of a series request, for both integrands and types
    for name in ("sin", "train"):
        for dtype in ("fp64", "fp32"):
            assert (name, dtype, "series", True) in seen and (name, dtype, "series", False) in seen
    # series_exact (the Integrator's default request) is the same path
    d = tc.DOMAINS["sin-3.4e9"]
    args = _native_args(native, d, "left", 0, d.n)
    assert native.riemann_effective_div(*args, D.fp64, V.series_exact) == V.ieee
    d = tc.DOMAINS["sin-3.0e9"]
    args = _native_args(native, d, "left", 0, d.n)
    assert native.riemann_effective_div(*args, D.fp64, V.series_exact) == V.series


def test_far_limit_edges(native):
    """One end beyond the limit is enough; the limit itself still runs the series; NaN and
    infinite ends take the per-sample tiles (the library returns NaN for them)."""
    D, V = native.DType, native.DivMode
    th = tt.TRIG_SERIES_MAX_N / tt.TWO_OVER_PI

    def eff(a, h, n, i0=0, name="sin", ts=0.0):
        return native.riemann_effective_div(tc.integrands.NATIVE_ID[name], a, h, 0.0, i0, n, [],
                                            ts, 1.0, D.fp64, V.series)
    assert eff(th - 1000.0, 1.0, 900) == V.series
    assert eff(th - 1000.0, 1.0, 1200) == V.ieee           # the last sample is beyond
    assert eff(-th - 200.0, 1.0, 900) == V.ieee            # the first is
    assert eff(th + 1000.0, -1.0, 3000) == V.ieee          # reversed: the first is
    assert eff(0.0, 1.0, 100, i0=int(th) + 5) == V.ieee    # a far slice of a near domain
    assert eff(0.0, 1.0, 100, i0=int(th) - 500) == V.series
    assert eff(0.0, 1.0, 1000, name="train", ts=2.0 ** -21) == V.series
    assert eff(0.0, 1.0, 1000, name="train", ts=-(2.0 ** -22)) == V.ieee
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert eff(bad, 1.0, 10) == V.ieee
    assert eff(0.0, float("nan"), 10, i0=1) == V.ieee


# ---------------------------------------------------------------------------- sensitivity
FP32_TILES = [c for c in tc.TILE_CASES if c.dtype == "fp32"]


@pytest.mark.parametrize("c", FP32_TILES, ids=lambda c: c.id)
def test_fp32_tile_cases_would_see_one_misplaced_sample(c):
    """Moving one sample of the tile by one step (|delta f'(theta)| at the tile's most
    sensitive sample) is worth at least 8 bounds: a structural slip cannot hide in it."""
    assert tc.tile_sensitivity(c) >= 8.0 * tc.tile_bound(c), \
        (tc.tile_sensitivity(c), tc.tile_bound(c))


def _holds(g, shift_quarters: int) -> bool:
    """Does the tile's angle range hold a point (2 m + shift_quarters) pi / 4?"""
    lo, hi = sorted((g.theta(0), g.theta(g.count - 1)))
    q = MP.pi / 2
    off = shift_quarters * MP.pi / 4
    return MP.floor((hi - off) / q) > MP.floor((lo - off) / q) or MP.floor((lo - off) / q) == (lo - off) / q


def test_tile_cases_hold_the_tiles_that_matter():
    """Per family, path and type: the first tile, the last full tile, a tile holding a zero
    of sin or cos (a multiple of pi / 2: where trig_tile declines for the sign change or
    Fast2Sum's precondition and the series tile's samples cancel) and a tile holding a
    quadrant boundary of the reduction (an odd multiple of pi / 4: two quadrants in one tile)."""
    groups = {}
    for c in tc.TILE_CASES:
        groups.setdefault((c.dom, c.dtype, c.div), []).append(c)
    for d in tc.DOMAINS.values():
        for div in ("series", "ieee"):
            if d.n >= tc.tile_of(d, div):
                assert (d.id, "fp64", div) in groups
    for (dom, dtype, div), cases in groups.items():
        d = tc.DOMAINS[dom]
        T = tc.tile_of(d, div)
        gs = [tc.geom(dom, c.rule, c.i_begin, T) for c in cases]
        starts = {c.i_begin for c in cases}
        assert 0 in starts and d.n - T in starts, (dom, dtype, div)
        assert any(_holds(g, 0) for g in gs), (dom, dtype, div, "no zero of sin / cos")
        assert any(_holds(g, 1) for g in gs), (dom, dtype, div, "no quadrant boundary")
        if d.n > 4 * T:
            assert any(c.i_begin % 2 == 1 for c in cases), (dom, dtype, div)


def test_case_ids_are_unique_and_far_fp32_slices_are_whole_tiles():
    for cases in (tc.POINT_CASES, tc.TILE_CASES, tc.SLICE_CASES, tc.PLAN_CASES):
        ids = [c.id for c in cases]
        assert len(set(ids)) == len(ids)
    for c in tc.SLICE_CASES:
        g = tc.geom(c.dom, c.rule, c.i_begin, c.count)
        if c.dtype == "fp32" and tc.runs_series(g, c.div) and g.theta_abs_max > 64.0:
            assert c.count % tt.SERIES_TILE[g.name] == 0, c.id


def test_fp64_tile_cases_have_vast_margin():
    worst = min(tc.tile_sensitivity(c) / tc.tile_bound(c) for c in tc.TILE_CASES
                if c.dtype == "fp64" and tc.DOMAINS[c.dom].exact)
    assert worst >= 100.0, worst   # (the smallest: the train's first tile, where sin theta ~ 0)
    assert len(FP32_TILES) >= 20
    assert {c.div for c in FP32_TILES} == {"series", "ieee"}


# ---------------------------------------------------------------------------- the bounds
def test_bounds_cross_check_the_projects_figures():
    """|theta| <= 1e5 on exact coordinates: the derived per-point series bound is inside the
    4 ulp(1) = 8.9e-16 the project allows against ocml (test_sin_series_per_point_accuracy);
    the per-sample tile's is fdlibm's 1 ulp of the value, where the project MEASURES < 0.9
    (test_fast_trig_cpu.py): a measurement is no derivation, so the bound keeps the 1."""
    assert tt.series_point_bound(1.0e5 * tt.TWO_OVER_PI) <= 4 * ULP1
    assert tt.series_point_bound(1.0e5 * tt.TWO_OVER_PI) >= 3 * ULP1   # and no slack to spare
    g = tc.geom("sin-pm40", "left", 0, 4096)
    assert tt.series_value_point_bound(g) == tt.series_point_bound(g.quadrants)
    assert tt.ieee_point_bound(g, 0.75, True) == math.ulp(0.75)
    assert tt.ieee_point_bound(g, 0.75, False) == 2 * math.ulp(0.75)
    assert abs(tt.PIO2_RESIDUAL - 3.6e-27) < 1e-28
    # the reduction's residual at the limit: an eighth of its rounding term
    assert tt.TRIG_SERIES_MAX_N * tt.PIO2_RESIDUAL < 2.0 ** -54 / 7


def test_bounds_are_monotone():
    nq = [0.0, 1e2, 1e5, 1e9, 2.0 ** 31, 1e12]
    for f in (tt.reduction_bound, tt.seed_bound, tt.series_point_bound,
              lambda q: tt.series_point_bound(q, True)):
        v = [f(q) for q in nq]
        assert v == sorted(v) and v[-1] > v[0]
    assert tt.series_point_bound(1e3, True) > 1e6 * tt.series_point_bound(1e3)
    # farther, rounded coordinates cost more; exact ones nothing
    s = tc.integrands.IntegrandSpec
    near = tt.geometry(s("sin", 0.1, 1.3), 1000, "left", 0, 192)
    far = tt.geometry(s("sin", 1000.1, 1001.3), 1000, "left", 0, 192)
    assert 0 < tt.angle_input_bound(near, 1) < tt.angle_input_bound(far, 1) \
        < tt.angle_input_bound(far, 2)
    for fp32 in (False, True):
        assert tt.series_tile_bound(near, fp32) < tt.series_tile_bound(far, fp32)
        assert tt.series_tile_bound(near, fp32, abs_sum=50.0) < tt.series_tile_bound(near, fp32)
        b = [tt.ieee_tile_bound(dataclasses.replace(g, count=32), fp32) for g in (near, far)]
        assert b[0] < b[1]
    # the train's inexact ts costs theta U64 twice
    ref = tc.geom("train-ref-1e9", "left", 10 ** 9 - 128, 128)
    assert tt.angle_input_bound(ref, 1) >= 2 * tt.U64 * 6.28
    # per point: a larger value, a farther window, the library instead of the fdlibm kernels
    for fp32 in (False, True):
        v = [tt.ieee_value_bound(x, True, fp32) for x in (1e-300, 1e-9, 0.3, 0.6, 1.0)]
        assert v == sorted(v) and v[-1] > v[0]
    assert tt.ieee_value_bound(0.3, True) < tt.ieee_value_bound(0.3, False) \
        < tt.ieee_value_bound(0.3, False, True)
    for g in (near, far):
        assert tt.ieee_point_bound(g, 0.1, True) < tt.ieee_point_bound(g, 0.9, True) \
            < tt.ieee_point_bound(g, 0.9, False)
    assert tt.ieee_point_bound(near, 0.5, True) < tt.ieee_point_bound(far, 0.5, True)
    assert tt.series_value_point_bound(near) < tt.series_value_point_bound(far)
    assert tt.series_value_point_bound(near) > tt.series_point_bound(near.quadrants)
    tr = [tc.geom(dom, "left", 0, 4096) for dom in ("train-56", "train-1e7", "train-3.8e9")]
    v = [tt.series_value_point_bound(g) for g in tr]      # exact angles: only |n| grows
    assert v == sorted(v) and v[-1] > v[0]
    # the host twin: more samples, farther rounded coordinates, more threads' additions
    hb = tt.host_value_bound
    assert hb(near, 1) < hb(dataclasses.replace(near, count=1000), 1)
    assert hb(near, 1) < hb(far, 1) and hb(near, 1) < hb(near, 16)
    # launches: more samples, a deeper grid, a longer chain cost more
    g = tc.geom("sin-0pi-1e9", "left", 0, 10 ** 9)
    for div, fp32 in (("series", False), ("series", True), ("ieee", False), ("ieee", True)):
        small = tt.launch_value_bound(dataclasses.replace(g, count=10 ** 6), div, fp32, 2048)
        big = tt.launch_value_bound(g, div, fp32, 2048)
        assert small < big < tt.launch_value_bound(g, div, fp32, 1)
    assert tt.launch_depth(10 ** 9, 192, 2048) < tt.launch_depth(10 ** 9, 192, 256)
    assert tt.launch_depth(10 ** 9, 192, 2048) < tt.launch_depth(10 ** 9, 32, 2048)
    assert tt.launch_depth(192 * 5 + 191, 192, 1, 64) == 1 + 3 + 10 + 1 + 10
    # depth in the grid: fewer lanes run more rounds (up to one finalize partial per thread);
    # more workgroups give the finalize more partials per thread; and in the finalize's block
    v = [tt.launch_depth(10 ** 9, 192, gr) for gr in (256, 64, 3, 1)]
    assert v == sorted(v) and v[-1] > v[0]
    assert tt.launch_depth(1000, 32, 256) < tt.launch_depth(1000, 32, 4096)
    v = [tt.launch_depth(10 ** 6, 32, 4096, 256, fb) for fb in (1024, 256, 64)]
    assert v == sorted(v) and v[-1] > v[0]


# ---------------------------------------------------------------------------- the host twins
def _angles(d, rule, i0, count):
    g = tc.geom(d.id, rule, i0, count)
    x = np.array([float(g.x(i)) for i in range(count)])   # exact families: the doubles
    return g, (x if d.name == "sin" else x * (1.0 / d.spec.p0))


@pytest.mark.parametrize("dom", [k for k, d in sorted(tc.DOMAINS.items()) if d.exact])
def test_fast_trig_host_within_its_bound_of_the_truth(native, dom):
    """The per-sample tiles' sin / cos (fast_trig.hpp on the host) on the exact families: every
    sample it keeps is within 1 ulp of the true value; beyond kFastTrigMaxN it declines."""
    import torch

    d = tc.DOMAINS[dom]
    count = min(512, d.n)
    shift = 0 if d.name == "sin" else 1
    for i0 in tc.window_starts(d, count):
        g, th = _angles(d, "left", i0, count)
        exact = [(MP.sin if shift == 0 else MP.cos)(g.theta(i)) for i in range(count)]
        x = torch.tensor(th, dtype=torch.float64)
        v, e = torch.empty_like(x), torch.empty_like(x)
        native.fast_trig_host(x.data_ptr(), count, shift, v.data_ptr(), e.data_ptr())
        v = v.numpy()
        kept = ~np.isnan(v)
        if np.abs(th).min() * tt.TWO_OVER_PI > tt.FAST_TRIG_MAX_N + 1:
            assert not kept.any()
            continue
        bound = np.array([tt.ieee_value_bound(float(t), True) for t in exact])
        err = np.array([float(abs(MP.mpf(float(a)) - t)) if k else 0.0
                        for a, t, k in zip(v, exact, kept)])
        assert (err <= bound).all(), float((err / bound).max())


HOST_SLICES = [("sin-near0", "mid", 1, 8191), ("sin-pm40", "left", 3, 10001),
               ("sin-1e5", "right", 5, 9000), ("sin-3.4e9", "mid", 7, 5000),
               ("sin-rev-pm40", "left", 1, 10239), ("sin-0pi-1e9", "left", 333333333, 100001),
               ("sin-pi0-1e9", "mid", 0, 65537), ("train-56", "mid", 11, 50001),
               ("train-neg-ts", "left", 0, 4097), ("train-1e5", "left", 28000001, 20000),
               ("train-3.8e9", "mid", (1800 << 30) - 70001, 70000),
               ("train-rev-56", "right", 9, 12345), ("train-ref-1e9", "left", 999000001, 99999),
               ("train-ref-rev-1e9", "mid", 5, 77777), ("train-small-ts", "left", 999900000, 54321)]


@pytest.mark.parametrize("dom,rule,i0,m", HOST_SLICES, ids=[f"{s[0]}-{s[1]}" for s in HOST_SLICES])
@pytest.mark.parametrize("threads", [1, 3])
def test_host_riemann_within_its_bound_of_the_truth(native, dom, rule, i0, m, threads):
    d = tc.DOMAINS[dom]
    c = native.RiemannConfig()
    c.integrand = getattr(native.Integrand, d.spec.name)
    c.a, c.b, c.n = d.spec.a, d.spec.b, d.n
    c.rule = getattr(native.Rule, rule)
    c.p0, c.p1 = d.spec.p0, d.spec.p1
    v = native.host_riemann(c, i0, m, native.HostPool(threads))
    g = tc.geom(dom, rule, i0, m)
    want = tt.true_value(d.spec, d.n, rule, i0, m)
    err, bound = float(abs(MP.mpf(v) - want)), tt.host_value_bound(g, threads)
    print(f"host {dom} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound
