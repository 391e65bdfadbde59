"""What makes the truth-referenced velocity-table cases meaningful, asserted on any box: the
closed form against sample-by-sample sums on every table and both signs of h, the truth against
fixtures.table_integral, each case's branch census (by the kernel's own coordinate operations)
and its distance from a switch point, every tile's DEFINITION and every path's
operation-by-operation emulation within the derived bound of the truth, the host engine's table
path on the same cases, and that the bounds are not vacuous: each listed defect, applied to the
definition or the emulation, misses the bound of a named case by a factor of 4 or more."""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction

import numpy as np
import pytest

import table_truth_cases as tc
from cuda_v_mpi_amd.utils import fixtures
from cuda_v_mpi_amd.utils import table_truth as tt

FACTOR = 4.0
CAP64, CAP32 = 2.0 ** -40, 2.0 ** -14


def _sub(g: tt.Geometry, first: int, count: int) -> tt.Geometry:
    return dataclasses.replace(g, i_begin=g.i_begin + first, count=count)


# ---------------------------------------------------------------------------- the truth
@pytest.mark.parametrize("name", tc.TABLES)
def test_closed_form_equals_direct_sum(name):
    """Every table, h > 0, h < 0 and h = 0, three rules, domains inside the table, across both
    ends and outside it, 1 to 700 samples: the segment-by-segment closed form and the
    sample-by-sample sum are the same rational."""
    from cuda_v_mpi_amd.models import integrands
    t = tc.table(name) or None
    top = float(tc.entries(name) - 1)
    for k, (a, b, n, m) in enumerate([(0.0, top, 700, 700), (top, 0.0, 333, 333), (-2.5, top + 3.25, 501, 400),
                                      (top + 3.0, -1.5, 97, 97), (0.3, 0.3, 10, 7), (-7.0, -7.0, 10, 3),
                                      (top + 1.0, top + 9.0, 64, 64), (0.25, top * 0.75, 100003, 1),
                                      (0.0, top, 1000003, 512)]):
        g = tt.geometry(integrands.table(t, a, b), n, ("left", "mid", "right")[k % 3], k, m)
        assert tt.true_sum(g) == tt.direct_sum(g), (name, a, b, n, m)
        vals, exact = tt.true_values(g)
        assert all(float(e) == v for e, v in zip(exact, vals))


def test_truth_against_table_integral():
    """The midpoint rule is exact on a piecewise-linear function whose knots fall on sample
    boundaries: n a multiple of the segment count. fixtures.table_integral is a float sum."""
    from cuda_v_mpi_amd.models import integrands
    for name in ("profile", "jag", "max"):
        t = tc.table(name) or None
        top = tc.entries(name) - 1
        g = tt.geometry(integrands.table(t), 4 * top, "mid")
        ref = fixtures.table_integral(0.0, float(top), t)
        scale = sum(abs(v) for v in g.table)
        assert abs(float(tt.true_value(g)) - ref) <= 1e-13 * scale, name
    g = tt.geometry(integrands.table(), 10 ** 9, "mid")
    assert float(tt.true_value(g)) == tc.WHOLE_1E9_MID


def test_tables_are_what_they_claim():
    jag = tc.table("jag")
    trap = sum(jag[1:-1]) + 0.5 * (jag[0] + jag[-1])
    assert abs(trap) <= 1e-12 * sum(abs(v) for v in jag)
    d = np.diff(jag)
    assert (d > 0).any() and (d < 0).any()
    off = np.array(tc.table("offset"))
    assert np.all(np.abs(off - 1e6) <= 1e-2) and np.ptp(off) > 1e-3
    dec = np.abs(tc.table("decades"))
    assert dec.max() / dec.min() >= 1e9
    assert len(tc.table("two")) == 2 and len(tc.table("max")) == tt.MAX_ENTRIES
    e = tc.table("ends")
    assert abs(e[1] - e[0]) < 1e-7 * abs(e[0]) and abs(e[-1] - e[-2]) > 1e4 * abs(e[-2])
    assert np.float32(e[0]) == np.float32(e[1])


# ---------------------------------------------------------------------------- the cases' conditions
@pytest.mark.parametrize("c", tc.GEOMS.values(), ids=lambda c: c.id)
def test_case_census_and_margin(c):
    """Each case holds the branches it names and none it forbids, in the launch's and in the
    point kernel's coordinates, and sits MARGIN ulps or more from a switch point unless it is
    there on purpose."""
    for points, count in ((False, c.count), (True, tc.point_count(c))):
        g = c.geometry(count)
        census = tt.tile_census(g, points)
        for k in c.need:
            assert census[k] > 0 or (points and count < c.count), (c.id, census)
        for k in c.forbid:
            assert census[k] == 0, (c.id, census)
        if not c.either:
            assert tt.switch_margin(g, points) >= tc.MARGIN, (c.id, tt.switch_margin(g, points))
    assert c.i_begin + c.count <= c.n
    if c.id.startswith("rev"):
        assert g.h < 0
    if c.id.startswith("ibegin"):
        assert c.i_begin > 1 << 32
    if "-sub" in c.id:
        assert abs(g.h) < math.ulp(g.x_abs_max)
    if c.id.startswith("far") and "-sub" not in c.id:
        assert abs(g.h) > math.ulp(g.x_abs_max)


def test_case_list_covers_what_it_claims():
    ids = set(tc.GEOMS)
    assert {c.table for c in tc.GEOMS.values()} == set(tc.TABLES)
    assert {c.count for c in tc.GEOMS.values()} >= {tc.ONE, tc.REM, tc.WG, tc.MANY}
    assert any(c.i_begin % 2 for c in tc.GEOMS.values())
    assert {g for c in tc.GEOMS.values() for g in c.grids} == {0, 1, 3}
    g = tc.GEOMS["kink-at-midpoint"].geometry()
    assert Fraction(tt.tile_midpoint(g, 0)) == 8              # kk = 0
    g = tc.GEOMS["kink-on-sample-20"].geometry()
    assert g.x(20) == 8
    g = tc.GEOMS["kink-half-step"].geometry()
    assert g.x(10) - 8 == Fraction(g.h) / 2
    g = tc.GEOMS["kink-last-knot"].geometry()
    assert g.x(0) < 35 < g.x(63) and g.nseg == 36
    g = tc.GEOMS["across-zero"].geometry()
    assert g.x(0) < 0 < g.x(63)
    g = tc.GEOMS["across-end"].geometry()
    assert g.x(0) < g.nseg < g.x(63)
    for cid, lo, hi in (("switch-below-1", 0.99, 1.0), ("switch-above-1", 1.0, 1.01),
                        ("switch-below-2", 1.99, 2.0), ("switch-above-2", 2.0, 2.01)):
        assert lo < 63 * abs(tc.GEOMS[cid].geometry().h) < hi
    assert set(tc.F32_SLOPE_CASES) <= ids


# ---------------------------------------------------------------------------- definition, emulation
def _tiles(g, T):
    n = g.count // T
    return sorted({0, n // 2, n - 1}) if n else []


@pytest.mark.parametrize("c", tc.GEOMS.values(), ids=lambda c: c.id)
def test_definition_and_emulation_within_point_bound(c):
    """Per sample, in the launch's and the point kernel's coordinates: the definition of the
    first, middle and last full tile and its fp64 emulation (r fused or not), the per-sample
    form for the per-sample tiles and the remainder, each within sample_bounds of v(x_i)."""
    for points in (False, True):
        g = c.geometry(tc.point_count(c) if points else c.count)
        bs = tt.sample_bounds("fp64-series", g, points)
        bi = tt.sample_bounds("fp64-ieee", g, points)
        for t in _tiles(g, 64):
            exact = [tt.interp_exact(g, g.x(64 * t + u)) for u in range(64)]
            _, vals = tt.defined_tile(g, t, points)
            emus = [tt.emulate_tile("fp64-series", g, t, points, fused)[1] for fused in (False, True)]
            for u in range(64):
                b = bs[64 * t + u]
                assert abs(vals[u] - exact[u]) <= b, (c.id, points, t, u)
                for e in emus:
                    assert abs(Fraction(e[u]) - exact[u]) <= b, (c.id, points, t, u)
        for t in _tiles(g, 32):
            _, vals, _ = tt.emulate_tile("fp64-ieee", g, t)
            for u in range(32):
                i = 32 * t + u
                assert abs(Fraction(vals[u]) - tt.interp_exact(g, g.x(i))) <= bi[i], (c.id, i)
        for path, b, T in (("fp64-series", bs, 64), ("fp64-ieee", bi, 32)):
            for i in range((g.count // T) * T, g.count):
                v = tt.emulate_point(path, g, tt.sample_coordinate(g, i, 2 if points else 1, T))
                assert abs(Fraction(v) - tt.interp_exact(g, g.x(i))) <= b[i], (c.id, path, i)


@pytest.mark.parametrize("path", tt.PATHS)
def test_emulated_tile_sums_within_launch_bound(path):
    """For every case, the first, middle and last tile of the path operation by operation
    (fp32 in exactly rounded fp32): within the launch bound of that tile's true sum."""
    worst = (0.0, "")
    T = tt.tile_len(path)
    for c in tc.GEOMS.values():
        g = c.geometry()
        for t in _tiles(g, T):
            sg = _sub(g, t * T, T)
            S, bound = tt.true_sum(sg), tt.launch_sum_bound(path, sg, 1)
            for fused in (False, True):
                v = tt.emulate_tile(path, sg, 0, fused=fused)[0]
                err = float(abs(Fraction(v) - S))
                assert err <= bound, (c.id, t, v, float(S), err, bound)
                worst = max(worst, (err / bound, c.id))
    print(f"TABLETRUTH cpu-emulation {path} worst ratio {worst[0]:.4f} at {worst[1]}")


def test_bounds_mean_something():
    """Every fp64 launch bound is at most 2**-40 of the launch's magnitude, every fp32 bound at
    most 2**-14, except where the coordinates themselves carry less: far out the bound is W
    ulp(x) per sample, and there it is at most 4 ulp(x) max|slope| per sample."""
    for c in tc.GEOMS.values():
        g = c.geometry()
        mag = tt.launch_magnitude(g)
        S = tt._Segs(g.table)
        coord = 4.0 * math.ulp(g.x_abs_max + 64 * abs(g.h)) * float(S.W.max()) * g.count
        for path in tt.PATHS:
            cap = CAP64 if path.startswith("fp64") else CAP32
            assert tt.launch_sum_bound(path, g, 1) <= cap * mag + coord, (c.id, path)


# ---------------------------------------------------------------------------- the host engine
@pytest.mark.parametrize("c", tc.GEOMS.values(), ids=lambda c: c.id)
def test_host_engine_against_truth(native, c):
    g = c.geometry()
    cfg = native.RiemannConfig()
    cfg.integrand = native.Integrand.table
    cfg.a, cfg.b, cfg.n = c.a, c.b, int(c.n)
    cfg.rule = getattr(native.Rule, c.rule)
    cfg.table = list(g.table)
    v = native.host_riemann(cfg, c.i_begin, c.count, native.HostPool(1))
    err, bound = float(abs(Fraction(v) - tt.true_value(g))), tt.host_value_bound(g)
    print(f"TABLETRUTH host {c.id} fp64-host err={err:.4e} bound={bound:.4e} ratio={err / bound:.4f}")
    assert err <= bound, (v, float(tt.true_value(g)), err, bound)


# ---------------------------------------------------------------------------- defects
def _defect_ratio(cid, defect, points=False):
    """The worst per-point ratio of the mutated definition over the case's tiles."""
    c = tc.GEOMS[cid]
    g = c.geometry(tc.point_count(c))
    b = tt.sample_bounds("fp64-series", g, points)
    worst = 0.0
    for t in range(min(g.count // 64, 48)):
        _, vals = tt.defined_tile(g, t, points, defect)
        for u in range(64):
            e = float(abs(vals[u] - tt.interp_exact(g, g.x(64 * t + u))))
            worst = max(worst, e / b[64 * t + u])
    return worst


def _report(name, ratio, where):
    print(f"TABLETRUTH defect {name}: ratio {ratio:.3e} at {where}")
    assert ratio >= FACTOR, (name, ratio, where)


@pytest.mark.parametrize("defect,cid", [
    (("knot_half",), "kink-on-sample-20"), (("knot_half",), "kink-at-midpoint"),
    (("centres",), "jag-line-1"), (("centres",), "kink-half-step"),
    (("wrong_dd",), "kink-in-first-half"), (("wrong_dd",), "kink-last-knot"),
    (("f32_slope",), "far-3e9"), (("f32_slope",), "jag-line-1"),
    (("clamp_short",), "across-end"), (("clamp_short",), "far-1e15"),
], ids=lambda v: "-".join(v) if isinstance(v, tuple) else v)
def test_defect_breaks_a_listed_case(defect, cid):
    _report(defect[0], _defect_ratio(cid, defect), cid)


@pytest.mark.parametrize("defect,cid", [(("f32_slope",), "far-2p60"), (("clamp_short",), "beyond-end-wg"),
                                        (("clamp_short",), "coarse-jag")],
                         ids=lambda v: "-".join(v) if isinstance(v, tuple) else v)
def test_defect_breaks_the_per_sample_form(defect, cid):
    """The same mutations in the per-sample form (the ieee tiles, the remainder loop): the last
    32 samples of the case against the fp64-ieee bound."""
    c = tc.GEOMS[cid]
    g = _sub(c.geometry(), c.count - 32, 32)
    b = tt.sample_bounds("fp64-ieee", g)
    ratio = max(float(abs(tt.point_defined(g, tt.sample_coordinate(g, i, 2), defect)
                          - tt.interp_exact(g, g.x(i)))) / b[i] for i in range(32))
    _report(f"{defect[0]} (per sample)", ratio, cid)


def test_defect_is_absent_from_the_definition():
    for cid in ("kink-on-sample-20", "jag-line-1", "far-3e9", "across-end", "coarse-jag"):
        assert _defect_ratio(cid, None) <= 1.0, cid


@pytest.mark.parametrize("cid", tc.F32_SLOPE_CASES)
def test_fp32_slope_from_rounded_entries_misses_the_fp32_bound(cid):
    """TableF32::pointf as it was, fmaf(fl32(v1) - fl32(v0), fr, fl32(v0)), in the fp32
    emulation: on an end segment whose entries round to one float, |x - lo| >= 3e9 away, the
    per-sample tile's sum misses the fp32-ieee launch bound; the form that subtracts in fp64 and
    converts the slope once is inside it."""
    g = _sub(tc.GEOMS[cid].geometry(), 0, 32)
    S, bound = tt.true_sum(g), tt.launch_sum_bound("fp32-ieee", g, 1)
    new = tt.emulate_tile("fp32-ieee", g, 0)[0]
    old = tt.emulate_tile("fp32-ieee", g, 0, f32_slope=True)[0]
    assert abs(Fraction(new) - S) <= bound
    s = tt.seg_exact(g, g.x(0))
    flat = np.float32(g.table[s]) == np.float32(g.table[s + 1]) and g.table[s] != g.table[s + 1]
    if flat:
        _report("fp32 slope from rounded entries (tile sum)", float(abs(Fraction(old) - S)) / bound, cid)
