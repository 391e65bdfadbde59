"""What makes the truth-referenced polynomial cases meaningful, asserted on any box: the closed
form against brute-force sums, the host mirrors (long double c_i h^i, the dispatcher) against
the real thing, every Taylor-pair tile's DEFINITION and every path's operation-by-operation
emulation within the derived bound of the truth, each case's own conditions, the caps the
bounds must respect, no fp32 denormal in the accuracy lists, and that the bounds are not
vacuous: each listed defect, applied to the definition or to the emulation, misses the bound of
a named case by a factor of 4 or more (the detecting case is printed).

What tile sums cannot see is stated and asserted too: a wrong odd part O cancels exactly in a
sub-tile's sum, (E + k O) + (E - k O) = 2 E, so a launch's value holds E only. In fp64 O is
held through point_values (series_point runs the tile's own operations per sample); in fp32
there is no point kernel and O is not observable, as test_pi4_truth_gpu.py says of its fp32
paths."""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction

import numpy as np
import pytest

import poly_truth_cases as pc
from cuda_v_mpi_amd.utils import poly_truth as pt

FACTOR = 4.0            # a defect must miss a bound by this much
CAP64, CAP32 = 2.0 ** -40, 2.0 ** -14


def _sub(g: pt.Geometry, first: int, count: int) -> pt.Geometry:
    return dataclasses.replace(g, i_begin=g.i_begin + first, count=count)


def _native_args(g):
    return (2, g.a, g.h, float(g.off), g.i_begin, g.count, list(g.coef), 0.0, 0.0)


# ---------------------------------------------------------------------------- the truth
@pytest.mark.parametrize("dom", sorted(pc.DOMAINS))
def test_closed_form_equals_brute_force(dom):
    """Every domain, three rules, 1 to 16 coefficients, 1 to 357 samples and one launch of
    64 * 256 + 37: the power-sum closed form and the sample-by-sample sum are the same
    rational."""
    d = pc.DOMAINS[dom]
    shapes = [("left", 1, 1), ("mid", 4, 64), ("right", 8, 357), ("mid", 16, 100)]
    if dom == "offset-neg":
        shapes.append(("left", 8, pc.SIZES[2]))
    for rule, nc, m in shapes:
        g = pc.geom(dom, nc, rule, min((d.n // 3) | 1, d.n - m), m)
        assert pt.true_sum(g) == pt.direct_sum(g), (dom, rule, nc, m)


def test_closed_form_on_degenerate_and_tiny_steps():
    for c in pc.DEGENERATE_CASES[:8] + pc.UNDERFLOW_CASES[:13]:
        g = c.geometry()
        assert pt.true_sum(g) == pt.direct_sum(g), c.id
    g = pc.DEGENERATE_CASES[0].geometry()
    assert g.h == 0.0 and pt.true_value(g) == 0


def test_power_sums():
    assert pt.power_sums(5, 3) == (5, 10, 30, 100)
    assert pt.power_sums(1000, 15)[15] == sum(i ** 15 for i in range(1000))


def test_true_values_round_once():
    vals, exact = pt.true_values(pc.geom("offset-3to5", 7, "mid", 5, 64))
    assert all(float(e) == v for e, v in zip(exact, vals))


# ---------------------------------------------------------------------------- rounding helpers
def test_rnd32_is_one_correct_rounding():
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.standard_normal(1000) * 10.0 ** rng.integers(-44, 38, 1000),
                         [2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -126, 3.4028235e38,
                          3.4028236e38, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 0.0]])
    with np.errstate(over="ignore"):
        for x in xs:
            assert pt.rnd32(Fraction(float(x))) == float(np.float32(x))
    fr = 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)     # double rounding would go down
    assert pt.rnd32(fr) == 1 + 2.0 ** -23


@pytest.mark.skipif(np.finfo(np.longdouble).nmant != 63, reason="needs the x87 long double")
def test_prepared_cs_is_the_long_double_product():
    """prepared_cs against numpy's long double on this box: the same products the launchers
    form, for steps down to the underflow cases'."""
    cases = [pc.geom("balanced", 8, "mid", 0, 64), pc.geom("far", 8, "left", 0, 64),
             pc.geom("offset-neg", 8, "left", 0, 64)] + [c.geometry() for c in pc.UNDERFLOW_CASES[:13]]
    for g in cases:
        hp, want = np.longdouble(1.0), []
        for c in g.coef:
            want.append(float(np.longdouble(c) * hp))
            hp = hp * np.longdouble(g.h)
        assert pt.prepared_cs(g) == want


# ---------------------------------------------------------------------------- the dispatcher
def _all_cases():
    for c in pc.LAUNCH_CASES:
        yield c.id, c.dtype, c.div, c.geometry(), c.path
    for c in pc.POINT_CASES:
        yield c.id, "fp64", c.div, c.geometry(), c.path
    for c in pc.DEGENERATE_CASES + pc.UNDERFLOW_CASES:
        yield c.id, c.dtype, c.div, c.geometry(), f"{c.dtype}-ieee"


def test_every_case_runs_the_path_it_names(native):
    """The mirror and the dispatcher itself, asked without a launch: every accuracy case runs
    the path it is filed under (9, 12 and 16 coefficients run Horner on both requests), every
    degenerate and underflow case runs Horner per sample on both requests, and the tile length
    is that path's."""
    D, V = native.DType, native.DivMode
    for cid, dtype, div, g, path in _all_cases():
        assert pt.effective_path(dtype, div, g) == path, cid
        eff = native.riemann_effective_div(*_native_args(g), getattr(D, dtype), getattr(V, div))
        assert f"{dtype}-{str(eff).split('.')[-1]}" == path, cid
        T = native.riemann_tile_len(*_native_args(g), getattr(D, dtype), getattr(V, div))
        assert T == pt.tile_len(path), cid
    for c in pc.LAUNCH_CASES:
        if c.ncoef in pc.HORNER_ONLY:
            assert c.path.endswith("ieee")
    # series_exact asks for the same tiles in fp64; series_direct does not
    g = pc.geom("unit", 7, "mid", 1, 64)
    assert pt.effective_path("fp64", "series_exact", g) == "fp64-series"
    assert pt.effective_path("fp64", "series_direct", g) == "fp64-ieee"
    for div, want in (("series_exact", "series"), ("series_direct", "ieee")):
        eff = native.riemann_effective_div(*_native_args(g), D.fp64, getattr(V, div))
        assert str(eff).split(".")[-1] == want


def test_series_range_limits():
    """poly_series_in_range by its mirror: h = 0, a step whose reciprocal overflows, a c_i h^i
    that is a denormal or zero; a zero coefficient is not held against the step."""
    base = pc.geom("unit", 8, "mid", 1, 64)
    assert pt.series_in_range(base)
    assert not pt.series_in_range(dataclasses.replace(base, h=0.0))
    assert not pt.series_in_range(dataclasses.replace(base, h=2.0 ** -1030))
    assert not pt.series_in_range(dataclasses.replace(base, h=math.inf))
    tiny = dataclasses.replace(base, h=2.0 ** -150)
    assert not pt.series_in_range(tiny)                                   # c_7 h^7 = 0
    assert pt.series_in_range(dataclasses.replace(tiny, coef=base.coef[:6] + (0.0, 0.0)))
    assert all(not pt.series_in_range(c.geometry()) for c in pc.UNDERFLOW_CASES)
    assert all(not pt.series_in_range(c.geometry()) for c in pc.DEGENERATE_CASES)


def test_buckets():
    assert [pt.bucket(n, True) for n in range(1, 9)] == [4, 4, 4, 4, 6, 6, 7, 8]
    assert [pt.bucket(n, False) for n in (1, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 16, 16]
    assert [pt.top_indices(n) for n in (4, 6, 7, 8)] == [(2, 3), (4, 5), (6, 5), (6, 7)]


# ---------------------------------------------------------------------------- coverage
def test_case_lists_cover_what_they_claim():
    paths = {p: [c for c in pc.LAUNCH_CASES if c.path == p] for p in pt.PATHS}
    for p, cases in paths.items():
        assert {c.family for c in cases} == set(pc.FAMILIES), p
        assert {c.count for c in cases} == set(pc.SIZES), p
        assert {c.grid for c in cases if c.count == pc.SIZES[2]} == {1, 3}, p
        assert {c.rule for c in cases} == set(pc.RULES) and {c.fused for c in cases} == {True, False}, p
        for fam in pc.FAMILIES:
            assert any(c.i_begin % 2 == 1 for c in cases if c.family == fam), (p, fam)
    for p in ("fp64-series", "fp32-series"):
        # every bucket, and within it every count that moves a top index
        assert {c.ncoef for c in paths[p] if c.family == "balanced"} == set(range(1, 9)), p
        assert {pt.top_indices(pt.bucket(c.ncoef, True)) for c in paths[p]} == {(2, 3), (4, 5), (6, 5), (6, 7)}
    for p in ("fp64-ieee", "fp32-ieee"):
        assert {pt.bucket(c.ncoef, False) for c in paths[p]} == {4, 8, 16}, p
        for div in ("series", "ieee"):
            assert set(pc.HORNER_ONLY) <= {c.ncoef for c in paths[p] if c.div == div}, (p, div)
    pts = {(c.path, c.family) for c in pc.POINT_CASES}
    assert pts == {(p, f) for p in ("fp64-series", "fp64-ieee") for f in pc.FAMILIES}
    assert {pt.bucket(c.ncoef, True) for c in pc.POINT_CASES if c.div == "series"} == {4, 6, 7, 8}
    assert {pt.bucket(c.ncoef, False) for c in pc.POINT_CASES if c.div == "ieee"} == {4, 8, 16}
    for c in pc.LAUNCH_CASES:
        assert all(v != 0.0 and math.frexp(v)[0] != 0.5 for v in c.geometry().coef[1:]), c.id
        assert c.i_begin >= 0 and c.i_begin + c.count <= pc.DOMAINS[c.dom].n, c.id


def test_families_are_what_they_claim():
    """Across zero: the middle tile's midpoint within half a step of 0 (so 0 lies inside the
    tile, between its two sub-tile centres). Far: |u_m| >= 2**53, so ulp(u_m) >= 2 and
    u_m -+ 16 is absorbed in part. Sub-ulp: |h| < ulp(x).
    Reversed: h < 0. Balanced: every |c_m| (16 h)^m in [1/2, 1]."""
    for c in pc.LAUNCH_CASES + pc.POINT_CASES:
        g, d = c.geometry(), pc.DOMAINS[c.dom]
        if d.zero:
            t = (g.count // 64) // 2      # start() puts the crossing in the middle tile
            assert abs(g.x(64 * t + Fraction(63, 2))) <= abs(Fraction(g.h)) / 2, c.id
        if d.family == "far":
            um = abs(pt.tile_midpoint(g, 0) * pt.inv_h(g))
            assert um >= 2.0 ** 53 and math.ulp(um) >= 2.0, c.id
        if d.family in ("far", "subulp"):
            assert abs(g.h) < math.ulp(g.x_abs_max), c.id
        if d.family == "reversed":
            assert g.h < 0, c.id
        if d.family == "balanced":
            assert all(0.5 <= abs(v) * (16 * abs(g.h)) ** m <= 1.0 + 1e-9 for m, v in enumerate(g.coef))


# ---------------------------------------------------------------------------- bounds against the truth
def _tile_sum_ieee(path, g):
    """One 32-sample Horner tile, emulated: fp64 one chain; fp32 two fp32 chains joined in fp64."""
    den = False
    if path.startswith("fp64"):
        acc = 0.0
        for u in range(32):
            acc += pt.emulate_horner(path, g, u, roundings=2)[0]
        return acc, den
    F, a = pt.F32(), [0.0, 0.0]
    for u in range(32):
        v, dn = pt.emulate_horner(path, g, u, roundings=2)
        den |= dn
        a[u & 1] = F.add(a[u & 1], v)
    return a[0] + a[1], den or F.denormal


def _tiles_of(c):
    g = c.geometry()
    T = pt.tile_len(c.path)
    n = g.count // T
    return g, T, sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("path", pt.PATHS)
def test_emulated_tiles_within_bound_and_free_of_denormals(path):
    """For every launch case of the path, the first, middle and last tile and the first
    remainder sample, operation by operation in exactly rounded arithmetic (both roundings of
    the centre): within the launch bound of that tile's true sum, and no fp32 intermediate a
    non-zero denormal or an underflowed zero (whether the packed instructions flush is not
    something the suite may depend on)."""
    worst = (0.0, "")
    for c in [c for c in pc.LAUNCH_CASES if c.path == path]:
        g, T, tiles = _tiles_of(c)
        for t in tiles:
            sg = _sub(g, t * T, T)
            S = pt.true_sum(sg)
            bound = pt.launch_sum_bound(path, sg, 1)
            if path.endswith("series"):
                runs = [pt.emulate_tile(path, sg, 0, fused) for fused in (False, True)]
                got = [(r[0], r[2]) for r in runs]
            else:
                got = [_tile_sum_ieee(path, sg)]
            for v, den in got:
                err = abs(Fraction(v) - S)
                assert err <= bound, (c.id, t, v, float(S), float(err), bound)
                assert not den, (c.id, t)
                worst = max(worst, (float(err) / bound, c.id))
        if g.count % T:
            i = (g.count // T) * T
            v, den = pt.emulate_horner(path, g, i, roundings=1)
            b = pt.sample_bounds(path, g)[i]
            assert abs(Fraction(v) - pt.p_exact(g.coef, g.x(i))) <= b and not den, c.id
    print(f"POLYTRUTH cpu-emulation {path} worst ratio {worst[0]:.4f} at {worst[1]}")


@pytest.mark.parametrize("c", pc.POINT_CASES, ids=lambda c: c.id)
def test_definition_within_point_bound_of_truth(c):
    """Per sample, with the point kernel's coordinates: the definition of every full series
    tile (both roundings of the centre) and the fp64 emulation of it, Horner's emulation for
    the rest, against p(x_i) within sample_bounds."""
    g = c.geometry()
    _, exact = pt.true_values(g)
    T = pt.tile_len(c.path)
    full = (g.count // T) * T
    if c.div == "series":
        for fused in (False, True):
            tiles = [pt.defined_tile(g, t, fused, points=True) for t in range(full // T)]
            local = np.concatenate([loc for _, loc in tiles])
            bound = pt.sample_bounds(c.path, g, points=True, local=local)
            vals = [v for tv, _ in tiles for v in tv]
            emu = [v for t in range(full // T) for v in pt.emulate_tile(c.path, g, t, fused, points=True)[1]]
            for i in range(full):
                assert abs(vals[i] - exact[i]) <= bound[i], (i, fused)
                assert abs(Fraction(emu[i]) - exact[i]) <= bound[i], (i, fused)
    bound = pt.sample_bounds(c.path, g, points=True)
    for i in range(0 if c.div == "ieee" else full, g.count):
        v, _ = pt.emulate_horner(c.path, g, i, roundings=2)
        assert abs(Fraction(v) - exact[i]) <= bound[i], i


def test_bounds_mean_something():
    """Every fp64 bound is at most 2**-40 of its case's magnitude sum_i M(x_i), every fp32 bound
    at most 2**-14: per launch, and per point case summed."""
    for c in pc.LAUNCH_CASES:
        g = c.geometry()
        cap = CAP64 if c.dtype == "fp64" else CAP32
        assert pt.launch_sum_bound(c.path, g, c.grid) <= cap * pt.launch_magnitude(g), c.id
        assert pt.launch_value_bound(c.path, g, c.grid) <= cap * abs(g.h) * pt.launch_magnitude(g), c.id
    for c in pc.POINT_CASES:
        g = c.geometry()
        assert pt.sample_bounds(c.path, g, points=True).sum() <= CAP64 * pt.launch_magnitude(g), c.id


# ---------------------------------------------------------------------------- defects
def _balanced_tile(nc: int, rule: str = "mid") -> pt.Geometry:
    """One tile of the balanced family across x = 0."""
    return pc.geom("balanced", nc, rule, pc.start("balanced", 64, rule), 64)


def _defect_ratios(g: pt.Geometry, defect, twice: int | None = None):
    """(worst per-point ratio, tile-sum ratio) of the mutated definition against the truth."""
    _, exact = pt.true_values(g)
    vals, local = pt.defined_tile(g, 0, False, defect=defect)
    pb = pt.sample_bounds("fp64-series", g, local=pt.defined_tile(g, 0, False)[1])
    point = max(float(abs(v - e)) / b for v, e, b in zip(vals, exact, pb))
    tot = sum(vals) + (vals[twice] if twice is not None else 0)
    return point, float(abs(tot - sum(exact))) / pt.launch_sum_bound("fp64-series", g, 1)


def _report(name, ratio, where):
    print(f"POLYTRUTH defect {name}: ratio {ratio:.3e} at {where}")
    assert ratio >= FACTOR, (name, ratio, where)


@pytest.mark.parametrize("nc", [4, 6, 7, 8])
def test_defect_top_index_off_by_two(nc):
    """ev or od two lower than Poly<NC>::parts has it (two higher leaves the array): the top
    even term is missing from every tile sum, the top odd term from the point values."""
    g = _balanced_tile(nc)
    point, total = _defect_ratios(g, ("ev", -2))
    _report(f"ev-2 NC={nc} (tile sum)", total, f"balanced-c{nc}")
    point, total = _defect_ratios(g, ("od", -2))
    _report(f"od-2 NC={nc} (points)", point, f"balanced-c{nc}")
    with pytest.raises(ValueError):
        pt.defined_tile(g, 0, False, defect=("ev", 2) if nc != 7 else ("od", 2))


@pytest.mark.parametrize("m", range(1, 8))
def test_defect_dropped_b(m):
    """b_m read as zero: an even m shows in the tile sum, an odd m in the point values."""
    g = _balanced_tile(8)
    point, total = _defect_ratios(g, ("drop_b", m))
    _report(f"b_{m} dropped ({'tile sum' if m % 2 == 0 else 'points'})",
            total if m % 2 == 0 else point, "balanced-c8")


@pytest.mark.parametrize("m", range(7))
def test_defect_skipped_shift_row(m):
    g = _balanced_tile(8, "left")
    point, total = _defect_ratios(g, ("skip_row", m))
    _report(f"shift row {m} skipped (points)", point, "balanced-c8-left")
    # every row feeds an even b_m (the last one finishes b_6): the tile sum sees each of them
    _report(f"shift row {m} skipped (tile sum)", total, "balanced-c8-left")


@pytest.mark.parametrize("defect", [("centre_sign", 0), ("centre_sign", 1), ("centre_step",),
                                    ("both_plus",)], ids=lambda d: "-".join(map(str, d)))
def test_defect_centres_and_signs(defect):
    g = _balanced_tile(8)
    point, total = _defect_ratios(g, defect)
    _report(f"{defect} (points)", point, "balanced-c8")
    _report(f"{defect} (tile sum)", total, "balanced-c8")


def test_defect_sample_counted_twice():
    g = _balanced_tile(8)
    for u in (0, 31, 32, 63):
        _, total = _defect_ratios(g, None, twice=u)
        _report(f"sample {u} counted twice (tile sum)", total, "balanced-c8")


@pytest.mark.parametrize("nc", [4, 8, 16])
def test_defect_horner_bucket_drops_its_top_coefficient(nc):
    dom = "unit" if nc <= 8 else "offset-3to5"
    g = pc.geom(dom, nc, "mid", pc.start(dom, 64, "mid"), 64)
    bound = pt.sample_bounds("fp64-ieee", g)
    ratio = max(float(abs(pt.horner_exact(g, i, drop_top=True) - pt.p_exact(g.coef, g.x(i)))) / bound[i]
                for i in range(g.count))
    _report(f"Horner bucket {nc} without c_{nc - 1} (points)", ratio, f"{dom}-c{nc}")
    tot = sum(pt.horner_exact(g, i, drop_top=True) for i in range(g.count))
    _report(f"Horner bucket {nc} without c_{nc - 1} (launch)",
            float(abs(tot - pt.true_sum(g))) / pt.launch_sum_bound("fp64-ieee", g, 1), f"{dom}-c{nc}")
    b32 = pt.launch_sum_bound("fp32-ieee", g, 1)
    _report(f"Horner bucket {nc} without c_{nc - 1} (fp32 launch)",
            float(abs(tot - pt.true_sum(g))) / b32, f"{dom}-c{nc}")


@pytest.mark.parametrize("m", range(0, 8, 2))
def test_defect_fp32_b_left_out_of_the_conversion(m):
    """PolyF32's loop that rounds b_m to packed fp32 skipping one m (bf[m] stays zero), in the
    fp32 emulation: every even m misses the fp32 launch bound. (An odd m cannot: below.)"""
    g = _balanced_tile(8)
    v, _, _ = pt.emulate_tile("fp32-series", g, 0, defect=("no_f32", m))
    ratio = float(abs(Fraction(v) - pt.true_sum(g))) / pt.launch_sum_bound("fp32-series", g, 1)
    _report(f"fp32 b_{m} not converted (tile sum)", ratio, "balanced-c8")


# ---------------------------------------------------------------------------- what sums cannot see
@pytest.mark.parametrize("defect", [("od", -2), ("drop_b", 1), ("drop_b", 3), ("drop_b", 5),
                                    ("drop_b", 7)], ids=lambda d: "-".join(map(str, d)))
def test_a_wrong_odd_part_is_invisible_to_tile_sums(defect):
    """(E + k O) + (E - k O) = 2 E: a defect confined to O changes no sub-tile sum, exactly,
    while it moves point values by many bounds. Launch values hold E only; O is held through
    point_values in fp64 and is not observable in fp32."""
    g = _balanced_tile(8)
    good, _ = pt.defined_tile(g, 0, False)
    bad, _ = pt.defined_tile(g, 0, False, defect=defect)
    for q in range(2):
        assert sum(good[32 * q:32 * q + 32]) == sum(bad[32 * q:32 * q + 32])
    point, total = _defect_ratios(g, defect)
    assert point >= FACTOR and total <= 1.0


@pytest.mark.parametrize("m", [1, 3, 5, 7])
def test_fp32_odd_b_is_not_observable(m):
    """The fp32 tile with an odd b_m missing still lands inside the fp32 launch bound: there is
    no fp32 point kernel, so the fp32 paths hold E only."""
    g = _balanced_tile(8)
    v, _, _ = pt.emulate_tile("fp32-series", g, 0, defect=("no_f32", m))
    assert abs(Fraction(v) - pt.true_sum(g)) <= pt.launch_sum_bound("fp32-series", g, 1)
