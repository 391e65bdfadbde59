"""What makes the truth-referenced 4/(1+x^2) cases meaningful, asserted on any box: the digamma
closed form against direct 400-bit sums, every series tile's DEFINITION within its derived
bound of the truth, each case's own conditions (the path the dispatcher runs, exact
coordinates where claimed, the tile across zero really across zero), the bitwise models
against independent arithmetic and the host twin, the caps the bounds must respect, and that
the bounds are not vacuous: each listed defect, applied to a definition or to the host
emulation of a tile, exceeds the bound of at least one case (the detecting case is printed:
profiles/r13/pi4_truth.md)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest

import pi4_truth_cases as pc
from cuda_v_mpi_amd.utils import pi4_truth as pt

MP = pt.MP
SERIES_TILES = [c for c in pc.TILE_CASES if c.path in pt.SERIES_PATHS]


def _rel(a, b) -> float:
    return float(abs(MP.mpf(a) - b) / abs(b))


# ---------------------------------------------------------------------------- the truth
@pytest.mark.parametrize("dom", sorted(pc.DOMAINS))
def test_closed_form_equals_direct_sums(dom):
    """Every family (reversed, across zero, h below ulp(x), far slices, h = 0) at 384 to 5000
    samples and odd starts: the closed form and the sample-by-sample sum agree to 2**-150."""
    d = pc.DOMAINS[dom]
    for rule, i0, m in (("left", 0, 384), ("mid", (d.n // 3) | 1, 1931),
                        ("right", max(0, min(d.n, 2 ** 51) - 5000), min(5000, d.n))):
        g = pc.geom(dom, rule, i0, m)
        a, b = pt.true_sum(g), pt.direct_sum(g)
        assert abs(a - b) <= MP.mpf(2) ** -150 * abs(b), (dom, rule, i0, m)


def test_closed_form_at_the_workloads_sizes():
    """N = 1e9 in milliseconds: the left rule is pi + h (the trapezoid correction
    h (f(0) - f(1)) / 2 ... = 1.0000001e-9), the midpoint rule pi to 1.3e-16."""
    left = pt.true_value(pc.geom("unit-1e9", "left")) - MP.pi
    mid = pt.true_value(pc.geom("unit-1e9", "mid")) - MP.pi
    assert abs(left - MP.mpf("1.0000001e-9")) < 1e-16 and 1.2e-16 < mid < 1.3e-16
    # the reversed interval under the mirrored rule: the same samples up to n fl(h) != 1
    rev = pt.true_value(pc.geom("rev-unit-96M", "right"))
    assert abs(rev + pt.true_value(pc.geom("unit-96M", "left"))) < 4 * 2.0 ** -53


def test_true_values_round_once():
    vals, exact = pt.true_values(pc.geom("8to9-96M", "mid", 5, 64))
    assert all(float(e) == v for e, v in zip(exact, vals))


# ---------------------------------------------------------------------------- rounding helpers
def test_rnd32_is_one_correct_rounding():
    """Against numpy on doubles (np.float32(double) rounds once), ties, the subnormal range,
    overflow, and a value that double rounding would get wrong."""
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-44, 38, 2000),
                         [2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -126, 3.4028235e38,
                          3.4028236e38, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 0.0]])
    with np.errstate(over="ignore"):
        for x in xs:
            assert pt.rnd32(Fraction(float(x))) == np.float32(x) or (
                math.isinf(float(np.float32(x))) and math.isinf(float(pt.rnd32(Fraction(float(x))))))
    # 1 + 2**-24 + 2**-60: above the tie, so up; through a double it becomes the tie and goes down
    fr = 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert pt.rnd32(fr) == np.float32(1 + 2.0 ** -23) and np.float32(float(fr)) == np.float32(1.0)


def test_model_block_sum_is_the_dpp_order():
    """One non-zero lane anywhere comes out unchanged; 256 distinct powers of two add up
    exactly whatever the order; and the order is the code's: the wave total of lanes 0..63
    holding 1, 2**-53, 2**-53, ... differs from the left-to-right sum."""
    for lane in (0, 17, 63, 64, 255):
        v = [0.0] * 256
        v[lane] = 0.1
        assert pt.model_block_sum(v) == 0.1
    assert pt.model_block_sum([1.0 + i for i in range(256)]) == sum(1.0 + i for i in range(256))
    v = [1.0] + [2.0 ** -53] * 63
    assert pt.model_block_sum(v) != math.fsum(v) or pt.model_block_sum(v) != sum(v)
    # pairs first: lane 1's 2**-53 is lost against 1, every other pair of them survives
    assert pt.model_block_sum(v) == 1.0 + 62 * 2.0 ** -53


def test_fp64_model_matches_the_host_twin(native):
    """host_riemann evaluates 1 / fma(x, x, 1) at x = fma(i, h, a) per sample, as f.point does:
    its value is SCALE h times the exact sum of model_point's values, up to the host's own
    summation (at most count additions of U64 each) and its two final products."""
    from cuda_v_mpi_amd import Integrator

    for a, b, n, rule in ((0.0, 1.0, 4099, "mid"), (9.0, 8.0, 2053, "left")):
        it = Integrator("pi4", n=n, rule=rule, backend="cpu", a=a, b=b)
        got = it.run().value
        g = pt.geometry(it.spec, n, rule)
        tot = MP.fsum(MP.mpf(pt.model_point("fp64-ieee", g, i)) for i in range(n))
        want = MP.mpf(pt.SCALE) * MP.mpf(g.h) * tot
        assert abs(MP.mpf(got) - want) <= (n + 4) * pt.U64 * abs(want), (got, float(want))


# ---------------------------------------------------------------------------- the cases' conditions
def _native_args(native, g):
    return (0, g.a, g.h, float(g.off), g.i_begin, g.count, [], 0.0, 0.0)


def _all_launches():
    for c in pc.TILE_CASES:
        yield c.id, c.path, pc.geom(c.dom, c.rule, c.i_begin, pt.tile_len(c.path))
    for c in pc.REM_CASES + pc.SLICE_CASES + pc.RANGE_CASES:
        yield c.id, c.path, pc.geom(c.dom, c.rule, c.i_begin, c.count)
    for c in pc.WINDOW_CASES:
        yield c.id, c.path, pc.geom(c.dom, c.rule, c.i_begin, pc.WINDOW)


def test_every_case_runs_the_path_it_names(native):
    """The dispatcher, asked without a launch: effective_div of every tile, remainder, window,
    slice and whole-range case is the path the case is filed under, the tile length is that
    path's, and the Python mirror of the dispatcher agrees with it on the far, degenerate and
    switch cases too."""
    D, V = native.DType, native.DivMode
    seen = set()
    for cid, path, g in _all_launches():
        dtype, div = pc.REQUEST[path]
        assert pc.expected_path(dtype, div, g) == path, cid
        args = _native_args(native, g)
        eff = native.riemann_effective_div(*args, getattr(D, dtype), getattr(V, div))
        assert f"{dtype}-{str(eff).split('.')[-1]}" == path, cid
        assert native.riemann_tile_len(*args, getattr(D, dtype), getattr(V, div)) == pt.tile_len(path)
        seen.add(path)
    assert seen == set(pc.PATHS)
    for c in pc.FAR_CASES:
        g = pc.geom(c.dom, "mid", c.i_begin, c.count)
        eff = native.riemann_effective_div(*_native_args(native, g), getattr(D, c.dtype),
                                           getattr(V, c.div))
        assert f"{c.dtype}-{str(eff).split('.')[-1]}" == pc.expected_path(c.dtype, c.div, g), c.id
    for c in pc.SWITCH_CASES:
        g = pt.geometry(c.spec, pc.SWITCH_N, "mid")
        assert native.riemann_pi4_ieee_narrow(*_native_args(native, g), getattr(D, c.dtype)) == \
            pc.expected_narrow(c.dtype, g) == (c.tag == "below"), c.id


def test_series_limits_are_the_codes(native):
    assert native.PI4_SERIES_MAX_X == pt.PI4_SERIES_MAX_X
    assert native.PI4_F32_SERIES_MAX_X == pt.PI4_F32_SERIES_MAX_X
    for path in pc.PATHS:
        T = pt.tile_len(path)
        half = {384: 192, 192: 96, 32: 16}[T]
        d = pc.DOMAINS[pc.dom_for(path, "unit")]
        if path.split("-")[1] != "ieee":     # the largest admitted h: one sample fewer is refused
            assert half * d.h <= pt.HALF_SPAN_H < half * (1.0 / (d.n - 2))


def test_far_series_requests_leave_the_series_tiles(native):
    """The two findings, at the dispatcher: an fp32 / fp32acc series request with an end beyond
    2**62 and an fp64 one beyond 2**249 run ieee (one end is enough, either sign, reversed
    too, NaN too); below the limits the series tiles still run; a == b is covered."""
    D, V = native.DType, native.DivMode

    def eff(dtype, div, a, h, n, i0=0):
        return str(native.riemann_effective_div(0, a, h, 0.5, i0, n, [], 0.0, 0.0,
                                                getattr(D, dtype), getattr(V, div))).split(".")[-1]
    h = 2.0 ** -26
    for dtype in ("fp32", "fp32acc"):
        assert eff(dtype, "series", 2.0 ** 61, h, 192) == "series"
        assert eff(dtype, "series", 2.0 ** 62 * (1 - 2.0 ** -30), h, 192) == "series"
        for a in (2.0 ** 62, -(2.0 ** 62), 1.2e19, 2e19, -2e19, 1e200, math.nan, math.inf):
            assert eff(dtype, "series", a, h, 192) == "ieee", (dtype, a)
        assert eff(dtype, "series", 0.0, 2.0 ** 40, 4, i0=2 ** 22) == "ieee"   # h too large anyway
        assert eff(dtype, "series", 1e200, 0.0, 292) == "ieee"
        assert eff(dtype, "series", 1.0, 0.0, 292) == "series"
    for div in ("series", "series_exact", "series_direct"):
        assert eff("fp64", div, 2e19, 2.0 ** -30, 400) == div
        assert eff("fp64", div, 2.0 ** 248, 0.0, 400) == div
        for a in (2.0 ** 249, -(2.0 ** 249), 1e200, math.nan):
            assert eff("fp64", div, a, 0.0, 400) == "ieee", (div, a)
        assert eff("fp64", div, 1.0, 0.0, 400) == div


@pytest.mark.parametrize("dom", [d for d in pc.DOMAINS if "exact" in d])
def test_exact_family_forms_every_coordinate_exactly(dom):
    """a dyadic, h = +-2**-27: every fp64 sample and tile midpoint is exact, and under the mid
    rule every 192-sample tile midpoint is an fp32 number, so the coordinate terms of the
    bounds vanish (the fp32 tiles keep the rounding of d_m, U32)."""
    d = pc.DOMAINS[dom]
    assert d.exact and abs(d.h) == 2.0 ** -27
    for rule in pc.RULES:
        g = pc.geom(dom, rule)
        assert pt.coords_exact(g) and pt.coord_rel(g, 2) == 0.0
    g = pc.geom(dom, "mid")
    assert pt.fp32_coords_exact(g)
    tiles = d.n // 192
    for t in (0, 1, tiles // 4, tiles // 3, tiles // 2 + 1, tiles - 2, tiles - 1):
        xm = pt.tile_anchor(g, "fp32-series", t)
        assert Fraction(xm) == g.x(Fraction(192 * t) + Fraction(191, 2)) and float(np.float32(xm)) == xm
    assert pt.defn_truth_rel("fp32-series", g) <= pt.U32 * (1 + 1e-4)
    assert pt.defn_truth_rel("fp64-series_exact", g) == 0.0
    assert not pt.coords_exact(pc.geom("unit-96M", "mid")) and not pt.fp32_coords_exact(pc.geom("unit-48M", "mid"))


def test_the_zero_tiles_hold_zero():
    for c in pc.TILE_CASES:
        if c.tag == "zero":
            g = pc.geom(c.dom, c.rule, c.i_begin, pt.tile_len(c.path))
            x0, x1 = g.x(0), g.x(g.count - 1)
            assert min(x0, x1) < 0 < max(x0, x1), c.id
            assert g.x_abs_min == 0.0 and min(abs(x0), abs(x1)) > 8 * abs(g.h)
    assert sum(c.tag == "zero" for c in pc.TILE_CASES) == 2 * len(pc.PATHS)


def test_case_lists_cover_what_they_claim():
    doms = {c.dom for c in pc.TILE_CASES}
    for path in pc.PATHS:
        mine = [c for c in pc.TILE_CASES if c.path == path]
        assert {"first", "middle", "last", "zero", "third", "x1"} <= {c.tag for c in mine}
        T = pt.tile_len(path)
        assert {c.count for c in pc.REM_CASES if c.path == path} == {1, 31, T - 1, T + 100}
        assert {(c.count, c.grid) for c in pc.SLICE_CASES if c.path == path and c.rule == "left"} == \
            {(T * k + r, gr) for k, r in ((69, 0), (69, 100), (261, 0)) for gr in (1, 2)}
    assert {"unit-1e9", "unit-1e10", "1e6", "1e12", "rev-1e12", "exact-0to4"} <= doms
    assert all(pc.DOMAINS[d].reverse_of for d in pc.DOMAINS if d.startswith("rev-"))
    assert max(c.count for c in pc.SLICE_CASES) == 261 * 384
    # h below ulp(x) on [1e12, 1e12 + 1024]; the far slices sit where the issue puts them
    assert pc.DOMAINS["1e12"].h < math.ulp(1e12)
    assert 2.0 ** 63 < pc.DOMAINS["far-1.2e19"].spec.a < 1.8446744e19 < pc.DOMAINS["far-2e19"].spec.a
    assert pc.DOMAINS["far-2e19"].h == 2.0 ** -26 and 96 * 2.0 ** -26 <= pt.HALF_SPAN_H


# ---------------------------------------------------------------------------- definition vs truth
@pytest.mark.parametrize("c", SERIES_TILES, ids=lambda c: c.id)
def test_definition_against_truth(c):
    """Pure host mathematics: what the rounded inputs of a series tile cost, within
    defn_truth_rel, on every single-tile case."""
    T = pt.tile_len(c.path)
    g = pc.geom(c.dom, c.rule, c.i_begin, T)
    D = pc.defined_sum(c.path, c.dom, c.rule, c.i_begin)
    S = pc.truth_sum(c.dom, c.rule, c.i_begin, T)
    err, bound = _rel(D, S), pt.defn_truth_rel(c.path, g)
    print(f"PI4TRUTH defn {c.id} {c.path} err={err:.4e} bound={bound:.4e}")
    assert err <= bound + 2.0 ** -300, (err, bound)      # (the closed form's own 2**-400)
    if pc.DOMAINS[c.dom].exact and c.path == "fp64-series_exact":
        assert bound == 0.0


def test_fp32_emulation_is_within_the_tile_bound_for_any_seed():
    """The host emulation of the fp32 tiles (exactly rounded fp32 operations) against the
    definition, with the seed exact and off by +-3e-7: inside tile_defn_rel, and the fp32
    tile's value moves by less than that bound when the seed does (e_m is formed from the s
    actually used)."""
    worst = 0.0
    for c in SERIES_TILES:
        if not c.path.startswith("fp32") or c.tag not in ("first", "middle", "zero", "x1"):
            continue
        g = pc.geom(c.dom, c.rule, c.i_begin, 192)
        D = pc.defined_sum(c.path, c.dom, c.rule, c.i_begin)
        bound = pt.tile_defn_rel(c.path, g)
        for sr in (0.0, 3e-7, -3e-7):
            err = _rel(pt.emulate_f32_tile(c.path, g, seed_rel=sr), D)
            assert err <= bound, (c.id, sr, err, bound)
            if c.path == "fp32-series":
                worst = max(worst, err)
    print(f"PI4TRUTH emulation fp32-series worst err={worst:.4e}")


# ---------------------------------------------------------------------------- caps on the bounds
def test_bounds_respect_their_caps():
    """Conditions the bounds must meet from their derivation alone.
    fp32 series tile against the definition: under 1e-9 relative (an eighth of the -8e-9 bias
    of the fp32 fold). fp32acc: its fold IS that fp32 fold (fmaf(s, 192 + t, acc)); the two
    fp32 roundings of the fold alone are 2 U32 = 1.2e-7, so no derived bound can come under
    U32 and none is claimed: the figure is asserted as what it is.
    series_exact on [0, 1]: single tile against the truth at or under 1e-15 relative, per
    point at or under 1.5 ulp."""
    for c in SERIES_TILES:
        g = pc.geom(c.dom, c.rule, c.i_begin, pt.tile_len(c.path))
        r = pt.tile_defn_rel(c.path, g)
        if c.path == "fp32-series":
            assert r < 1e-9 / 50, (c.id, r)
        elif c.path == "fp32acc-series":
            assert 2 * pt.U32 < r < 2 * pt.U32 * (1 + 1e-3), (c.id, r)
        elif c.path == "fp64-series_exact" and c.dom.endswith("unit-96M"):
            S = float(pc.truth_sum(c.dom, c.rule, c.i_begin, 384))
            assert pt.tile_truth_bound(c.path, g, S) <= 1e-15 * S, c.id
    for c in pc.WINDOW_CASES:
        if c.div == "series_exact" and c.dom.endswith("unit-96M"):
            g = pc.geom(c.dom, c.rule, c.i_begin, pc.WINDOW)
            vals, _ = pc.truth_values(c.dom, c.rule, c.i_begin, pc.WINDOW)
            ulps = pt.point_bound(c.path, g, vals) / np.array([math.ulp(v) for v in vals])
            assert ulps.max() <= 1.5, (c.id, ulps.max())


# ---------------------------------------------------------------------------- the bounds are not vacuous
def _tile_truth(c):
    T = pt.tile_len(c.path)
    g = pc.geom(c.dom, c.rule, c.i_begin, T)
    S = pc.truth_sum(c.dom, c.rule, c.i_begin, T)
    return g, S, pt.tile_truth_bound(c.path, g, float(S))


def _detect(name, cases, value_of):
    """value_of(case) -> (defective value, reference, absolute bound) or None; at least one
    case must exceed its bound."""
    hits, tried = [], 0
    for c in cases:
        r = value_of(c)
        if r is None:
            continue
        tried += 1
        v, ref, bound = r
        err = float(abs(MP.mpf(v) - ref))
        if err > bound:
            hits.append((err / bound, c.id))
    assert tried and hits, name
    ratio, cid = max(hits)
    print(f"PI4TRUTH defect {name}: detected by {len(hits)} of {tried} cases, "
          f"largest err/bound {ratio:.3g} at {cid}")


def test_defect_em_left_out_of_the_fp32_fold():
    """The fold of the fp32 tile done in fp32 (192 + sum e rounds to 192: e_m is dropped),
    against the definition at the GPU test's bound."""
    def value(c):
        if c.path != "fp32-series" or c.tag not in ("first", "middle", "zero", "third"):
            return None
        g = pc.geom(c.dom, c.rule, c.i_begin, 192)
        D = pc.defined_sum(c.path, c.dom, c.rule, c.i_begin)
        return pt.emulate_f32_tile(c.path, g, defect="fold32"), D, pt.tile_defn_rel(c.path, g) * float(D)
    _detect("e_m left out of the fp32 fold", SERIES_TILES, value)


def _shifted_sum(c, shift: Fraction):
    T = pt.tile_len(c.path)
    g = pc.geom(c.dom, c.rule, c.i_begin, T)
    return pt.progression_sum(g.x(0) + shift * Fraction(g.h), Fraction(g.h), T)


@pytest.mark.parametrize("name,shift", [("anchor at U/2 instead of (U-1)/2", Fraction(1, 2)),
                                        ("rule offset ignored", Fraction(-1, 2))])
def test_defect_misplaced_tile(name, shift):
    """Every sample of the tile half a step off (the midpoint anchored at U/2; a mid-rule
    launch run as a left one), against the truth."""
    def value(c):
        if shift < 0 and c.rule != "mid":
            return None
        g, S, bound = _tile_truth(c)
        return _shifted_sum(c, shift), S, bound
    _detect(name, pc.TILE_CASES, value)


def test_defect_one_sub_tile_centre_sign_flipped():
    """The 32 samples of the last sub-tile placed at -c0 instead of +c0 (they repeat the first
    sub-tile's, mirrored)."""
    def value(c):
        T = pt.tile_len(c.path)
        if T == 32:
            return None
        g, S, bound = _tile_truth(c)
        mid = Fraction(T - 1, 2)
        good = MP.fsum(pt.f_true(g.x(i)) for i in range(T - 32, T))
        bad = MP.fsum(pt.f_true(g.x(2 * mid - i)) for i in range(T - 32, T))
        return S - good + bad, S, bound
    _detect("sign of one sub-tile centre flipped", SERIES_TILES, value)


def test_defect_one_sample_counted_twice():
    def value(c):
        g, S, bound = _tile_truth(c)
        return S + pt.f_true(g.x(7)), S, bound
    _detect("one sample counted twice", pc.TILE_CASES, value)
    assert all(float(pt.f_true(_tile_truth(c)[0].x(7))) > _tile_truth(c)[2] for c in pc.TILE_CASES[:40])


def test_defect_e2_left_out_of_an_fp64_series_tile():
    """s (1 + e) in place of s (1 + e + e^2): the defined sum less s sum e_k^2 with the exact
    seed s = 1 / d_m (e_m = 0, e_k = -(2 x_m h k + h^2 k^2) s), against the definition at the
    GPU test's bound."""
    def value(c):
        if c.path not in ("fp64-series", "fp64-series_exact"):
            return None
        g = pc.geom(c.dom, c.rule, c.i_begin, 384)
        p = pt.defined_inputs(c.path, g)
        D = pc.defined_sum(c.path, c.dom, c.rule, c.i_begin)
        s = 1 / pt._mpq(p["dm"])
        e2 = MP.fsum((pt._mpq(2 * p["xm"] * p["h"] * k + p["h"] ** 2 * k * k) * s) ** 2
                     for k in pt._offsets(384))
        return D - s * e2, D, pt.tile_defn_rel(c.path, g) * float(D)
    _detect("e^2 left out of an fp64 series tile", SERIES_TILES, value)


def test_a_pair_constant_off_by_one_step_is_invisible_to_tile_sums():
    """Listed, not detected: one pair constant k_j off by one step in the e^2 term of ONE pair
    of one sub-tile changes an fp64 tile sum by 2 s ((k + 1)^2 - k^2) A'^2 <= 2 * 32 h^2, under
    an ulp of the sum at every admitted h. Per-point windows see the linear term's constants;
    this one is left at that."""
    h = 2.0e-6 / 192
    assert 2 * 32 * h * h < 0.5 * math.ulp(384.0 * 0.5)
