"""The integer references of the exact Riemann / 2-D field tests, checked without a GPU:
against fractions.Fraction at random points, the admissibility of every case the GPU tests
launch (budgets from the inputs alone, the tile paths the table cases reach), the custom-table
plumbing, and the host engine on the same cases, which must return the reference's bits."""
from __future__ import annotations

import math
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

import riemann_exact_cases as rc
from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.utils import exact_riemann as xr


# ------------------------------------------------------------------------------ references
def _frac_table(T, x: Fraction) -> Fraction:
    s = min(max(math.floor(x), 0), len(T) - 2)
    return T[s] + (T[s + 1] - T[s]) * (x - s)


def test_table_reference_against_fractions():
    rng = random.Random(1)
    T = [int(v) for v in rc.table("t200")]
    for _ in range(300):
        k = rng.choice(rc.KS + (10,))
        off2 = rng.choice((0, 1, 2))
        a_num = rng.randrange(-8 << (k + 1), 4 << (k + 1))      # from 8 below the table
        i = rng.randrange(0, 210 << k)                            # to past its end
        x = Fraction(a_num + 2 * i + off2, 1 << (k + 1))
        got = int(xr.exact_table_samples(rc.table("t200"), a_num, k, off2, i, 1)[0])
        assert Fraction(got, 1 << (k + 1)) == _frac_table(T, x), (k, off2, a_num, i)
    # a sum is the sum of its samples, across both ends of the table
    k, a_num = 5, rc.a_num_of(5)
    n = 204 << k
    want = sum(_frac_table(T, Fraction(a_num + 2 * i + 1, 1 << (k + 1))) for i in range(n))
    assert Fraction(xr.exact_table_sum(rc.table("t200"), a_num, k, 1, 0, n), 1 << (k + 1)) == want
    assert (xr.exact_table_sum(rc.table("t200"), a_num, k, 1, 0, 1000)
            + xr.exact_table_sum(rc.table("t200"), a_num, k, 1, 1000, n - 1000)
            == xr.exact_table_sum(rc.table("t200"), a_num, k, 1, 0, n))


def test_poly_reference_against_fractions():
    rng = random.Random(2)
    for _ in range(300):
        deg = rng.randrange(0, 4)
        coef = [rng.randrange(-7, 8) for _ in range(deg + 1)] + [0] * rng.randrange(0, 3)
        k = rng.choice((3, 6, 7, 10))
        off2 = rng.choice((0, 1, 2))
        a_num = rng.randrange(-16 << (k + 1), 16 << (k + 1))
        i = rng.randrange(0, 1 << 12)
        x = Fraction(a_num + 2 * i + off2, 1 << (k + 1))
        got = int(xr.exact_poly_samples(coef, a_num, k, off2, i, 1)[0])
        want = sum(c * x ** j for j, c in enumerate(coef))
        assert Fraction(got, 1 << xr.poly_unit_bits(coef, k)) == want, (coef, k, a_num, i)
    c = rc.POLY_CASES[0]
    tot = xr.exact_poly_sum(c.coef, rc.poly_a_num(c), c.k, 1, 5, 300)
    want = sum(sum(cj * Fraction(rc.poly_a_num(c) + 2 * i + 1, 1 << (c.k + 1)) ** j
                   for j, cj in enumerate(c.coef)) for i in range(5, 305))
    assert Fraction(tot, 1 << xr.poly_unit_bits(c.coef, c.k)) == want


def test_table2d_reference_against_fractions():
    rng = random.Random(3)
    T = rc.field("f37x53")
    ny, nx = T.shape
    for _ in range(300):
        rx, ry = rng.choice((rc.Q, rc.E8, rc.HALF, rc.ONE, rc.FOUR)), rng.choice(
            (rc.Q, rc.E8, rc.T8, rc.HALF, rc.ONE, rc.T2))
        gx, gy = xr.table2d_grid_of(nx, rx), xr.table2d_grid_of(ny, ry)
        r, c = rng.randrange(gy), rng.randrange(gx)
        x = Fraction((2 * c + 1) * rx[0], 1 << (rx[1] + 1))
        y = Fraction((2 * r + 1) * ry[0], 1 << (ry[1] + 1))
        ix, iy = min(math.floor(x), nx - 2), min(math.floor(y), ny - 2)
        fx, fy = x - ix, y - iy
        top = int(T[iy, ix]) + (int(T[iy, ix + 1]) - int(T[iy, ix])) * fx
        bot = int(T[iy + 1, ix]) + (int(T[iy + 1, ix + 1]) - int(T[iy + 1, ix])) * fx
        want = top + (bot - top) * fy
        # one sample: the row's sum over columns [0, c] minus the sum over [0, c)
        got = xr.exact_table2d_sum(T, rx, ry, c + 1, gy, r, r + 1)
        if c:
            got -= xr.exact_table2d_sum(T, rx, ry, c, gy, r, r + 1)
        assert Fraction(got, 1 << (rx[1] + ry[1] + 2)) == want, (rx, ry, r, c)
    with pytest.raises(ValueError):
        xr.table2d_grid_of(53, rc.T8)     # 3 does not divide 52 cells


def test_census_counts_by_hand():
    """A flat table of 3 entries at k = 6 (64 samples per segment), left rule from x = -1/2:
    tile 0 straddles x = 0 inside the clamped first segment (one), tile 1 the knot at 1
    (kink), tile 2 the table's end, where the last segment goes on (one)."""
    t = np.array([1, 2, 4], dtype=np.int64)
    assert xr.table_tile_census(t, -64, 6, 0, 0, 3 * 64 + 5) == dict(one=2, kink=1, coarse=0, rem=5)
    # h = 1/8: a tile spans 8 segments of a long table
    assert xr.table_tile_census(rc.table("t200"), 0, 3, 0, 0, 128)["coarse"] == 2
    # aligned: integer a, left rule, k >= 7 — no tile straddles a knot
    assert xr.table_tile_census(rc.table("t200"), 0, 7, 0, 0, 199 * 128)["kink"] == 0


# ------------------------------------------------------------------------------ admissibility
@pytest.mark.parametrize("c", rc.TABLE_CASES + list(rc.PLAN_CASES.values()) + [rc.LOOPBACK_CASE],
                         ids=lambda c: c.id)
def test_table_case_within_budget(c):
    b = rc.table_budget(c)
    assert b["fp64"] < xr.F64_BITS, b
    if c.dtype == "fp32":
        assert b["fp32"] < xr.F32_BITS, b
    n = rc.n_of(c)
    assert n % 64 not in (0,) and n <= 600_000
    spec = rc.table_spec(c)
    assert (spec.b - spec.a) / n == 2.0 ** -c.k            # the step the kernels form
    assert spec.a == rc.a_num_of(c.k) * 2.0 ** -(c.k + 1)
    assert spec.a < -2.5 and spec.b > len(spec.table) - 1 + 2.25
    assert (rc.a_num_of(c.k) % (128 << 1)) != 0              # a is no multiple of 64 h


def test_table_cases_reach_every_tile_path():
    series = [c for c in rc.TABLE_CASES if c.div == "series"]
    tot = {p: sum(rc.table_census(c)[p] for c in series) for p in ("one", "kink", "coarse")}
    assert min(tot.values()) >= 8, tot
    # every fp32 case list on its own has kinked tiles, and each list's cases are all fp32 series
    for lst in (rc.FP32_WHOLE, rc.FP32_SLICES, [rc.PLAN_CASES["fp32"]]):
        assert lst and sum(rc.table_census(c)["kink"] for c in lst) >= 8
    for k in rc.KS:   # every step of the sweep runs fp32 x series, all three rules
        assert {c.rule for c in rc.FP32_WHOLE if c.k == k and c.tab == "t200"} == set(rc.RULES)
    for c in rc.FP32_WHOLE:
        if c.k >= 6:
            assert rc.table_census(c)["kink"] > 0, c.id
    # the grids: a remainder inside a wave, q = 0, more tiles than lanes
    assert {c.grid for c in series} == set(rc.GRIDS)
    assert {c.fused for c in series} == {True, False}
    # slices start on odd samples too
    for lst in ([c for c in rc.TABLE_CASES if c.rank is not None and c.tab == t]
                for t in ("t200", "t2048")):
        assert sum(rc.span(c)[0] % 2 for c in lst) >= 2
    assert len(rc.TABLE_CASES) <= 60


def _kink_slope_sums(c) -> dict:
    i0, m = rc.span(c)
    return xr.table_kink_slope_sums(rc.table(c.tab), rc.a_num_of(c.k), c.k, rc.OFF2[c.rule], i0, m)


@pytest.mark.parametrize("c", [c for c in rc.TABLE_CASES if c.div == "series" and c.k >= 5]
                         + list(rc.PLAN_CASES.values()) + [rc.LOOPBACK_CASE], ids=lambda c: c.id)
def test_kinked_cases_can_see_a_wrong_kink_weight(c):
    """A kinked tile's sum is linear in its slope change, with a weight set by where the knot
    falls in the tile; a wrong weight shows in a launch's sum only through the slope changes
    summed per knot position. Every kink-bearing case has such a sum that is not zero (at
    k = 6 there is one position and the sum telescopes to last slope minus first slope: the
    tables' first slopes are not zero, their flat tails are)."""
    sums = _kink_slope_sums(c)
    assert rc.table_census(c)["kink"] == 0 or any(sums.values()), sums
    if c.k >= 6 and c.rank is None:
        assert any(sums.values())


def test_kink_slope_sums_by_hand():
    t = np.array([0, 1, 3, 3, 0], dtype=np.int64)      # slope changes 1, -2, -3 at knots 1, 2, 3
    # k = 6, left rule from x = 1/2: every tile has its knot 32 steps (64 half steps) in
    got = xr.table_kink_slope_sums(t, 64, 6, 0, 0, 3 * 64)
    assert got == {64: 1 - 2 - 3}
    assert xr.table_kink_slope_sums(t, 0, 6, 0, 0, 3 * 64) == {}   # aligned: no kinked tile


@pytest.mark.parametrize("c", rc.POLY_CASES + [rc.POLY_PLAN_CASE], ids=lambda c: c.id)
def test_poly_case_within_budget(c):
    b = rc.poly_budget(c)
    assert b["fp64"] < xr.F64_BITS, b
    if c.dtype == "fp32":
        assert b["fp32"] < xr.F32_BITS, b
    assert all(abs(v) <= 7 for v in c.coef)
    spec = rc.poly_spec(c)
    assert (spec.b - spec.a) / rc.poly_n(c) == 2.0 ** -c.k
    assert rc.poly_n(c) % 64 != 0


def test_poly_cases_cover_every_bucket():
    f64 = [c for c in rc.POLY_CASES if c.dtype == "fp64"]
    assert {len(c.coef) for c in f64 if c.div == "series"} >= {3, 4, 6, 7, 8, 9}
    assert {len(c.coef) for c in f64 if c.div == "ieee"} >= {3, 4, 8, 9}
    # at least 2 tile rounds per lane at one workgroup of 256 lanes for the degree-2 case
    assert rc.poly_n(rc.POLY_PLAN_CASE) // 64 >= 2 * 256


@pytest.mark.parametrize("c", rc.FIELD_CASES, ids=lambda c: c.id)
def test_field_case_within_budget(native, c):
    assert rc.field_budget(c) < xr.F64_BITS
    ny, nx = rc.field(c.tab).shape
    gx, gy = rc.field_grid(c)
    X, Y = float(nx - 1), float(ny - 1)
    assert (nx - 1) / X == 1.0 and X / gx == c.rx[0] * 2.0 ** -c.rx[1]
    assert (ny - 1) / Y == 1.0 and Y / gy == c.ry[0] * 2.0 ** -c.ry[1]
    assert native.table2d_path(nx, ny, X, Y, gx, gy, 0, gy) == c.path
    if c.path == "stream":   # partial workgroups in x (256 columns) and y
        assert gx % 256 != 0
        assert native.table2d_multistep_phases(nx, ny, X, Y, gx, gy, 0, gy, 0,
                                               rc.FIELD_STEPS, 16) == 16


def test_field_reference_rows_add_up():
    c = rc.FIELD_CASES[1]
    gx, gy = rc.field_grid(c)
    parts = [xr.exact_table2d_sum(rc.field(c.tab), c.rx, c.ry, gx, gy, r0, r1)
             for r0, r1 in rc.field_cuts(gy)]
    assert sum(parts) == xr.exact_table2d_sum(rc.field(c.tab), c.rx, c.ry, gx, gy, 0, gy)
    assert all(r0 % 2 == 1 for r0, _ in rc.field_cuts(gy)[1:])


# ------------------------------------------------------------------------------ emulation
def _f32(v, what):
    """v as the packed-fp32 path would hold it: it must already be an fp32 value."""
    v = np.asarray(v, dtype=np.float64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v), f"{what} rounds in fp32"
    return v


def _emulate_table_series(c) -> tuple[float, int]:
    """The segment-line tiles of Table / TableF32 (integrands.hpp, integrands_f32.hpp) on the
    case's samples, operation by operation in numpy fp64 — every product and sum formed in
    the kernel's order, every value the fp32 path rounds to fp32 checked to be one already —
    plus the remainder samples. Returns (h * sum, widest fp32 pair accumulator in bits)."""
    T = np.asarray(rc.table(c.tab), dtype=np.float64)
    nseg = len(T) - 1
    k, h, f32 = c.k, 2.0 ** -c.k, c.dtype == "fp32"
    cast = _f32 if f32 else (lambda v, what: np.asarray(v, dtype=np.float64))
    a, off = rc.a_num_of(k) * 2.0 ** -(k + 1), rc.OFF2[c.rule] / 2
    i0, n = rc.span(c)
    seg = lambda t: np.clip(t, 0.0, nseg - 1.0).astype(np.int64)  # noqa: E731

    def point(t):  # Table::point / TableF32::pointf
        i = seg(t)
        fr = cast(t - i, "fr")
        return cast((T[i + 1] - T[i]) * fr + T[i], "point")

    tiles = n // 64
    xm = (i0 + off + 64.0 * np.arange(tiles) + 31.5) * h + a
    lo, hi = seg(xm - 31.5 * h), seg(xm + 31.5 * h)
    kj = np.arange(16) + 0.5
    total, widest = 0.0, 0.0
    line = hi <= lo + 1
    if line.any():
        x, l, kinked = xm[line], lo[line], (hi == lo + 1)[line]
        v0, v1 = T[l], T[l + 1]
        v2 = T[np.minimum(l + 2, nseg)]
        d0 = v1 - v0
        vm, D = d0 * (x - l) + v0, d0 * h
        dD = np.where(kinked, ((v2 - v1) - d0) * h, 0.0)
        kk = np.where(kinked, ((l + 1.0) - x) * (1.0 / h), 0.0)
        Df, dDf = cast(D, "Df"), cast(dD, "dDf")
        for c0 in (-16.0, 16.0):
            vc, r = cast(c0 * D + vm, "vc"), cast(c0 - kk, "r")
            for sign in (1.0, -1.0):
                g = cast(sign * kj[None, :] * Df[:, None] + vc[:, None], "g")
                over = np.maximum(cast(r[:, None] + sign * kj[None, :], "r + k"), 0.0)
                g = np.where(kinked[:, None], cast(over * dDf[:, None] + g, "g with kink"), g)
                acc = cast(np.cumsum(g, axis=1), "pair accumulator")
                widest = max(widest, float(np.abs(acc).max()))
                total += float(acc[:, -1].sum())
    if (~line).any():   # coarse: per sample, two chains of 32
        x0 = xm[~line] - 31.5 * h
        v = point(x0[:, None] + np.arange(64)[None, :] * h)
        for chain in (v[:, 0::2], v[:, 1::2]):
            acc = cast(np.cumsum(chain, axis=1), "coarse chain")
            widest = max(widest, float(np.abs(acc).max()))
            total += float(acc[:, -1].sum())
    rem = np.arange(tiles * 64, n)
    if len(rem):
        total += float(point((i0 + off + rem) * h + a).sum())
    assert abs(total) * 2.0 ** (k + 1) < 2.0 ** 53
    return total * h, math.log2(widest * 2.0 ** (k + 1)) if widest else 0.0


@pytest.mark.parametrize("c", [c for c in rc.TABLE_CASES if c.div == "series"]
                         + list(rc.PLAN_CASES.values()), ids=lambda c: c.id)
def test_emulated_series_tiles_are_exact(c):
    """What the budgets promise, shown on the cases themselves: the kernels' own arithmetic
    forms no value that rounds — in fp32 where the packed path holds it in fp32 — and its sum
    is the integer reference, bit for bit. So a GPU mismatch is the kernel's."""
    got, bits = _emulate_table_series(c)
    assert got == rc.table_ref(c)
    if c.dtype == "fp32":
        # the widest fp32 accumulator, in bits of the unit: inside the budget's bound
        assert bits <= rc.table_budget(c)["fp32"] < xr.F32_BITS


# ------------------------------------------------------------------------------ plumbing
def test_custom_table_spec():
    tab = [float(v) for v in rc.table("t200")]
    spec = integrands.table(tab, a=-1.5, b=201.25)
    assert spec.native_table() == tab and spec.table == tuple(tab)
    assert integrands.table().native_table() == list(integrands.fixtures.profile_table())
    assert integrands.table().table == ()
    x = torch.tensor([-1.5, 0.0, 0.5, 17.25, 198.5, 199.0, 201.0], dtype=torch.float64)
    want = [float(_frac_table([int(v) for v in tab], Fraction(float(v)))) for v in x]
    assert spec.f_torch(x).tolist() == want
    # analytic(): the exact trapezoid value of the given table, end segments extended
    T = [int(v) for v in tab]
    inside = sum(Fraction(T[i] + T[i + 1], 2) for i in range(199))
    left = Fraction(3, 2) * (_frac_table(T, Fraction(-3, 2)) + T[0]) / 2
    right = Fraction(9, 4) * (_frac_table(T, Fraction(805, 4)) + T[199]) / 2
    assert spec.analytic() == pytest.approx(float(inside + left + right), rel=1e-14)
    assert spec.analytic(0.0, 199.0) == pytest.approx(float(inside), rel=1e-14)
    with pytest.raises(ValueError):
        integrands.table([1.0])


def test_table_tensor_cache_is_per_table():
    """ops.kernels caches the device copy of a spec's table: per table, not per device alone."""
    from cuda_v_mpi_amd.ops import kernels

    a = integrands.table([1.0, 2.0, 3.0])
    b = integrands.table([4.0, 5.0, 6.0, 7.0])
    dev = torch.device("cpu")
    saved = dict(kernels._TABLE_CACHE)
    try:
        ta, tb = kernels._table_tensor(a, dev), kernels._table_tensor(b, dev)
        assert ta.tolist() == [1.0, 2.0, 3.0] and tb.tolist() == [4.0, 5.0, 6.0, 7.0]
        assert kernels._table_tensor(a, dev) is ta
        assert kernels._table_tensor(integrands.table(), dev).numel() == 1801
    finally:
        kernels._TABLE_CACHE.clear()
        kernels._TABLE_CACHE.update(saved)


# ------------------------------------------------------------------------------ host engine
@pytest.mark.parametrize("c", [c for c in rc.TABLE_CASES if c.dtype == "fp64" and c.div == "series"],
                         ids=lambda c: c.id)
@pytest.mark.parametrize("threads", [1, 3])
def test_host_engine_table_exact(c, threads):
    """The host engine (per sample, fp64, vector lanes and compensated block sums) on the
    table cases: every operation exact, so the reference's bits. One rank's slice through
    slice-of-7 decomposition where the case is a slice."""
    it = Integrator(rc.table_spec(c), n=rc.n_of(c), rule=c.rule, backend="host", threads=threads)
    if c.rank is None:
        assert it.run().value == rc.table_ref(c)
    else:
        i0, m = rc.span(c)
        assert it._m.host_riemann(it._cfg, i0, m, it._pool) == rc.table_ref(c)


@pytest.mark.parametrize("c", [c for c in rc.POLY_CASES if c.div == "ieee" and c.dtype == "fp64"],
                         ids=lambda c: c.id)
def test_host_engine_poly_exact(c):
    it = Integrator(rc.poly_spec(c), n=rc.poly_n(c), rule=c.rule, backend="host", threads=2)
    i0, m = rc.poly_span(c)
    assert it._m.host_riemann(it._cfg, i0, m, it._pool) == rc.poly_ref(c)
