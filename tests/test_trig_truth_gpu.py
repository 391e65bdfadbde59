"""The sin and train-velocity kernels against the truth (utils/trig_truth.py: mpmath at 200
bits, closed-form sums), with bounds derived from the kernels' own operations: per point, per
single tile (the packed-fp32 tiles' first per-tile check), slices and whole ranges, plans,
reversed intervals and far angles. Cases: trig_truth_cases.py (their CPU-side conditions:
test_trig_truth_cpu.py). Every test prints its measured error next to the bound
(`TRIGTRUTH ...` lines: profiles/r11/trig_truth.md is made of them); the asserts use the
derived bounds only.

Far angles: beyond kTrigSeriesMaxN = 2**31 - 2**16 quadrants a launch runs the per-sample
tiles. Before that limit existed the series tiles took their quadrant from a saturated
integer conversion there, and the far cases below failed by O(1) per sample:
    test_point_values_against_truth[sin-3.4e9-left-i0-series]
    AssertionError: (3137, -0.9999999973532341, 7.275666097620451e-05, 1.0000727540142103, ...)
(sample, kernel value, true value, error; 42 such cases on the parent commit's build, all
passing here: profiles/r11/trig_truth.md).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import riemann_exact_cases as xc
import trig_truth_cases as tc
from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import trig_truth as tt

pytestmark = pytest.mark.gpu
MP = tt.MP
MIRROR = {"left": "right", "mid": "mid", "right": "left"}


def _record(kind, cid, path, err, bound):
    print(f"TRIGTRUTH {kind} {cid} {path} err={err:.4e} bound={bound:.4e} "
          f"ratio={err / bound if bound > 0 else float('inf'):.4f}")


def _errs(v: np.ndarray, exact: list) -> np.ndarray:
    return np.array([float(abs(MP.mpf(float(a)) - e)) for a, e in zip(v, exact)])


def test_tile_lengths_are_the_codes(cuda, native):
    """T of every path, read from the dispatcher: the single-tile launches below rely on it."""
    for dom in ("sin-pm40", "train-56"):
        d = tc.DOMAINS[dom]
        s = d.spec
        args = (s.native_id, s.a, d.h, 0.0, 0, d.n, [], s.p0, s.p1)
        for dt in (native.DType.fp64, native.DType.fp32):
            assert native.riemann_tile_len(*args, dt, native.DivMode.series) == tt.SERIES_TILE[d.name]
            assert native.riemann_tile_len(*args, dt, native.DivMode.ieee) == tt.IEEE_TILE


# ---------------------------------------------------------------------------- per point
def _point_bounds(c, div, vals, exact):
    d = tc.DOMAINS[c.dom]
    g = tc.geom(c.dom, c.rule, c.i_begin, c.count)
    trig, _ = tc.truth_trig(c.dom, c.rule, c.i_begin, c.count)
    series = tc.runs_series(g, div)
    T = tt.SERIES_TILE[d.name] if series else tt.IEEE_TILE
    full = (c.count // T) * T
    fast = np.zeros(c.count, dtype=bool)
    if not series and d.exact:   # which per-sample tiles run the fdlibm kernels (exact angles)
        w = 1.0 if d.name == "sin" else 1.0 / d.spec.p0
        for t0 in range(0, full, T):
            fast[t0:t0 + T] = tt.ieee_tile_fast(float(g.x(t0)) * w, float(g.x(t0 + T - 1)) * w)
    lib = np.array([tt.ieee_point_bound(g, float(t), bool(f)) for t, f in zip(trig, fast)])
    if series:
        lib[:full] = tt.series_value_point_bound(g)
    return lib, ("series" if series else "ieee")


@pytest.mark.parametrize("div", ["series", "ieee"])
@pytest.mark.parametrize("c", tc.POINT_CASES, ids=lambda c: c.id)
def test_point_values_against_truth(cuda, c, div):
    """Every sample of a 4096-sample window, exactly as the hot tile computes it, against the
    true f: absolute error over the derived bound (the series tiles' constant bound; the
    per-sample tiles' 1 or 2 ulp of the value; the coordinate term where coordinates round;
    a partial last tile is summed point by point with the library)."""
    d = tc.DOMAINS[c.dom]
    v = kernels.point_values(d.spec, d.n, rule=c.rule, div=div, i_begin=c.i_begin,
                             n_local=c.count).cpu().numpy()
    vals, exact = tc.truth_values(c.dom, c.rule, c.i_begin, c.count)
    bound, path = _point_bounds(c, div, vals, exact)
    err = _errs(v, exact)
    k = int(np.argmax(err / bound))
    _record("point", c.id, f"fp64-{div}>{path}", err[k], bound[k])
    assert (err <= bound).all(), (k, v[k], vals[k], err[k], bound[k])


# ---------------------------------------------------------------------------- single tiles
@pytest.mark.parametrize("c", tc.TILE_CASES, ids=lambda c: c.id)
def test_single_tile_against_truth(cuda, c):
    """grid = 1, n_local = T: partials[0] is one lane's one tile (fp64 and packed-fp32 series
    tiles, fp64 and fp32 per-sample tiles) against the closed-form sum of its samples."""
    d = tc.DOMAINS[c.dom]
    T = tc.tile_of(d, c.div)
    p = kernels.riemann_partials(d.spec, d.n, c.rule, c.dtype, c.div, grid=1, i_begin=c.i_begin,
                                 n_local=T)
    got = float(p[0].item())
    err = float(abs(MP.mpf(got) - tc.truth_sum(c.dom, c.rule, c.i_begin, T)))
    bound = tc.tile_bound(c)
    g = tc.geom(c.dom, c.rule, c.i_begin, T)
    div, fp32 = tc.effective_path(g, c.dtype, c.div)
    _record("tile", c.id, f"{'fp32' if fp32 else 'fp64'}-{div}", err, bound)
    assert err <= bound, (got, err, bound)


# ---------------------------------------------------------------------------- slices, ranges
def _slice_bound(c, grid):
    g = tc.geom(c.dom, c.rule, c.i_begin, c.count)
    div, fp32 = tc.effective_path(g, c.dtype, c.div)
    return g, div, fp32, tt.launch_value_bound(g, div, fp32, grid)


@pytest.mark.parametrize("c", tc.SLICE_CASES, ids=lambda c: c.id)
def test_slices_and_ranges_against_truth(cuda, c):
    """h * sum of multi-tile slices (T k + r, odd starts, grids 1, 3 and the default, the
    three rules), of the workload's own N = 1e9 launches, of slices beyond 2**32 and of far
    ranges, against h * the closed form."""
    d = tc.DOMAINS[c.dom]
    grid = c.grid or kernels.default_grid()
    got = float(kernels.riemann(d.spec, d.n, c.rule, c.dtype, c.div, grid=grid,
                                i_begin=c.i_begin, n_local=c.count).item())
    g, div, fp32, bound = _slice_bound(c, grid)
    want = MP.mpf(g.h) * tc.truth_sum(c.dom, c.rule, c.i_begin, c.count)
    err = float(abs(MP.mpf(got) - want))
    _record("slice", c.id, f"{'fp32' if fp32 else 'fp64'}-{div}", err, bound)
    assert err <= bound, (got, float(want), err, bound)


@pytest.mark.parametrize("c", tc.PLAN_CASES, ids=lambda c: c.id)
def test_plans_against_truth(cuda, c):
    """Through Integrator (series_exact request: the default): chained and multi-step
    batches, graphs off and on, three steps each. Every step within the bound of the truth,
    all steps bitwise equal, and the plan reports the division that ran (far: ieee)."""
    d = tc.DOMAINS[c.dom]
    n = c.n or d.n
    it = Integrator(d.spec, n=n, rule="left", dtype=c.dtype, block=c.block,
                    multistep=c.multistep)
    g = tt.geometry(d.spec, n, "left", 0, n)
    div, fp32 = tc.effective_path(g, c.dtype, "series")
    assert str(it.plan.effective_div).split(".")[-1] == div
    assert it.describe()["div"] == div
    bound = tt.launch_value_bound(g, div, fp32, it.plan.grid, it.plan.block)
    want = tt.true_value(d.spec, n, "left", 0, n)
    vals = []
    for graphs in (False, True):
        it.run_steps(3, pipeline=False, graphs=graphs)
        vals += [it.plan.host_result(it.plan.host_index_of(k, graphs)) for k in range(3)]
    err = float(abs(MP.mpf(vals[0]) - want))
    _record("plan", c.id, f"{'fp32' if fp32 else 'fp64'}-{div}", err, bound)
    assert len(set(vals)) == 1, vals
    assert err <= bound, (vals[0], float(want), err, bound)


# ---------------------------------------------------------------------------- reversed
REVERSED = [("sin-rev-pm40", "sin-pm40"), ("sin-rev-coarse", None), ("train-rev-56", "train-56"),
            ("train-rev-coarse", "train-56-coarse")]


@pytest.mark.parametrize("div", ["series", "ieee"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("rev,fwd", REVERSED, ids=[r for r, _ in REVERSED])
def test_reversed_interval_against_truth_and_forward(cuda, rev, fwd, dtype, div):
    """b < a (h < 0): the value is within the bound of the truth, and where the forward
    family exists it agrees with the negated forward value under the mirrored rule (the same
    samples: x'_j = b - (j + off') |h| is x_{n-1-j} of the rule with 1 - off'). The code
    guarantees the BOUND-WISE relation only: the two launches visit the samples of a tile in
    opposite order (the pair +k / -k additions swap, the tiles are dealt from the other end),
    so the sums round differently and are not bitwise negatives of each other."""
    for rule in tc.RULES:
        d = tc.DOMAINS[rev]
        grid = 3
        got = float(kernels.riemann(d.spec, d.n, rule, dtype, div, grid=grid).item())
        c = tc.SliceCase(rev, rule, 0, d.n, dtype, div, grid)
        g, edv, fp32, bound = _slice_bound(c, grid)
        want = MP.mpf(g.h) * tc.truth_sum(rev, rule, 0, d.n)
        err = float(abs(MP.mpf(got) - want))
        _record("reversed", c.id, f"{'fp32' if fp32 else 'fp64'}-{edv}", err, bound)
        assert err <= bound, (got, float(want), err, bound)
        if fwd is None:
            continue
        f = tc.DOMAINS[fwd]
        assert f.n == d.n and f.spec.a == d.spec.b and f.spec.b == d.spec.a
        cf = tc.SliceCase(fwd, MIRROR[rule], 0, f.n, dtype, div, grid)
        fwant = MP.mpf(f.h) * tc.truth_sum(fwd, MIRROR[rule], 0, f.n)
        assert abs(fwant + want) <= MP.mpf(2) ** -150 * max(1, abs(want))   # the same samples
        fgot = float(kernels.riemann(f.spec, f.n, MIRROR[rule], dtype, div, grid=grid).item())
        assert abs(got + fgot) <= bound + _slice_bound(cf, grid)[3], (got, fgot)


REV_TABLE = [c for c in xc.TABLE_CASES if c.rank is None and c.tab == "t200" and c.k in (3, 6)]
REV_POLY = [c for c in xc.POLY_CASES if c.rank is None and c.coef == xc.DEG3]


@pytest.mark.parametrize("c", REV_TABLE + REV_POLY, ids=lambda c: "rev-" + c.id)
def test_reversed_table_and_polynomial_are_exact(cuda, c):
    """The table and a degree-3 polynomial on dyadic inputs over the reversed interval: the
    samples are the forward ones of the mirrored rule, every operation is still exact (the
    table's negative-h tiles take the one-segment line or the per-sample fallback), so the
    value is bitwise the negated integer reference of the mirrored forward case."""
    table = isinstance(c, xc.TableCase)
    fwd = (xc.table_spec if table else xc.poly_spec)(c)
    n = xc.n_of(c) if table else xc.poly_n(c)
    spec = dataclasses.replace(fwd, a=fwd.b, b=fwd.a)
    assert (spec.b - spec.a) / n == -(2.0 ** -c.k)
    ref = (xc.table_ref if table else xc.poly_ref)(c._replace(rule=MIRROR[c.rule]))
    got = float(kernels.riemann(spec, n, c.rule, c.dtype, c.div, grid=c.grid,
                                fused=getattr(c, "fused", True)).item())
    assert got == -ref, (got, -ref)
