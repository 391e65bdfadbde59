"""Every velocity-table kernel path against an exact rational truth (utils/table_truth.py):
point values and launch values of the segment-line tiles (line, kink and coarse branches) and of
the per-sample form, fp64 and packed fp32, and every element of interp_fill, within bounds
derived from the kernels' own operations. Cases: table_truth_cases.py (their CPU-side conditions,
the branch census and the defect tests: test_table_truth_cpu.py). Every case first asserts the
path and tile length it runs and prints its measured error next to the bound (`TABLETRUTH ...`
lines: profiles/r18/table_truth.md is made of them); the asserts use the derived bounds only.

There is no fp32 point kernel: the fp32 tiles are observed through single-tile launches at grid 1.

On the parent commit TableF32::pointf (the fp32 per-sample form: the ieee tiles, the coarse
branch and the remainder loop of the fp32 series tiles) formed its slope from fp32-rounded
entries, fmaf(fl32(v1) - fl32(v0), fr, fl32(v0)): an error of 2**-24 |v| in the slope, multiplied
by fr = x - lo, which is unbounded on the two extrapolating end segments. The `ends` table's
first segment (87.1, 87.100001) rounds to one float, so the parent build returns the constant
87.1 there. By the exactly rounded fp32 emulation of that form (emulate_tile(f32_slope=True);
the parent's build itself was not run), the launches that miss their bound on the parent are
    test_launches_against_truth[far-3e9-fp32-ieee-g1-*]        x = -3e9: every sample 87.1 where
                                                               87.1 - 3e3 is true; the sum is off
                                                               by 1.59e6, 8.6e5 bounds
    test_launches_against_truth[far-3e9-fp32-series-g1-*]      through its 17 remainder samples:
                                                               off by 5.1e4, 1.5e4 bounds
    test_launches_against_truth[far-neg-2p60-fp32-ieee-g1-*]   x = -2**60: off by 2.9e14, 8.8e5
                                                               bounds
    test_launches_against_truth[far-neg-2p60-fp32-series-g1-*] its 63 remainder samples: 1.2e5
                                                               bounds
Where the entries do not round together the old form stays inside: far+3e9-sub, far-1e15 and
far-2p60 sit on the last segment (1e-3, 250.7; slope error 2**-24 250 against a bound in units of
250 |x|), ends-beyond and rev-ends reach x = -20 only. With the slope subtracted in fp64 and
converted once, all pass.

One more case failed on the parent, on the device: test_points_against_truth[rev-mix-series]
returned -43.995 for sample 127 where 1.4224 is true. Table::series_point, the point kernel's
copy of the tile, took the kink branch for every tile with hi != lo, so a reversed tile across a
knot (h < 0: hi = lo - 1), which tile_acc sums per sample, was evaluated with the knot of segment
lo + 1. Launch values were never affected; series_point now branches as tile_acc does.

The fp64 launch paths, the fp32 line and kink tiles (which form d in fp64) and interp_fill run
the same code on both builds and show no defect: "exact for any h" holds for them as derived in
table_truth._terms, h = 0 and h < 0 included.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest
import torch

import table_truth_cases as tc
from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import table_truth as tt

pytestmark = pytest.mark.gpu


def _record(kind, cid, path, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"TABLETRUTH {kind} {cid} {path} err={err:.4e} bound={bound:.4e} ratio={ratio:.4f}")


def _err(got: float, want: Fraction) -> float:
    return float(abs(Fraction(got) - want)) if np.isfinite(got) else float("inf")


def _args(g):
    return (4, g.a, g.h, float(g.off), g.i_begin, g.count, [], 0.0, 0.0)


def _assert_path(native, dtype, div, g, path):
    assert tt.effective_path(dtype, div) == path
    eff = native.riemann_effective_div(*_args(g), getattr(native.DType, dtype),
                                       getattr(native.DivMode, div))
    assert f"{dtype}-{str(eff).split('.')[-1]}" == path
    T = native.riemann_tile_len(*_args(g), getattr(native.DType, dtype), getattr(native.DivMode, div))
    assert T == tt.tile_len(path)


# ---------------------------------------------------------------------------- per point
@pytest.mark.parametrize("cid,div", tc.POINT_CASES, ids=lambda v: v)
def test_points_against_truth(cuda, native, cid, div):
    """Up to 4096 values of point_values, fp64 series (series_point: the tile's own operations
    per sample, whichever branch the tile takes) and ieee, each within its bound of v(x_i)."""
    c = tc.GEOMS[cid]
    g = c.geometry(tc.point_count(c))
    path = f"fp64-{div}"
    _assert_path(native, "fp64", div, g, path)
    v = kernels.point_values(c.spec, c.n, rule=c.rule, div=div, i_begin=c.i_begin,
                             n_local=g.count).cpu().numpy()
    _, exact = tt.true_values(g)
    bound = tt.sample_bounds(path, g, points=True)
    err = np.array([_err(float(a), e) for a, e in zip(v, exact)])
    k = int(np.argmax(err / bound))
    _record("point", cid, path, err[k], bound[k])
    assert (err <= bound).all(), (k, v[k], float(exact[k]), err[k], bound[k])


# ---------------------------------------------------------------------------- launches
@pytest.mark.parametrize("c", tc.LAUNCH_CASES, ids=lambda c: c.id)
def test_launches_against_truth(cuda, native, c):
    """The value of kernels.riemann (h sum) on all four paths against the exact h sum v(x_i):
    one tile, a tile and a remainder, a workgroup of tiles, thousands of tiles at grids 1, 3 and
    the default; three rules, fused and two-kernel in turn, every start a rank slice."""
    q = tc.GEOMS[c.geom]
    g = q.geometry()
    _assert_path(native, c.dtype, c.div, g, c.path)
    grid = c.grid or kernels.default_grid()
    got = float(kernels.riemann(q.spec, q.n, q.rule, c.dtype, c.div, grid=grid, i_begin=q.i_begin,
                                n_local=q.count, fused=c.fused).item())
    err, bound = _err(got, tt.true_value(g)), tt.launch_value_bound(c.path, g, grid)
    _record("launch", c.id, c.path, err, bound)
    assert err <= bound, (got, float(tt.true_value(g)), err, bound)


@pytest.mark.parametrize("dtype,div", tc.REQUESTS)
@pytest.mark.parametrize("n,rule", tc.WHOLE)
def test_whole_range_against_closed_form(cuda, native, n, rule, dtype, div):
    """The built-in profile over [0, 1800] at N = 100 003 ... 1e9 on the default grid against the
    closed form."""
    spec = integrands.table()
    g = tt.geometry(spec, n, rule)
    path = tt.effective_path(dtype, div)
    _assert_path(native, dtype, div, g, path)
    grid = kernels.default_grid()
    got = float(kernels.riemann(spec, n, rule, dtype, div, grid=grid).item())
    err, bound = _err(got, tt.true_value(g)), tt.launch_value_bound(path, g, grid)
    _record("whole", f"profile-N{n}-{rule}", path, err, bound)
    assert err <= bound, (got, float(tt.true_value(g)), err, bound)


@pytest.mark.parametrize("dtype,div", tc.REQUESTS)
@pytest.mark.parametrize("name,a", tc.DEGENERATE)
def test_degenerate_interval(cuda, native, name, a, dtype, div):
    """a == b: h = 0, every sample at a; the value is exactly 0.0 and the unscaled sum is count
    v(a) within the launch bound, on every path (the series tiles take the line branch: lo ==
    hi, and 1 / h = inf is never used)."""
    spec = integrands.table(tc.table(name) or None, a, a)
    g = tt.geometry(spec, tc.DEGENERATE_N, "mid", 0, tc.DEGENERATE_COUNT)
    path = tt.effective_path(dtype, div)
    _assert_path(native, dtype, div, g, path)
    kw = dict(grid=1, i_begin=0, n_local=g.count)
    got = float(kernels.riemann(spec, tc.DEGENERATE_N, "mid", dtype, div, **kw).item())
    part = float(kernels.riemann_partials(spec, tc.DEGENERATE_N, "mid", dtype, div, **kw)[0].item())
    err, bound = _err(part, tt.true_sum(g)), tt.launch_sum_bound(path, g, 1)
    _record("degenerate-sum", f"{name}-a{a:g}", path, err, bound)
    assert got == 0.0, got
    assert err <= bound, (part, float(tt.true_sum(g)), err, bound)


# ---------------------------------------------------------------------------- the plan
PLAN_N, PLAN_GRID = 64 * 4097 + 5, 5


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_plan_on_the_jagged_table(cuda, native, dtype):
    """An Integrator on the jagged table over [-4, 40] (both ends extrapolate), 64 * 4097 + 5
    samples on 5 workgroups: the plan reports the segment tiles and its value is within the
    launch bound of the truth."""
    spec = integrands.table(tc.table("jag"), -4.0, 40.0)
    it = Integrator(spec, n=PLAN_N, rule="mid", dtype=dtype, div="series", grid=PLAN_GRID)
    assert str(it.plan.effective_div).split(".")[-1] == "series"
    assert (it.plan.grid, it.plan.block) == (PLAN_GRID, 256)
    g = tt.geometry(spec, PLAN_N, "mid")
    path = f"{dtype}-series"
    got = it.run().value
    err, bound = _err(got, tt.true_value(g)), tt.launch_value_bound(path, g, PLAN_GRID)
    _record("plan", "jag-4to40", path, err, bound)
    assert err <= bound, (got, float(tt.true_value(g)), err, bound)


# ---------------------------------------------------------------------------- interp_fill
@pytest.mark.parametrize("name,dt,i0,n", tc.FILL_CASES, ids=lambda v: str(v))
def test_interp_fill_against_truth(cuda, name, dt, i0, n):
    """Every element of interp_fill against v(dt i) at the exact dt i: windows of at most 10 001
    elements at i0 = 0, 7, across the table's end and at 2**33 (far beyond it), n = 1, 2 and odd."""
    tab = tc.table(name)
    dev_tab = torch.tensor(tab, dtype=torch.float64, device=cuda) if tab else None
    full = tab or tuple(float(v) for v in integrands.table().native_table())
    y = kernels.interp_fill(n, i0=i0, dt=dt, table=dev_tab).cpu().numpy()
    bound = tt.fill_bounds(full, dt, i0, n)
    err = np.array([_err(float(y[i]), tt.fill_true(full, dt, i0 + i)) for i in range(n)])
    k = int(np.argmax(err / bound))
    _record("fill", f"{name}-dt{dt:g}-i{i0}-n{n}", "fp64-fill", err[k], bound[k])
    assert (err <= bound).all(), (k, y[k], err[k], bound[k])
