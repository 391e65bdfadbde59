"""Every polynomial kernel path against an exact rational truth (utils/poly_truth.py): point
values and launch values of the Taylor-pair tiles and of Horner per sample, fp64 and packed
fp32, within bounds derived from the kernels' own operations. Cases: poly_truth_cases.py (their
CPU-side conditions, the defect tests and what tile sums cannot see: test_poly_truth_cpu.py).
Every case first asserts the path it runs, so a silent fallback cannot test nothing, and prints
its measured error next to the bound (`POLYTRUTH ...` lines: profiles/r17/poly_truth.md is made
of them); the asserts use the derived bounds only.

Launch values hold the even part E of a sub-tile only ((E + k O) + (E - k O) = 2 E); the odd
part is held through point_values in fp64 and is not observable in fp32 (no fp32 point kernel).

Degenerate and tiny steps: before kernels.hpp poly_series_in_range existed a series request ran
the Taylor-pair tiles at any h. On the parent commit's build
    test_degenerate_and_underflow[fp64-series-a0-c4]      ran series, value nan, expected 0.0
    test_degenerate_and_underflow[fp32-series-a1e+30-c2]  ran series, value nan, expected 0.0
and every other a == b case of a series request with 1 to 8 coefficients fail, 33 in all
(u_m = x_m * inf, and the shift's first fma is 0 * inf), and the 26 underflow cases of a series
request, among them
    [fp64-series-0to2p-140-d7-t0-pure]      ran series, sum 1.7885390178462238e-294, truth
                                            1.788539017845758e-294: 2.6e-13 relative, where
                                            the Horner bound allows 8e-16 (c_7 h^7 = 2**-1033
                                            keeps 41 bits)
    [fp64-series-0to2p-140-d7-t-1090-pure]  ran series, sum 1.09e-313, truth 5.87e-313: c_7 h^7
                                            is zero, every full tile returns 0 and only the
                                            five remainder samples are left
    [fp32-series-...]                       13 cases: the sum (0.0, everything is below the fp32
                                            range) is inside the bound, but the launch ran the
                                            tiles where effective_div now reports Horner
59 failures in all (profiles/r17/poly_truth.md lists every one with the value it returned). With
the range test they run Horner per sample and pass. The accuracy lists (86 point cases, 320
launches, far and sub-ulp slices included) found no defect: they run the same kernels on both
builds, the dispatcher differing outside poly_series_in_range only, and their largest error is
0.74 of its bound per point and 0.24 per launch.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import poly_truth_cases as pc
from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import poly_truth as pt

pytestmark = pytest.mark.gpu


def _record(kind, cid, path, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"POLYTRUTH {kind} {cid} {path} err={err:.4e} bound={bound:.4e} ratio={ratio:.4f}")


def _err(got: float, want: Fraction) -> float:
    return float(abs(Fraction(got) - want)) if np.isfinite(got) else float("inf")


def _args(g):
    return (2, g.a, g.h, float(g.off), g.i_begin, g.count, list(g.coef), 0.0, 0.0)


def _effective(native, dtype, div, g) -> str:
    eff = native.riemann_effective_div(*_args(g), getattr(native.DType, dtype),
                                       getattr(native.DivMode, div))
    return f"{dtype}-{str(eff).split('.')[-1]}"


def _assert_path(native, dtype, div, g, path):
    assert pt.effective_path(dtype, div, g) == path
    assert _effective(native, dtype, div, g) == path
    T = native.riemann_tile_len(*_args(g), getattr(native.DType, dtype), getattr(native.DivMode, div))
    assert T == pt.tile_len(path)


# ---------------------------------------------------------------------------- per point
@pytest.mark.parametrize("c", pc.POINT_CASES, ids=lambda c: c.id)
def test_points_against_truth(cuda, native, c):
    """64 * 4 + 37 values of point_values, fp64 series and Horner, every bucket and family:
    the full tiles through series_point (the tile's own operations per sample: this is where
    the odd part O is held), the 37 through point(); each within its bound of p(x_i). The
    tile-local terms of the bound use L(k) = sum |b_m| k^m of the definition."""
    d = pc.DOMAINS[c.dom]
    g = c.geometry()
    _assert_path(native, "fp64", c.div, g, c.path)
    v = kernels.point_values(pc.spec(c.dom, c.ncoef), d.n, rule=c.rule, div=c.div,
                             i_begin=c.i_begin, n_local=pc.POINT_COUNT).cpu().numpy()
    _, exact = pt.true_values(g)
    local = None
    if c.div == "series":
        local = np.concatenate([pt.defined_tile(g, t, False, points=True)[1]
                                for t in range(g.count // 64)])
    bound = pt.sample_bounds(c.path, g, points=True, local=local)
    err = np.array([_err(float(a), e) for a, e in zip(v, exact)])
    k = int(np.argmax(err / bound))
    _record("point", c.id, c.path, err[k], bound[k])
    assert (err <= bound).all(), (k, v[k], float(exact[k]), err[k], bound[k])


# ---------------------------------------------------------------------------- launches
@pytest.mark.parametrize("c", pc.LAUNCH_CASES, ids=lambda c: c.id)
def test_launches_against_truth(cuda, native, c):
    """The value of kernels.riemann (h sum) on all four paths against the exact h sum p(x_i):
    one tile, five tiles and a remainder, a whole round at grids 1 and 3; three rules, fused
    and two-kernel in turn, every start a rank slice (i_begin > 0)."""
    d = pc.DOMAINS[c.dom]
    g = c.geometry()
    _assert_path(native, c.dtype, c.div, g, c.path)
    got = float(kernels.riemann(pc.spec(c.dom, c.ncoef), d.n, c.rule, c.dtype, c.div, grid=c.grid,
                                i_begin=c.i_begin, n_local=c.count, fused=c.fused).item())
    err, bound = _err(got, pt.true_value(g)), pt.launch_value_bound(c.path, g, c.grid)
    _record("launch", c.id, c.path, err, bound)
    assert err <= bound, (got, float(pt.true_value(g)), err, bound)


# ---------------------------------------------------------------------------- degenerate, underflow
@pytest.mark.parametrize("c", pc.DEGENERATE_CASES + pc.UNDERFLOW_CASES, ids=lambda c: c.id)
def test_degenerate_and_underflow(cuda, native, c):
    """a == b at 0, 1, -3.5 and 1e30 with three full tiles and five samples: h = 0, the value is
    exactly 0.0 on every path. Monomials of degree 5 to 7 on [0, 2**-140] and
    [2**-150, 2**-149] whose c_d h^d is a denormal or zero: the unscaled sum (the value h sum
    would itself underflow) is within the Horner bound of the truth, the bound's underflow
    floor included. Either kind runs Horner per sample on either request, and
    riemann_effective_div reports it; a == b sums to count p(a) within the same bound."""
    g = c.geometry()
    degenerate = isinstance(c, pc.DegenerateCase)
    n = pc.DEGENERATE_N if degenerate else pc.UNDERFLOW_COUNT
    ran = _effective(native, c.dtype, c.div, g)
    path = f"{c.dtype}-ieee"
    kw = dict(grid=1, i_begin=0, n_local=g.count)
    got = float(kernels.riemann(c.spec, n, "mid", c.dtype, c.div, **kw).item())
    part = float(kernels.riemann_partials(c.spec, n, "mid", c.dtype, c.div, **kw)[0].item())
    err = _err(part, pt.true_sum(g))
    bound = pt.launch_sum_bound(path, g, 1, floor=not degenerate)
    print(f"POLYTRUTH {'degenerate' if degenerate else 'underflow'} {c.id} ran={ran} value={got!r} sum={part!r} "
          f"truth={float(pt.true_sum(g))!r}")
    _record("degenerate-sum" if degenerate else "underflow-sum", c.id, ran, err, bound)
    assert ran == path == pt.effective_path(c.dtype, c.div, g)
    if degenerate:
        assert got == 0.0, got
    assert err <= bound, (part, float(pt.true_sum(g)), err, bound)


# ---------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("block", pc.PLAN_BLOCKS)
def test_plan_balanced_degree7(cuda, native, block):
    """An Integrator on the balanced degree-7 polynomial, the multi-step launch that closes its
    batch itself, 8 steps on 5 workgroups of 64 and of 1024 threads: the plan reports the
    Taylor-pair tiles, the 8 kept steps are the same bits, and that value is within the launch
    bound (at the plan's grid and block) of the truth. kernels.riemann on 5 workgroups of its
    own 256 threads is held to the same truth; the two sum the same 4097 tile values in different
    trees, so they agree within the sum of their bounds, not bit for bit."""
    spec = pc.plan_spec()
    it = Integrator(spec, n=pc.PLAN_N, rule="mid", div="series", grid=pc.PLAN_GRID, block=block,
                    slots=pc.PLAN_STEPS, close="launch")
    assert it.plan.multistep and it.plan.close_in_launch
    assert (it.plan.grid, it.plan.block) == (pc.PLAN_GRID, block)
    assert str(it.plan.effective_div).split(".")[-1] == "series"
    g = pt.geometry(spec, pc.PLAN_N, "mid")
    _assert_path(native, "fp64", "series", g, "fp64-series")
    it.run_steps(pc.PLAN_STEPS, pipeline=True, graphs=False)
    steps = [it.plan.host_result(it.plan.host_index_of(k, False)) for k in range(pc.PLAN_STEPS)]
    one = float(kernels.riemann(spec, pc.PLAN_N, "mid", "fp64", "series", grid=pc.PLAN_GRID).item())
    want = pt.true_value(g)
    bound = pt.launch_value_bound("fp64-series", g, pc.PLAN_GRID, block)
    bound1 = pt.launch_value_bound("fp64-series", g, pc.PLAN_GRID)
    _record("plan", f"balanced-c8-block{block}", "fp64-series", _err(steps[0], want), bound)
    _record("plan-launch", f"balanced-c8-block{block}", "fp64-series", _err(one, want), bound1)
    assert len(set(steps)) == 1, steps
    assert _err(steps[0], want) <= bound and _err(one, want) <= bound1, (steps[0], one, float(want))
    assert abs(steps[0] - one) <= bound + bound1
