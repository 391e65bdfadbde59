"""The headline tile's squares at the shapes where what they leave out is largest.

div series_exact squares a residual that is linear within its 32-sample sub-tile (Pi4::tile_acc:
e_sq = e_c +- k A', no per-pair curvature term (k^2 - 85.25) B); the linear terms are summed in
closed form per 384-sample tile. The omitted term is at most 155 h^2 s per residual, i.e.
2 |e| 155 h^2 ~ 7e-20 of a value of order 1 at the largest h the series tiles accept
(192 h <= 2e-6: N >= 9.6e7 on [0, 1]). These tests run at that h, N = 96 000 001, not at the
workload's N = 1e9, with the bounds the existing tests use there: a few ulp of one tile's sum
against the point kernel, 1e-15 of a workgroup's sum against IEEE division, and bitwise
equal steps of a multi-step batch."""
from __future__ import annotations

import math

import pytest

from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu

N = 96_000_001
TILE = 384
TILES = N // TILE  # 250 000 full tiles
# the first tile, the tile nearest x = 1/sqrt(3) (where |f''| of 1/(1+x^2) vanishes and the
# slope is steepest), the last full tile
I_BEGIN = [0, TILE * round(TILES / math.sqrt(3.0)), TILE * (TILES - 1)]


@pytest.mark.parametrize("i0", I_BEGIN)
def test_one_tile_at_the_largest_h_equals_its_points(cuda, i0):
    """One 384-sample tile: the tile sum (closed-form linear terms + 384 squares of the
    sub-tile-linear residual) equals h * fsum of the point kernel's values over the same
    samples to 4 ulp, the bound of test_pi4_series_exact_point_kernel_sums_to_the_tile at
    N = 1e9."""
    spec = integrands.pi4()
    pts = kernels.point_values(spec, N, rule="left", div="series_exact", i_begin=i0,
                               n_local=TILE)
    want = math.fsum(pts.cpu().tolist()) * (1.0 / N)
    got = float(kernels.riemann(spec, N, rule="left", div="series_exact", grid=1, i_begin=i0,
                                n_local=TILE).item())
    print(f"i0={i0} tile={got!r} points={want!r} rel={(got - want) / want:.3e}")
    assert got == pytest.approx(want, rel=4 * 2.0**-52, abs=0), (got, want)


@pytest.mark.parametrize("i0", I_BEGIN[:2] + [TILE * (TILES - 256)])
def test_one_workgroup_of_tiles_equals_ieee_division(cuda, i0):
    """256 tiles (one per lane of a workgroup; two workgroups share them at grid 2): the
    series_exact sum equals the IEEE-division sum of the same samples to 1e-15 relative, the
    whole-run bound, and grids 1 and 2 agree to the same bound."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=i0, n_local=TILE * 256)
    got = {g: float(kernels.riemann(spec, N, div="series_exact", grid=g, **kw).item())
           for g in (1, 2)}
    ieee = {g: float(kernels.riemann(spec, N, div="ieee", grid=g, **kw).item()) for g in (1, 2)}
    for g in (1, 2):
        print(f"i0={i0} grid={g} series_exact={got[g]!r} ieee={ieee[g]!r} "
              f"rel={(got[g] - ieee[g]) / ieee[g]:.3e}")
        assert got[g] == pytest.approx(ieee[g], rel=1e-15, abs=0), (g, got[g], ieee[g])
    assert got[1] == pytest.approx(got[2], rel=1e-15, abs=0), got


def test_multistep_batch_at_the_largest_h(cuda):
    """Three steps in one multi-step batch: bitwise equal to each other, and equal to a
    one-launch-per-step plan's value to 1e-15 relative."""
    it = Integrator("pi4", n=N, div="series_exact", slots=3)
    assert it.plan.multistep and str(it.plan.effective_div).endswith("series_exact")
    it.run_steps(3, pipeline=False, graphs=False)
    got = [it.plan.host_result(it.plan.host_index_of(k, False)) for k in range(3)]
    one = Integrator("pi4", n=N, div="series_exact", multistep=False)
    assert not one.plan.multistep
    want = one.run().value
    print(f"batch={got!r} single={want!r} rel={(got[0] - want) / want:.3e}")
    assert len(set(got)) == 1 and math.isfinite(got[0]), got
    for v in got:
        assert v == pytest.approx(want, rel=1e-15, abs=0), (v, want)
