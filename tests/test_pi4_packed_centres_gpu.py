"""The headline tile's sub-tile centres in packed fp32, where a wrong half could show.

div series_exact forms the centres and slopes of the two sub-tiles at +c0 and -c0 as the low
and high halves of three v_pk_fma_f32 (Pi4::centres_f32 / slopes_f32) and lets the pair loop
read its half through op_sel. A swapped half, a wrong sign of c0 or a centre of the wrong
sub-tile changes a sample's e^2 by up to ~4e-12 of its value (thousands of ulp) wherever |e| is
near its largest, 2e-6: at the largest h the series tiles accept (N = 96 000 001 on [0, 1]),
away from x = 0. The pair loop itself is hand-ordered (Pi4::subtile_squares: one asm statement
per sub-tile, where the compiler adds no wait states), so a tile against its own points, under
a partial exec mask too, is also what shows that its order keeps the hardware's distance rule.
The references are the IEEE-division kernel and the true function in x87
extended precision, never the code under test; the bounds are the existing tests': 1.5 ulp per
point against the true value, 2 ulp against IEEE division, 1e-15 of a sum against IEEE
division, 4 ulp of a tile's sum against its own points, bitwise equal steps."""
from __future__ import annotations

import math

import numpy as np
import pytest

from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu

N = 96_000_001
TILE = 384
SUB = 32
TILES = N // TILE


def true_values(n: int, i0: int, count: int, a: float = 0.0, b: float = 1.0):
    """4 / (1 + x^2) at x = a + i h in x87 extended precision, h the launch's fp64 step."""
    h = np.longdouble((b - a) / n)
    x = np.longdouble(a) + (np.arange(count, dtype=np.longdouble) + np.longdouble(i0)) * h
    return np.longdouble(4) / (np.longdouble(1) + x * x)


def ulps(got: np.ndarray, want: np.ndarray, of: np.ndarray) -> np.ndarray:
    return np.abs((got.astype(np.longdouble) - want.astype(np.longdouble)) /
                  np.spacing(np.abs(of).astype(np.float64)).astype(np.longdouble)).astype(np.float64)


# the middle of the interval (|e| up to 1.6e-6) and the last full tile (2e-6, the largest)
@pytest.mark.parametrize("tile", [TILES // 2, TILES - 1])
def test_sub_tile_boundaries(cuda, tile):
    """Every sample of one whole tile, and on their own the 24 samples next to a sub-tile
    boundary (the first and the last of each of the 12 sub-tiles: k = -15.5 and +15.5, the
    largest offsets from the centres that the +-c0 halves carry)."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=TILE * tile, n_local=TILE)
    v = kernels.point_values(spec, N, div="series_exact", **kw).cpu().numpy()
    w = kernels.point_values(spec, N, div="ieee", **kw).cpu().numpy()
    true = true_values(N, TILE * tile, TILE)
    ut, ui = ulps(v, true, true), ulps(v, w, w)
    u = np.arange(TILE)
    border = (u % SUB == 0) | (u % SUB == SUB - 1)
    assert border.sum() == 24
    print(f"tile {tile}: vs true max {ut.max():.4f} (border {ut[border].max():.4f}); "
          f"vs ieee max {ui.max():.4f} (border {ui[border].max():.4f})")
    assert ut[border].max() <= 1.5 and ui[border].max() <= 2.0, (ut[border], ui[border])
    assert ut.max() <= 1.5, ut.max()
    assert ui.max() <= 2.0, ui.max()


# kernels.riemann launches 256-thread workgroups; lane g owns tiles g, g + lanes, ...
#   69 tiles:  wave 0 runs one full round, lanes 0-4 of wave 1 the exec-masked extra round
#   261 tiles: at grid 1 every lane runs one round and lanes 0-4 of wave 0 the masked one
#              after it; at grid 2 lanes 0-4 of the second workgroup's first wave
# and + 100 samples adds the per-point remainder
@pytest.mark.parametrize("n_local", [TILE * 69, TILE * 69 + 100, TILE * 261])
@pytest.mark.parametrize("grid", [1, 2])
def test_exec_masked_extra_round(cuda, grid, n_local):
    """Five lanes of a wave run a tile of their own under a partial exec mask."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=TILE * (TILES // 2), n_local=n_local, grid=grid)
    got = float(kernels.riemann(spec, N, div="series_exact", **kw).item())
    ieee = float(kernels.riemann(spec, N, div="ieee", **kw).item())
    print(f"grid={grid} n_local={n_local} series_exact={got!r} ieee={ieee!r} "
          f"rel={(got - ieee) / ieee:.3e}")
    assert got == pytest.approx(ieee, rel=1e-15, abs=0), (got, ieee)


def test_a_tile_across_zero(cuda, native):
    """[-1, 1/2] at the largest h 1.5 / n admits: the tile that holds x = 0, where the slope
    A = -2 x h s changes sign, against the fsum of its own points and against IEEE division."""
    a, b, n = -1.0, 0.5, 144_000_001
    assert native.series_ok((b - a) / n)
    h = (b - a) / n
    i0 = TILE * 250_000
    assert a + i0 * h < 0.0 < a + (i0 + TILE) * h
    spec = integrands.IntegrandSpec("pi4", a, b)
    kw = dict(rule="left", i_begin=i0, n_local=TILE)
    pts = kernels.point_values(spec, n, div="series_exact", **kw)
    want = math.fsum(pts.cpu().tolist()) * h
    got = float(kernels.riemann(spec, n, div="series_exact", grid=1, **kw).item())
    ieee = float(kernels.riemann(spec, n, div="ieee", grid=1, **kw).item())
    print(f"tile={got!r} points={want!r} rel={(got - want) / want:.3e}; ieee={ieee!r} "
          f"rel={(got - ieee) / ieee:.3e}")
    assert got == pytest.approx(want, rel=4 * 2.0**-52, abs=0), (got, want)
    assert got == pytest.approx(ieee, rel=1e-15, abs=0), (got, ieee)


def test_two_small_plans_agree_bitwise(cuda):
    """Three steps of one persistent multi-step launch and of a chained plan on the same grid at
    N = 96 000 001: all six values the same bits."""
    kw = dict(n=N, div="series_exact", slots=3)
    ms = Integrator("pi4", close="kernel", **kw)
    ch = Integrator("pi4", multistep=False, grid=ms.plan.grid, **kw)
    assert ms.plan.multistep and not ch.plan.multistep and ms.plan.grid == ch.plan.grid
    assert str(ms.plan.effective_div).endswith("series_exact")
    for it in (ms, ch):
        it.run_steps(3, pipeline=True, graphs=True)
        assert it.plan.graphs_ready, it.plan.graph_error
    got = [ms.plan.host_result(ms.plan.host_index_of(k, True)) for k in range(3)]
    want = [ch.plan.host_result(ch.plan.host_index_of(k, True)) for k in range(3)]
    print(f"multistep={got!r} chained={want!r}")
    assert math.isfinite(got[0]) and len(set(got)) == 1 and got == want, (got, want)
