"""The headline tile's packed-fp32 squares where fp32 could show.

div series_exact keeps the seed, the sub-tile centres and the closed-form sum of the residuals'
linear terms in fp64, and forms each sample's own residual e_sq = e_c +- k A' and its square in
fp32 (Pi4::tile_acc: two v_pk_fma_f32 per +-k pair). With |e| <= 2e-6 the fp32 residual is off
by at most 3 * 2^-24 * 2e-6 ~ 3.6e-13, its square by ~1.7e-18 of a value of order 1: under 1/60
ulp at the largest h the series tiles accept (192 h <= 2e-6: N >= 9.6e7 on [0, 1]). These tests
run at that h (N = 96 000 001), away from [0, 1] and at a small h (N = 1e10, the smallest A' in
fp32), with the bounds the existing tests use: 1e-15 of a sum against the true function or IEEE
division, 1.5 ulp per point against the true value and 2 ulp against IEEE division, 4 ulp of a
tile's sum against its own points, and bitwise equal steps."""
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
TILES = N // TILE  # 250 000 full tiles
WINDOW = 4096
# the first tile, the middle of the interval, the last 384 samples
I_BEGIN = [0, TILE * (TILES // 2), N - TILE]


def true_values(n: int, i0: int, count: int, a: float = 0.0, b: float = 1.0):
    """4 / (1 + x^2) at x = a + i h in x87 extended precision, h the launch's fp64 step."""
    h = np.longdouble((b - a) / n)
    x = np.longdouble(a) + (np.arange(count, dtype=np.longdouble) + np.longdouble(i0)) * h
    return np.longdouble(4) / (np.longdouble(1) + x * x)


def ulps(got: np.ndarray, want: np.ndarray, of: np.ndarray) -> np.ndarray:
    return np.abs((got.astype(np.longdouble) - want.astype(np.longdouble)) /
                  np.spacing(np.abs(of).astype(np.float64)).astype(np.longdouble)).astype(np.float64)


@pytest.mark.parametrize("i0", I_BEGIN)
def test_one_tile_against_the_true_function(cuda, i0):
    """One 384-sample tile at the largest admitted h: h * sum of the true values at the same
    coordinates (x87 extended precision), to the whole-sum tolerance 1e-15 relative."""
    spec = integrands.pi4()
    got = float(kernels.riemann(spec, N, rule="left", div="series_exact", grid=1, i_begin=i0,
                                n_local=TILE).item())
    want = float(true_values(N, i0, TILE).sum() * np.longdouble(1.0 / N))
    print(f"i0={i0} tile={got!r} true={want!r} rel={(got - want) / want:.3e}")
    assert got == pytest.approx(want, rel=1e-15, abs=0), (got, want)


@pytest.mark.parametrize("i0", [0, TILE * (TILES // 2), N - WINDOW])
def test_point_values_at_the_largest_h(cuda, i0):
    """4096 samples: every series_exact value within 1.5 ulp of the true value and within 2 ulp
    of the IEEE path's value."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=i0, n_local=WINDOW)
    v = kernels.point_values(spec, N, div="series_exact", **kw).cpu().numpy()
    w = kernels.point_values(spec, N, div="ieee", **kw).cpu().numpy()
    true = true_values(N, i0, WINDOW)
    ut, ui = ulps(v, true, true), ulps(v, w, w)
    print(f"i0={i0} vs true max {ut.max():.4f} mean {ut.mean():.4f}; vs ieee max {ui.max():.4f}")
    assert ut.max() <= 1.5, (i0, ut.max())
    assert ui.max() <= 2.0, (i0, ui.max())


@pytest.mark.parametrize("i0", I_BEGIN)
def test_one_tile_equals_its_own_points(cuda, i0):
    """The tile sum (fp64 closed-form linear terms + 384 fp32 squares in two running sums)
    equals h * fsum of the point kernel's values (fp64 residual + the same fp32 square, one by
    one) to 4 ulp of the tile sum."""
    spec = integrands.pi4()
    pts = kernels.point_values(spec, N, rule="left", div="series_exact", i_begin=i0,
                               n_local=TILE)
    want = math.fsum(pts.cpu().tolist()) * (1.0 / N)
    got = float(kernels.riemann(spec, N, rule="left", div="series_exact", grid=1, i_begin=i0,
                                n_local=TILE).item())
    print(f"i0={i0} tile={got!r} points={want!r} rel={(got - want) / want:.3e}")
    assert got == pytest.approx(want, rel=4 * 2.0**-52, abs=0), (got, want)


# (a, b, n, first sample): [-1, 1/2] at the largest h 1.5 / n admits, 256 tiles centred on
# x = 0, where the slope A = -2 x h s changes sign; [8, 9], |x| larger (1 + x^2 up to 82, the
# seed s down to 1/82), at the largest h again
AWAY = [(-1.0, 0.5, 144_000_001, TILE * (250_000 - 128)),
        (8.0, 9.0, N, TILE * 1000)]


@pytest.mark.parametrize("a,b,n,i0", AWAY)
def test_away_from_the_unit_interval_equals_ieee_division(cuda, native, a, b, n, i0):
    """256 tiles at grids 1 and 2 against IEEE division to 1e-15 relative, on intervals the
    series tiles still accept (asserted: a fallback to another division would test nothing)."""
    assert native.series_ok((b - a) / n)
    assert str(Integrator("pi4", n=n, div="series_exact", a=a, b=b).plan.effective_div).endswith(
        "series_exact")
    spec = integrands.IntegrandSpec("pi4", a, b)
    h = (b - a) / n
    if a < 0:  # the window straddles x = 0
        assert a + i0 * h < 0.0 < a + (i0 + TILE * 256) * h
    kw = dict(rule="left", i_begin=i0, n_local=TILE * 256)
    for g in (1, 2):
        got = float(kernels.riemann(spec, n, div="series_exact", grid=g, **kw).item())
        ieee = float(kernels.riemann(spec, n, div="ieee", grid=g, **kw).item())
        print(f"[{a}, {b}] grid={g} series_exact={got!r} ieee={ieee!r} "
              f"rel={(got - ieee) / ieee:.3e}")
        assert got == pytest.approx(ieee, rel=1e-15, abs=0), (g, got, ieee)


def test_small_h_equals_ieee_division(cuda):
    """N = 1e10, 256 tiles from about N / 3: the slopes A' are at their smallest in fp32."""
    n = 10**10
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=TILE * (n // 3 // TILE), n_local=TILE * 256)
    for g in (1, 2):
        got = float(kernels.riemann(spec, n, div="series_exact", grid=g, **kw).item())
        ieee = float(kernels.riemann(spec, n, div="ieee", grid=g, **kw).item())
        print(f"grid={g} series_exact={got!r} ieee={ieee!r} rel={(got - ieee) / ieee:.3e}")
        assert got == pytest.approx(ieee, rel=1e-15, abs=0), (g, got, ieee)


def test_multistep_batch_is_deterministic_and_equals_chained(cuda):
    """Three steps of one persistent multi-step launch at the largest h: bitwise equal to each
    other and to a chained (one launch per step) plan's steps on the same grid."""
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
