"""The long tile of div series_exact (integrands.hpp Pi4Long): 1536 samples per seed in 24
sub-tiles of 64, run where 768 h <= 2e-6. Everything here is at N = 384 000 001 on [0, 1], the
largest step the long tile admits (|e| up to 2e-6: where a wrong half, sign or centre shows as
thousands of ulp), unless a test says otherwise, and every launch asserts through the
dispatcher (riemann_tile_len, plan.tile) that the long tile is what runs.

The references are never the code under test: the truth (utils/pi4_truth.py: mpmath, digamma
closed form), the true function in x87 extended precision, the IEEE-division kernel, and for
tile = "short" values recorded from the build before the long tile existed. The bounds are the
existing tests': pi4_truth's launch bound, 1.5 ulp per point against the true value, 2 ulp
against IEEE division, 1e-15 of a sum against IEEE division, 4 ulp of a tile's sum against its
own points, bitwise equal steps and kernel forms; the single tiles use the long tile's own
derived bound (pi4_truth.tile_truth_bound, LONG_PATH)."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import pi4_truth as pt

pytestmark = pytest.mark.gpu

N = 384_000_001
TILE = 1536
SUB = 64
TILES = N // TILE
MP = pt.MP


def assert_long(spec, n, **kw):
    assert kernels.riemann_tile_len(spec, n, tile="long", **kw) == TILE
    assert kernels.riemann_tile_len(spec, n, **kw) in (TILE, 384)  # auto: either, never else


def true_values(n: int, i0: int, count: int, a: float = 0.0, b: float = 1.0):
    """4 / (1 + x^2) at x = a + i h in x87 extended precision, h the launch's fp64 step."""
    h = np.longdouble((b - a) / n)
    x = np.longdouble(a) + (np.arange(count, dtype=np.longdouble) + np.longdouble(i0)) * h
    return np.longdouble(4) / (np.longdouble(1) + x * x)


def ulps(got: np.ndarray, want: np.ndarray, of: np.ndarray) -> np.ndarray:
    return np.abs((got.astype(np.longdouble) - want.astype(np.longdouble)) /
                  np.spacing(np.abs(of).astype(np.float64)).astype(np.longdouble)).astype(np.float64)


# ---------------------------------------------------------------------------- stage 0
def test_op_sel_and_neg_hi_on_a_scalar_pair(cuda):
    """v_pk_fma_f32 with op_sel / op_sel_hi picking one half of a scalar pair (k_a, k_b) for
    both lanes and neg_hi negating the high lane gives, bit for bit, what the scalar pairs
    (k, -k) give, for the low and for the high half of the slope and centre pairs; and both are
    the fp32 fma of the values meant."""
    rng = np.random.default_rng(20)
    ac = (rng.standard_normal((4096, 4)) * np.array([1e-9, 3e-9, 2e-6, 1e-6])).astype(np.float32)
    ac[0] = [1.0, 2.0, 3.0, 5.0]  # halves and signs readable at a glance
    ka, kb = 3.5, 19.5
    out = kernels.pk_modifier_check(torch.from_numpy(ac).to(cuda), ka, kb).cpu().numpy()
    new, old = out[:, :8].view(np.uint32), out[:, 8:].view(np.uint32)
    print(f"row 0: new {out[0, :8].tolist()} old {out[0, 8:].tolist()}")
    assert (new == old).all(), np.argwhere(new != old)[:8]
    assert out[0, :8].tolist() == [6.5, -0.5, 22.5, -16.5, 12.0, -2.0, 44.0, -34.0]
    a64, c64 = ac[:, 0:2].astype(np.float64), ac[:, 2:4].astype(np.float64)
    col = 0
    for half in (0, 1):
        for k in (ka, kb):
            for sign in (1.0, -1.0):
                want = (sign * k * a64[:, half] + c64[:, half]).astype(np.float32)
                assert (out[:, col].view(np.uint32) == want.view(np.uint32)).all(), (half, k, sign)
                col += 1


# ---------------------------------------------------------------------------- one tile
@pytest.mark.parametrize("i0", [0, TILE * (TILES // 2) + 1, N - TILE],
                         ids=["first", "middle-odd-start", "last"])
def test_one_tile(cuda, i0):
    """grid = 1, n_local = 1536: partials[0] is one lane's one tile. Against the truth at the
    long tile's derived bound, and against the sum of its own point values to 4 ulp."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=i0, n_local=TILE)
    assert_long(spec, N, **kw)
    got = float(kernels.riemann_partials(spec, N, grid=1, tile="long", **kw)[0].item())
    g = pt.geometry(spec, N, "left", i0, TILE)
    S = pt.true_sum(g)
    err, bound = float(abs(MP.mpf(got) - S)), pt.tile_truth_bound(pt.LONG_PATH, g, float(S))
    pts = kernels.point_values(spec, N, div="series_exact", tile="long", **kw).cpu().tolist()
    own = math.fsum(pts) / 4.0
    print(f"tile at {i0}: {got!r} truth err {err:.3e} bound {bound:.3e} ({err / bound:.3f}); "
          f"own points {own!r} ({(got - own) / math.ulp(got):+.2f} ulp)")
    assert err <= bound
    assert abs(got - own) <= 4 * math.ulp(got)


# ---------------------------------------------------------------------------- point values
@pytest.mark.parametrize("n,i0", [(N, TILE * (TILES // 2)), (N, N - 4096 - 1000),
                                  (10**9, TILE * 81_380)],
                         ids=["middle", "end", "n-1e9"])
def test_point_values(cuda, n, i0):
    """4096 point values from a tile's start: two whole tiles (a tile border, 47 sub-tile
    borders) and 1024 samples of a partial tile: within 1.5 ulp of the true value and 2 ulp of
    IEEE division, the samples next to a sub-tile border (k = -31.5 and +31.5) on their own."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=i0, n_local=4096)
    assert_long(spec, n, **kw)
    v = kernels.point_values(spec, n, div="series_exact", tile="long", **kw).cpu().numpy()
    w = kernels.point_values(spec, n, div="ieee", **kw).cpu().numpy()
    true = true_values(n, i0, 4096)
    ut, ui = ulps(v, true, true), ulps(v, w, w)
    u = np.arange(4096)
    border = ((u % SUB == 0) | (u % SUB == SUB - 1)) & (u < 2 * TILE)
    tile, rest = u < 2 * TILE, u >= 2 * TILE
    print(f"n={n} i0={i0}: tiles vs true max {ut[tile].max():.4f} at {ut[tile].argmax()} "
          f"(border {ut[border].max():.4f}); vs ieee max {ui[tile].max():.4f} "
          f"(border {ui[border].max():.4f}); remainder vs true max {ut[rest].max():.4f}, "
          f"vs ieee {ui[rest].max():.4f}")
    assert not (v[:2 * TILE] == w[:2 * TILE]).all()   # the tiles' values, not the division's
    assert ut[tile].max() <= 1.5 and ui[tile].max() <= 2.0, (ut[tile].max(), ui[tile].max())
    # The last 1024 samples are no full tile: the kernel divides there (f.point, as in every
    # launch's remainder), which is not this tile's arithmetic and is not held to 1.5 ulp
    # anywhere (a rounded 1 + x^2 alone costs up to an ulp): pi4_truth's per-sample bound.
    g = pt.geometry(spec, n, "left", i0, 4096)
    rel = pt.ieee_rel("fp64-ieee", g)
    assert (np.abs(v[rest].astype(np.longdouble) - true[rest]) <= rel * true[rest]).all()


# ---------------------------------------------------------------------------- slices
# kernels.riemann_partials launches 256-thread workgroups; lane g owns tiles g, g + lanes, ...
#   69 tiles:  wave 0 runs one full round, lanes 0-4 of wave 1 the exec-masked extra round
#   261 tiles: at grid 1 every lane runs one round and lanes 0-4 of wave 0 the masked one
#              after it; at grid 2 lanes 0-4 of the second workgroup's first wave
#   + 100 samples adds the per-point remainder; 1535 samples are no full tile at all
@pytest.mark.parametrize("grid,n_local", [(g, n) for n in (TILE * 69, TILE * 69 + 100, TILE * 261)
                                           for g in (1, 2)] + [(1, TILE - 1)])
def test_slices_against_the_truth(cuda, grid, n_local):
    spec = integrands.pi4()
    i0 = TILE * (TILES // 2)
    kw = dict(rule="left", i_begin=i0, n_local=n_local)
    assert_long(spec, N, **kw)
    p = kernels.riemann_partials(spec, N, grid=grid, tile="long", **kw).cpu().tolist()
    g = pt.geometry(spec, N, "left", i0, n_local)
    S = pt.true_sum(g)
    got = math.fsum(p)
    err = float(abs(MP.mpf(got) - S))
    bound = pt.launch_sum_bound("fp64-series_exact", g, float(S), grid)
    print(f"grid={grid} n_local={n_local}: err {err:.3e} bound {bound:.3e} ({err / bound:.3f})")
    assert err <= bound


@pytest.mark.parametrize("a,b,n,i0", [
    (-1.0, 0.5, 576_000_001, TILE * 250_000 - TILE * 34),   # x = 0 inside the slice
    (8.0, 9.0, N, TILE * 1000),                             # s = 1 / (1 + x^2) ~ 1/70
], ids=["across-zero", "eight-to-nine"])
@pytest.mark.parametrize("grid", [1, 2])
def test_sign_change_and_small_seed(cuda, grid, a, b, n, i0):
    """A 69-tile slice where the slope A = -2 x h s changes sign, and one where the seed is
    small: against IEEE division to 1e-15 relative."""
    spec = integrands.IntegrandSpec("pi4", a, b)
    h = (b - a) / n
    kw = dict(rule="left", i_begin=i0, n_local=TILE * 69, grid=grid)
    if a < 0:
        assert a + i0 * h < 0.0 < a + (i0 + TILE * 69) * h
    assert_long(spec, n, rule="left", i_begin=i0, n_local=TILE * 69)
    got = float(kernels.riemann(spec, n, div="series_exact", tile="long", **kw).item())
    ieee = float(kernels.riemann(spec, n, div="ieee", **kw).item())
    print(f"[{a}, {b}] grid={grid}: long={got!r} ieee={ieee!r} rel={(got - ieee) / ieee:.3e}")
    assert got == pytest.approx(ieee, rel=1e-15, abs=0), (got, ieee)


def test_degenerate_interval_keeps_returning_zero(cuda):
    """a == b (h = 0): the dispatcher keeps the 384-sample tile and the value is 0."""
    spec = integrands.IntegrandSpec("pi4", 0.75, 0.75)
    assert kernels.riemann_tile_len(spec, 10**9) == 384
    assert float(kernels.riemann(spec, 10**9, grid=2, n_local=TILE * 300).item()) == 0.0


# ---------------------------------------------------------------------------- a 3-step batch
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("grid", [1, 3])
def test_three_step_batch_is_one_value_in_every_form(cuda, grid, block):
    """Three steps of the queue, the static multi-step launch, the chained kernels (all by one
    graph replay) and the fused kernel: the same bits, step to step and form to form."""
    kw = dict(n=N, div="series_exact", slots=3, grid=grid, block=block, tile="long",
              slice_of=(3, 64))  # a 1/64 share: 6e6 samples a step
    plans = {"queue": Integrator("pi4", close="kernel", work="queue", **kw),
             "static": Integrator("pi4", close="kernel", work="static", **kw),
             "chained": Integrator("pi4", multistep=False, **kw)}
    assert plans["queue"].plan.work == "queue" and plans["static"].plan.work == "static"
    assert plans["queue"].plan.multistep and not plans["chained"].plan.multistep
    vals = {}
    for name, it in plans.items():
        assert it.plan.tile == "long" and it.plan.grid == grid and it.plan.block == block
        it.run_steps(3, pipeline=True, graphs=True)
        assert it.plan.graphs_ready, it.plan.graph_error
        vals[name] = [it.plan.host_result(it.plan.host_index_of(k, True)) for k in range(3)]
    one = plans["queue"].run().value   # the fused kernel, at the plan's grid and block
    print(f"grid={grid} block={block}: {vals} fused={one!r}")
    first = vals["queue"][0]
    assert math.isfinite(first) and first > 0
    for name, v in vals.items():
        assert v == [first] * 3, (name, v)
    assert one == first


def test_a_plan_takes_the_long_tile_where_the_step_admits_it(cuda, monkeypatch):
    """RiemannConfig::tile = auto: long at N = 1e9 and at N = 384 000 001, short just above
    that step and on request; MIINT_PI4_TILE=short is the A/B's other side; the grid is the
    one the plan had before (the residency)."""
    monkeypatch.delenv("MIINT_PI4_TILE", raising=False)
    auto = Integrator("pi4", n=10**9)
    assert auto.plan.tile == "long" and auto.plan.multistep and auto.plan.work == "queue"
    short = Integrator("pi4", n=10**9, tile="short")
    assert short.plan.tile == "short" and short.plan.grid == auto.plan.grid
    assert Integrator("pi4", n=N).plan.tile == "long"
    assert Integrator("pi4", n=N - 2).plan.tile == "short"
    assert Integrator("pi4", n=10**9, div="series").plan.tile == "short"
    with pytest.raises(RuntimeError, match="tile = long"):
        Integrator("pi4", n=96_000_001, tile="long")
    monkeypatch.setenv("MIINT_PI4_TILE", "short")
    assert Integrator("pi4", n=10**9).plan.tile == "short"
    monkeypatch.delenv("MIINT_PI4_TILE")
    a, b = auto.run().value, short.run().value
    print(f"N = 1e9: long {a!r} short {b!r}")
    assert abs(a - b) <= 2 * math.ulp(b)


# ---------------------------------------------------------------------------- tile = "short"
# riemann_partials(pi4, 1e9, grid=2, i_begin=384 * 1_000_000, n_local=2 * 384 * 256) of the
# build before the long tile existed (div series_exact, left rule), as hex floats
SHORT_RECORDED = ['0x1.4ea470bc4f480p+16', '0x1.4e9ecd89fc7e0p+16']


def test_short_tile_is_the_earlier_kernel(cuda):
    """tile = "short" at N = 1e9, where auto runs the long tile: the 384-sample kernel, whose
    partials are bit for bit what the build before this tile gave."""
    spec = integrands.pi4()
    kw = dict(rule="left", i_begin=384 * 1_000_000, n_local=2 * 384 * 256)
    assert kernels.riemann_tile_len(spec, 10**9, tile="short", **kw) == 384
    assert kernels.riemann_tile_len(spec, 10**9, tile="long", **kw) == TILE
    p = kernels.riemann_partials(spec, 10**9, grid=2, tile="short", **kw).cpu().tolist()
    print("short partials:", [v.hex() for v in p])
    assert [v.hex() for v in p] == SHORT_RECORDED
