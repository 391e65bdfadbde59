"""Every 4/(1+x^2) kernel path against references that are not kernels (utils/pi4_truth.py):
the truth (mpmath, digamma closed form), what each series tile is defined to evaluate, and
bitwise models of the per-sample paths, with bounds derived from the kernels' own operations.
Cases: pi4_truth_cases.py (their CPU-side conditions: test_pi4_truth_cpu.py). Every case first
asserts the path it runs (the dispatcher's effective division, and for ieee whether the narrow
reciprocal or the library division applies), so a silent fallback cannot test nothing. Every
test prints its measured error next to the bound (`PI4TRUTH ...` lines:
profiles/r13/pi4_truth.md is made of them); the asserts use the derived bounds only.

Far coordinates and degenerate intervals: before kPi4SeriesMaxX / kPi4SeriesMaxXF32 existed
the dispatcher chose the series tiles from h alone. On the parent commit's build
    test_far_and_degenerate[fp32-series-far-2e19-i960-n192]     value nan (d_m = inf, s = 0)
    test_far_and_degenerate[fp32-series-far-1.2e19-i960-n192]   value 0.0 (the seed 1 / d_m is a
                                                                flushed denormal), truth 7.9e-44
    test_far_and_degenerate[fp64-series-point-1e200-i0-n484]    value nan, expected 0.0
and their fp32acc / series_exact / series_direct siblings fail, 13 cases in all
(profiles/r13/pi4_truth.md lists them); with the limits they run the library division and
pass.
"""
from __future__ import annotations

import numpy as np
import pytest

import pi4_truth_cases as pc
from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import pi4_truth as pt

pytestmark = pytest.mark.gpu
MP = pt.MP
MODEL_MAX = 20_000      # samples up to which a launch is also modelled bit for bit


def _record(kind, cid, path, err, bound):
    print(f"PI4TRUTH {kind} {cid} {path} err={err:.4e} bound={bound:.4e} "
          f"ratio={err / bound if bound > 0 else (0.0 if err == 0 else float('inf')):.4f}")


def _err(got: float, want) -> float:
    return float(abs(MP.mpf(got) - want))


def _args(g):
    return (0, g.a, g.h, float(g.off), g.i_begin, g.count, [], 0.0, 0.0)


def _assert_path(native, path, g, narrow=None):
    """The dispatcher runs `path` for a launch of geometry g (and, for ieee, the narrow or the
    library division as `narrow` says)."""
    dtype, div = pc.REQUEST[path]
    D, V = native.DType, native.DivMode
    eff = native.riemann_effective_div(*_args(g), getattr(D, dtype), getattr(V, div))
    assert f"{dtype}-{str(eff).split('.')[-1]}" == path
    if div == "ieee":
        want = pc.expected_narrow(dtype, g) if narrow is None else narrow
        assert native.riemann_pi4_ieee_narrow(*_args(g), getattr(D, dtype)) == want
    return dtype, div


def _partials(dom, n, g, rule, dtype, div, grid):
    return kernels.riemann_partials(dom.spec, n, rule, dtype, div, grid=grid, i_begin=g.i_begin,
                                    n_local=g.count).cpu().numpy()


def test_tile_lengths_are_the_codes(cuda, native):
    """T of every path, read from the dispatcher: the single-tile launches below rely on it."""
    D, V = native.DType, native.DivMode
    for path, (dtype, div) in pc.REQUEST.items():
        g = pc.geom(pc.dom_for(path, "unit"), "left")
        assert native.riemann_tile_len(*_args(g), getattr(D, dtype), getattr(V, div)) == pt.tile_len(path)
    assert (pt.TILE64, pt.TILE32, pt.TILE_PER_SAMPLE) == (384, 192, 32)


# ---------------------------------------------------------------------------- single tiles
@pytest.mark.parametrize("c", pc.TILE_CASES, ids=lambda c: c.id)
def test_single_tile(cuda, native, c):
    """grid = 1, n_local = T: partials[0] is one lane's one tile, every other lane adds zeros.
    Series tiles: against the definition at the bound of the tile's arithmetic alone, and
    against the truth at that plus the definition's own distance. ieee tiles: equal to the
    model bit for bit, and inside the truth bound."""
    d = pc.DOMAINS[c.dom]
    T = pt.tile_len(c.path)
    g = pc.geom(c.dom, c.rule, c.i_begin, T)
    dtype, div = _assert_path(native, c.path, g)
    got = float(_partials(d, d.n, g, c.rule, dtype, div, 1)[0])
    S = pc.truth_sum(c.dom, c.rule, c.i_begin, T)
    err, bound = _err(got, S), pt.tile_truth_bound(c.path, g, float(S))
    _record("tile-truth", c.id, c.path, err, bound)
    if c.path in pt.SERIES_PATHS:
        D = pc.defined_sum(c.path, c.dom, c.rule, c.i_begin)
        derr, dbound = _err(got, D), pt.tile_defn_rel(c.path, g) * float(D)
        _record("tile-defn", c.id, c.path, derr, dbound)
        assert derr <= dbound, (got, float(D), derr, dbound)
    else:
        want = pc.model_parts(c.path, c.dom, c.rule, c.i_begin, T, 1)[0]
        _record("tile-model", c.id, c.path, abs(got - want), 0.0)
        assert got == want, (got, want)
    assert err <= bound, (got, float(S), err, bound)


# ---------------------------------------------------------------------------- remainders
@pytest.mark.parametrize("c", pc.REM_CASES, ids=lambda c: c.id)
def test_remainders(cuda, native, c):
    """n_local = 1, 31, T - 1 (f.point per sample, one per lane, through the DPP wave sum) and
    T + 100 (a tile and the remainder): against the truth, and bit for bit against the model
    wherever only per-sample code runs (every path's remainder; the ieee tiles)."""
    d = pc.DOMAINS[c.dom]
    g = pc.geom(c.dom, c.rule, c.i_begin, c.count)
    dtype, div = _assert_path(native, c.path, g)
    got = float(_partials(d, d.n, g, c.rule, dtype, div, 1)[0])
    S = pc.truth_sum(c.dom, c.rule, c.i_begin, c.count)
    err, bound = _err(got, S), pt.launch_sum_bound(c.path, g, float(S), 1)
    _record("remainder", c.id, c.path, err, bound)
    if div == "ieee" or c.count < pt.tile_len(c.path):
        want = pc.model_parts(c.path, c.dom, c.rule, c.i_begin, c.count, 1)[0]
        assert got == want, (got, want)
    assert err <= bound, (got, float(S), err, bound)


# ---------------------------------------------------------------------------- per point
@pytest.mark.parametrize("c", pc.WINDOW_CASES, ids=lambda c: c.id)
def test_point_windows(cuda, native, c):
    """4096 values of point_values (every sample as the hot tile computes it; the samples past
    the window's last full tile by f.point) against SCALE f, per sample, for the four fp64
    divisions."""
    d = pc.DOMAINS[c.dom]
    g = pc.geom(c.dom, c.rule, c.i_begin, pc.WINDOW)
    _assert_path(native, c.path, g)
    v = kernels.point_values(d.spec, d.n, rule=c.rule, div=c.div, i_begin=c.i_begin,
                             n_local=pc.WINDOW).cpu().numpy()
    vals, exact = pc.truth_values(c.dom, c.rule, c.i_begin, pc.WINDOW)
    full = (pc.WINDOW // pt.tile_len(c.path)) * pt.tile_len(c.path)
    bound = pt.point_bound(c.path, g, vals)
    bound[full:] = pt.point_bound(c.path, g, vals[full:], full_tile=False)
    err = np.array([float(abs(MP.mpf(float(a)) / 4 - e)) for a, e in zip(v, exact)])
    k = int(np.argmax(err / bound))
    _record("point", c.id, c.path, err[k], bound[k])
    assert (err <= bound).all(), (k, v[k], vals[k], err[k], bound[k])


@pytest.mark.parametrize("dtype,div", [("fp32", "series"), ("fp32", "ieee"), ("fp32acc", "series")])
@pytest.mark.parametrize("fam", pc.POINT32_FAMILIES)
def test_fp32_single_samples(cuda, native, fam, dtype, div):
    """The fp32 paths have no point_values: 64 launches of one sample each (n_local = 1 runs
    Pi4F32::point through the remainder loop) equal model_point bit for bit, and are within
    point32_bound of the truth."""
    path = f"{dtype}-{div}"
    dom = pc.dom_for(path, fam)
    d = pc.DOMAINS[dom]
    worst = (0.0, 1.0)
    for j in range(pc.POINT32_COUNT):
        i = (d.n // 3 | 1) + 977 * j
        g = pc.geom(dom, "mid", i, 1)
        _assert_path(native, path, g)
        got = float(_partials(d, d.n, g, "mid", dtype, div, 1)[0])
        assert got == pt.model_point(path, g, 0), (i, got)
        t = float(pt.f_true(g.x(0)))
        e, b = _err(got, pt.f_true(g.x(0))), pt.point32_bound(g, t)
        assert e <= b, (i, got, t, e, b)
        worst = max(worst, (e / b, b))
    _record("point32", f"{path}-{dom}", path, worst[0] * worst[1], worst[1])


# ---------------------------------------------------------------------------- slices, ranges
def _value_case(native, c):
    d = pc.DOMAINS[c.dom]
    g = pc.geom(c.dom, c.rule, c.i_begin, c.count)
    dtype, div = _assert_path(native, c.path, g)
    grid = c.grid or kernels.default_grid()
    got = float(kernels.riemann(d.spec, d.n, c.rule, dtype, div, grid=grid, i_begin=c.i_begin,
                                n_local=c.count).item())
    S = pc.truth_sum(c.dom, c.rule, c.i_begin, c.count)
    want = MP.mpf(pt.SCALE) * MP.mpf(g.h) * S
    return d, g, dtype, div, grid, got, want, pt.launch_value_bound(c.path, g, float(S), grid)


@pytest.mark.parametrize("c", pc.SLICE_CASES, ids=lambda c: c.id)
def test_slices(cuda, native, c):
    """69 tiles (a full round and the exec-masked extra round), + 100 samples (the per-point
    remainder) and 261 tiles, at grids 1 and 2, for every path, against SCALE h times the
    closed form; the reversed, across-zero and off-unit families at the middle shape. The
    per-sample paths' partials also equal the model's, bit for bit."""
    d, g, dtype, div, grid, got, want, bound = _value_case(native, c)
    err = _err(got, want)
    _record("slice", c.id, c.path, err, bound)
    assert err <= bound, (got, float(want), err, bound)
    if div == "ieee" and c.count <= MODEL_MAX:
        p = _partials(d, d.n, g, c.rule, dtype, div, grid)
        assert tuple(p.tolist()) == pc.model_parts(c.path, c.dom, c.rule, c.i_begin, c.count, grid)


REV_SLICES = [c for c in pc.SLICE_CASES if c.dom.startswith("rev-")]


@pytest.mark.parametrize("c", REV_SLICES, ids=lambda c: c.id)
def test_reversed_against_forward(cuda, native, c):
    """b < a (h < 0): the reversed slice and the forward slice of the mirrored rule over the
    same stretch (samples n - i_begin - count ... of the forward family) are negatives of each
    other within the sum of both bounds (and the distance of the two truths: n fl(h) is not
    b - a exactly, so the two sample sets differ in the last places). Bound-wise only: the two
    launches visit a tile's samples in opposite order."""
    _, g, _, _, _, got, want, bound = _value_case(native, c)
    f = pc.DOMAINS[c.dom].reverse_of
    cf = pc.SliceCase(c.path, f, pc.MIRROR[c.rule], pc.DOMAINS[f].n - c.i_begin - c.count, c.count,
                      c.grid)
    _, gf, _, _, _, fgot, fwant, fbound = _value_case(native, cf)
    assert gf.h == -g.h
    slack = float(abs(want + fwant))
    assert slack <= 1e-6 * float(abs(want))         # the same stretch of the axis
    _record("reversed", c.id, c.path, abs(got + fgot), bound + fbound + slack)
    assert abs(got + fgot) <= bound + fbound + slack, (got, fgot)


@pytest.mark.parametrize("c", pc.RANGE_CASES, ids=lambda c: c.id)
def test_whole_ranges(cuda, native, c):
    """N = 1e9 (left, mid), 5e9, 1e10 and 96 000 001 on the default grid against the closed
    form. These derived worst-case bounds are looser than the empirical figures the older tests
    hold the same launches to (1e-15 / 2e-15 / 1e-12 relative between paths, 1e-9 absolute for
    fp32): both stay."""
    _, _, _, _, _, got, want, bound = _value_case(native, c)
    err = _err(got, want)
    _record("range", c.id, c.path, err, bound)
    assert err <= bound, (got, float(want), err, bound)


# ---------------------------------------------------------------------------- switch points
@pytest.mark.parametrize("c", pc.SWITCH_CASES, ids=lambda c: c.id)
def test_ieee_switch_points(cuda, native, c):
    """64-sample ieee launches with both ends below |x| = 2**249 (fp64) / 2**49 (fp32), both
    beyond, and one on each side: the narrow reciprocal runs only in the first, the library
    division in the others, fp32acc refuses them; either way the partial equals the model bit
    for bit and is inside the truth bound."""
    path = f"{c.dtype}-ieee"
    g = pt.geometry(c.spec, pc.SWITCH_N, "mid")
    narrow = c.tag == "below"
    _assert_path(native, path, g, narrow=narrow)
    if c.dtype == "fp32acc" and not narrow:
        with pytest.raises(RuntimeError, match="beyond 2\\^49"):
            kernels.riemann_partials(c.spec, pc.SWITCH_N, "mid", c.dtype, "ieee", grid=1)
        return
    got = float(kernels.riemann_partials(c.spec, pc.SWITCH_N, "mid", c.dtype, "ieee", grid=1)[0].item())
    want = pt.model_partials(path, g, 1)[0]
    S = pt.true_sum(g)
    err, bound = _err(got, S), pt.launch_sum_bound(path, g, float(S), 1)
    _record("switch", c.id, path + ("-narrow" if narrow else "-wide"), err, bound)
    assert got == want, (got, want)
    assert err <= bound, (got, float(S), err, bound)


def test_library_division_switch_runs_the_wide_tiles(cuda, native):
    """set_pi4_library_division forces Pi4Wide / Pi4F32Wide on [0, 1]: the dispatcher says so,
    and the tile is still the model's, bit for bit."""
    native.set_pi4_library_division(True)
    try:
        for path in ("fp64-ieee", "fp32-ieee"):
            dom = pc.dom_for(path, "unit")
            d = pc.DOMAINS[dom]
            i0 = 32 * (d.n // 64)
            g = pc.geom(dom, "mid", i0, 32 + 7)
            dtype, div = _assert_path(native, path, g, narrow=False)
            got = float(_partials(d, d.n, g, "mid", dtype, div, 1)[0])
            assert got == pc.model_parts(path, dom, "mid", i0, 32 + 7, 1)[0]
    finally:
        native.set_pi4_library_division(False)


# ---------------------------------------------------------------------------- far, degenerate
@pytest.mark.parametrize("c", pc.FAR_CASES, ids=lambda c: c.id)
def test_far_and_degenerate(cuda, native, c):
    """Slices at |x| = 2**61 (the fp32 series tiles still run), 1.2e19 (their seed would be
    denormal) and 2e19 (d_m would overflow to NaN), a == b at 1.0 and 1e200 (h = 0: the value
    is 0.0 on every path), and the wide-domain launches at 1e150 and 1e160 (the value, and
    the exact zero where 1 + x^2 overflows: the bound carries an underflow floor per sample).
    The path is asserted first: beyond the limits a series request runs the library division;
    fp32acc refuses."""
    d = pc.DOMAINS[c.dom]
    g = pc.geom(c.dom, "mid", c.i_begin, c.count)
    path = pc.expected_path(c.dtype, c.div, g)
    D, V = native.DType, native.DivMode
    eff = native.riemann_effective_div(*_args(g), getattr(D, c.dtype), getattr(V, c.div))
    assert f"{c.dtype}-{str(eff).split('.')[-1]}" == path
    kw = dict(grid=1, i_begin=c.i_begin, n_local=c.count)
    if c.raises:
        assert path == "fp32acc-ieee" and not pc.expected_narrow(c.dtype, g)
        with pytest.raises(RuntimeError, match="beyond 2\\^49"):
            kernels.riemann(d.spec, d.n, "mid", c.dtype, c.div, **kw)
        return
    got = float(kernels.riemann(d.spec, d.n, "mid", c.dtype, c.div, **kw).item())
    S = pt.true_sum(g)
    want = MP.mpf(pt.SCALE) * MP.mpf(g.h) * S
    err, bound = _err(got, want), pt.launch_value_bound(path, g, float(S), 1)
    _record("far", c.id, path, err, bound)
    assert err <= bound, (got, float(want), err, bound)      # NaN fails here
    if g.h == 0.0 or c.dom == "wide-1e160":
        assert got == 0.0, got
    if path.endswith("ieee") and c.count <= MODEL_MAX:
        p = kernels.riemann_partials(d.spec, d.n, "mid", c.dtype, c.div, **kw)
        assert float(p[0].item()) == pt.model_partials(path, g, 1)[0]


# ---------------------------------------------------------------------------- plans
@pytest.mark.parametrize("path,n", pc.PLAN_CASES, ids=[p for p, _ in pc.PLAN_CASES])
def test_plans(cuda, path, n):
    """One Integrator per path at its largest h: three steps of a multi-step plan and of a
    chained plan on the same grid. Every step within the launch bound of the truth, all six
    the same bits, and the plans report the division that ran."""
    dtype, div = pc.REQUEST[path]
    kw = dict(n=n, dtype=dtype, div=div, slots=3)
    ms = Integrator("pi4", close="kernel", **kw)
    ch = Integrator("pi4", multistep=False, grid=ms.plan.grid, **kw)
    assert not ch.plan.multistep and ms.plan.grid == ch.plan.grid
    g = pt.geometry(ms.spec, n, "left")
    S = pt.true_sum(g)
    want = MP.mpf(pt.SCALE) * MP.mpf(g.h) * S
    bound = pt.launch_value_bound(path, g, float(S), ms.plan.grid, ms.plan.block)
    vals = []
    for it in (ms, ch):
        assert f"{dtype}-{str(it.plan.effective_div).split('.')[-1]}" == path
        assert it.describe()["div"] == div
        it.run_steps(3, pipeline=True, graphs=True)
        assert it.plan.graphs_ready, it.plan.graph_error
        vals += [it.plan.host_result(it.plan.host_index_of(k, True)) for k in range(3)]
    err = _err(vals[0], want)
    _record("plan", f"{path}-n{n}", path, err, bound)
    assert len(set(vals)) == 1, vals
    assert err <= bound, (vals[0], float(want), err, bound)
