"""Parameter sweeps of a runtime integrand on the MI355X (csrc/runtime/expr_sweep.cpp):
f(x, p0..p7) over K rows per launch against the host sweep and closed forms; the edges of the
lane split, bitwise row independence, slices and loopback ranks, many small rows, 64-bit
sample indices, argument errors and the CLI."""
from __future__ import annotations

import json
import math
import os
import subprocess

import numpy as np
import pytest

from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.parallel import loopback
from cuda_v_mpi_amd.parallel.decomposition import rank_slice

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECAY = "p0*exp(-p0*x)"          # on [0, 2]: 1 - exp(-2 p0)
DECAY_P = [0.5, 1.0, 2.0, 4.0]
LORENTZ = "1.0/(1.0+p0*x*x)"     # on [0, 1]: atan(sqrt(p0)) / sqrt(p0)
LORENTZ_P = [0.25, 1.0, 9.0]


def _rows(ps):
    return [[p] for p in ps]


def _sweep(expr, rows, a, b, n, **kw):
    return kernels.riemann_expr_sweep(expr, rows, a, b, n, **kw).cpu().numpy()


def _host(native, expr, rows, a, b, n, rule):
    rows = np.asarray(rows, dtype=np.float64)
    return native.HostExprSweep(expr, rows.shape[1]).integrate(
        rows, a, b, n, getattr(native.Rule, rule), 0, n, native.HostPool(4))


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("n", [1, 3, 511, 512, 513, 2051])
def test_sweep_edges_of_the_lane_split(native, cuda, n):
    """grid = 2 (512 lanes): fewer samples than lanes, the remainder lanes, a per-lane count
    that is no multiple of 4. The midpoint rule of a line is exact: p0/2 + p1."""
    rows = [[1.0, 0.0], [2.0, 1.0], [-3.0, 0.5]]
    v = _sweep("p0*x+p1", rows, 0.0, 1.0, n, rule="mid", grid=2)
    assert v.shape == (3,)
    assert v.tolist() == pytest.approx(list(_host(native, "p0*x+p1", rows, 0.0, 1.0, n, "mid")),
                                       rel=1e-13)
    assert v.tolist() == pytest.approx([p0 / 2 + p1 for p0, p1 in rows], rel=1e-13)


def test_sweep_rows_are_independent_bitwise(native, cuda):
    n = 100_003
    ps = np.linspace(0.5, 4.0, 8).tolist()
    v = _sweep(DECAY, _rows(ps), 0.0, 2.0, n)
    assert _bits(_sweep(DECAY, _rows(ps), 0.0, 2.0, n)) == _bits(v)  # a second call
    for k, p in enumerate(ps):  # each row alone
        assert _bits(_sweep(DECAY, [[p]], 0.0, 2.0, n)) == _bits(v[k:k + 1])
    assert _bits(_sweep(DECAY, _rows(ps[::-1]), 0.0, 2.0, n)) == _bits(v[::-1])
    many = np.linspace(0.1, 5.0, 33).tolist()
    many[29] = many[4] = ps[3]  # a repeated row among 33
    w = _sweep(DECAY, _rows(many), 0.0, 2.0, n)
    assert _bits(w[4:5]) == _bits(w[29:30]) == _bits(v[3:4])
    # another sample split: equal to rounding, not bitwise
    assert _sweep(DECAY, _rows(ps), 0.0, 2.0, n, grid=7).tolist() == pytest.approx(v.tolist(),
                                                                                  rel=1e-14)


def test_sweep_midpoint_analytic(cuda):
    n = 4_000_001
    v = _sweep(DECAY, _rows(DECAY_P), 0.0, 2.0, n, rule="mid")
    assert v.tolist() == pytest.approx([1 - math.exp(-2 * p) for p in DECAY_P], rel=1e-9)
    v = _sweep(LORENTZ, _rows(LORENTZ_P), 0.0, 1.0, n, rule="mid")
    assert v.tolist() == pytest.approx([math.atan(math.sqrt(p)) / math.sqrt(p)
                                        for p in LORENTZ_P], rel=1e-9)


def test_sweep_gpu_against_host(native, cuda):
    n = 200_001
    for expr, ps, b in ((DECAY, DECAY_P, 2.0), (LORENTZ, LORENTZ_P, 1.0)):
        v = _sweep(expr, _rows(ps), 0.0, b, n, rule="mid")
        assert v.tolist() == pytest.approx(list(_host(native, expr, _rows(ps), 0.0, b, n, "mid")),
                                           rel=1e-12)


def test_sweep_without_parameters(cuda):
    """nparams = 0: K identical rows, and the value ExprIntegrator gives for the same f."""
    n = 1_000_003
    v = _sweep("4.0/(1.0+x*x)", [[], [], []], 0.0, 1.0, n)
    assert v.shape == (3,) and len(set(_bits(v))) == 1
    assert v[0] == pytest.approx(kernels.riemann_expr("4.0/(1.0+x*x)", 0.0, 1.0, n), rel=1e-14)


def test_sweep_slices_and_ranks(native, cuda):
    n = 1_234_567
    rows = _rows(DECAY_P)
    whole = _sweep(DECAY, rows, 0.0, 2.0, n)
    parts = [_sweep(DECAY, rows, 0.0, 2.0, n, i_begin=b, n_local=c)
             for b, c in (rank_slice(n, r, 4) for r in range(4))]
    for k in range(len(rows)):
        assert math.fsum(p[k] for p in parts) == pytest.approx(whole[k], rel=1e-14)

    def body(rank, comm):
        es = native.ExprSweep(DECAY, 1, 0)
        b, c = rank_slice(n, rank, 3)
        return es.integrate(rows, 0.0, 2.0, n, native.Rule.left, b, c, 1.0, comm)
    out = loopback.run_ranks(3, body)
    for v in out:
        assert _bits(v) == _bits(out[0])
        assert v.tolist() == pytest.approx(whole.tolist(), rel=1e-14)


def test_sweep_many_small_rows(native, cuda):
    """The regime the launch shape exists for: one sample slice, 2048 row lanes."""
    k, n = 4096, 1000
    assert native.expr_sweep_shape(n, k) == (1, 2048)
    rows = _rows(np.linspace(0.1, 10.0, k).tolist())
    v = _sweep("exp(-p0*x*x)", rows, 0.0, 2.0, n, rule="mid")
    assert v.shape == (k,)
    np.testing.assert_allclose(v, _host(native, "exp(-p0*x*x)", rows, 0.0, 2.0, n, "mid"),
                               rtol=1e-12, atol=0.0)


def test_sweep_sample_indices_past_32_bits(cuda):
    """Samples 2^33 .. 2^33 + 1024 of the 2^40-sample left rule of x on [0, 2^40] (h = 1):
    the sum of those integers, exactly representable at every step."""
    i0, c, n = 2**33, 1025, 2**40
    v = _sweep("x", [[]], 0.0, float(n), n, i_begin=i0, n_local=c)
    assert v.tolist() == pytest.approx([float(sum(range(i0, i0 + c)))], rel=1e-15)


def test_sweep_argument_errors(native, cuda):
    with pytest.raises(RuntimeError, match="non-finite"):
        kernels.riemann_expr_sweep(DECAY, [[1.0], [float("nan")]], 0.0, 2.0, 1000)
    with pytest.raises(ValueError):  # ragged rows
        kernels.riemann_expr_sweep("p0*x+p1", [[1.0, 2.0], [3.0]], 0.0, 1.0, 1000)
    es = native.ExprSweep("p0*x+p1", 2, 0)
    with pytest.raises(RuntimeError, match="nparams"):  # a row of the wrong width
        es.integrate([[1.0, 2.0, 3.0]], 0.0, 1.0, 1000, native.Rule.left, 0, 1000)
    with pytest.raises(RuntimeError, match="slice"):
        es.integrate([[1.0, 2.0]], 0.0, 1.0, 1000, native.Rule.left, 500, 501)
    assert es.integrate([], 0.0, 1.0, 1000, native.Rule.left, 0, 1000).shape == (0,)
    empty = kernels.riemann_expr_sweep(DECAY, [], 0.0, 2.0, 1000)
    assert empty.shape == (0,) and empty.is_cuda and empty.dtype.is_floating_point


def test_integrate_expr_sweep_hip_api(cuda):
    from cuda_v_mpi_amd import integrate_expr_sweep

    r = integrate_expr_sweep(DECAY, _rows(DECAY_P), 0.0, 2.0, n=200_001, rule="mid",
                             analytic=[1 - math.exp(-2 * p) for p in DECAY_P])
    assert r.rows == 4 and r.nparams == 1 and r.seconds > 0
    assert r.values == _sweep(DECAY, _rows(DECAY_P), 0.0, 2.0, 200_001, rule="mid").tolist()
    assert max(r.abs_err) < 1e-9  # midpoint truncation at this n: h^2/24 |f'(b) - f'(a)| < 7e-11


@pytest.mark.parametrize("ranks", [[], ["--loopback", "2"]])
def test_cli_riemann_sweep(cuda, ranks):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        pytest.skip("CLI not built")
    p = subprocess.run([exe, "--expr", DECAY, "--a", "0", "--b", "2", "--n", "1e6", "--rule",
                        "mid", "--linspace", "p0=0.5:4:8", "--json", "--iters", "3", *ranks],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.splitlines()[-1])
    assert rec["rows"] == 8 and rec["nparams"] == 1 and len(rec["values"]) == 8
    assert rec["values"] == pytest.approx([1 - math.exp(-2 * q) for q in np.linspace(0.5, 4, 8)],
                                          rel=1e-9)
    assert rec["ms_per_sweep"] > 0 and rec["subintervals_per_s"] > 0
    assert rec["comm"] == ("loopback" if ranks else "none")
