"""Parameter sweeps of a runtime integrand (miint/expr.hpp, ExprSweep / HostExprSweep) on
the CPU: the generated kernel source, the hipRTC compile for gfx950 without a device, the
launch shape as a property, the host sweep against numpy, HostExpr, threads and rank slices,
and the CLI's --params reader. GPU numerics: tests/test_expr_sweep_gpu.py."""
from __future__ import annotations

import json
import os
import random
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = {"left": 0.0, "mid": 0.5, "right": 1.0}


def test_sweep_source_wraps_the_expression(native):
    src = native.expr_sweep_source("exp(-p0*x*x)", 1)
    assert "miint_fp(double x, double p0) { return (exp(-p0*x*x)); }" in src
    assert "miint_expr_sweep_partials" in src and "miint_expr_sweep_close" in src
    assert "const double* __restrict__ params" in src
    assert "miint_fp(double x) {" in native.expr_sweep_source("x", 0)


def test_sweep_compiles_for_gfx950_without_a_device(native):
    code = native.expr_sweep_compile("exp(-p0*x*x)", 1)
    assert code[:4] == b"\x7fELF" or code[:4] == b"__CL"  # code object (or offload bundle)
    assert native.expr_sweep_compile("exp(-p0*x*x)", 1) == code
    assert native.expr_sweep_compile("exp(-p0*x*x)", 2) != b""  # its own cache entry


def test_sweep_nparams_and_unknown_parameter(native):
    with pytest.raises(RuntimeError, match="nparams"):
        native.expr_sweep_source("x", 9)
    with pytest.raises(RuntimeError, match="nparams"):
        native.expr_sweep_source("x", -1)
    with pytest.raises(RuntimeError, match="does not compile"):
        native.expr_sweep_compile("x*p1", 1)
    with pytest.raises(RuntimeError, match="nparams"):
        native.HostExprSweep("x", 9)
    with pytest.raises(RuntimeError, match="does not compile"):
        native.HostExprSweep("x*p1", 1)


@pytest.mark.parametrize("bad", ["x; x", "x) { return 0", "asm(\"s_nop 0\")", "asm (x)",
                                 "__builtin_amdgcn_s_sleep(1)", "x\\", "#define y", "'a'",
                                 "", "x" * 5000,
                                 "x <% return 0; %>", "x <: 0 :>", "%:define y", "x%>",
                                 "(<%%>)"])
def test_sweep_rejects_what_expr_source_rejects(native, bad):
    """The strings tests/test_expr_cpu.py refuses for expr_source, through the sweep."""
    with pytest.raises(RuntimeError, match="expression"):
        native.expr_source(bad)
    with pytest.raises(RuntimeError, match="expression"):
        native.expr_sweep_source(bad, 1)


def test_sweep_shape_properties(native):
    """gx depends on n_local and grid only; 1 <= gx <= 2048; 1 <= gy <= rows; a lane's share
    of the samples fits the kernel's 32-bit count, or the call raises."""
    rng = random.Random(20251)
    cases = [(1, 1), (1, 1 << 20), (1 << 40, 1), (1 << 40, 1 << 20), (1000, 4096),
             (10**6, 4096), (10**9, 8)]
    cases += [(int(2 ** rng.uniform(0, 40)), int(2 ** rng.uniform(0, 20))) for _ in range(300)]
    raised = 0
    for n_local, rows in cases:
        rows2 = rng.randint(1, 1 << 20)
        for grid in (0, 1, 3, 2048):
            try:
                gx, gy = native.expr_sweep_shape(n_local, rows, grid)
            except RuntimeError as e:
                assert "32-bit" in str(e)
                assert grid and -(-n_local // (grid * 256)) >= 2**32 - 1
                with pytest.raises(RuntimeError, match="32-bit"):  # whatever the row count
                    native.expr_sweep_shape(n_local, rows2, grid)
                raised += 1
                continue
            assert 1 <= gx <= 2048 and 1 <= gy <= rows
            assert gx == grid or grid == 0
            assert -(-n_local // (gx * 256)) < 2**32
            assert native.expr_sweep_shape(n_local, rows2, grid)[0] == gx
    assert raised >= 1  # (2^40, grid 1): 2^32 samples per lane
    assert native.expr_sweep_shape(1000, 4096) == (1, 2048)  # many small rows
    assert native.expr_sweep_shape(10**9, 8) == (2048, 1)    # few large rows
    for bad in ((10, 0, 0), (10, (1 << 20) + 1, 0), (10, 1, 2049), (10, 1, -1)):
        with pytest.raises(RuntimeError):
            native.expr_sweep_shape(*bad)


def _numpy_rows(f, rows, a, b, n, rule):
    """h * sum of f(a + (i + off) h, row) with the host's sample positions (one fma per
    sample is within an ulp of this) and an exact sum."""
    import math

    h = (b - a) / n
    x = a + (np.arange(n, dtype=np.float64) + OFF[rule]) * h
    return [math.fsum(f(x, *row)) * h for row in rows]


@pytest.mark.parametrize("rule", ["left", "mid", "right"])
def test_host_sweep_against_numpy(native, rule):
    n = 4097
    pool = native.HostPool(2)
    lin = [[1.0, 0.5], [2.0, 1.0], [0.25, 3.0]]
    v = native.HostExprSweep("p0*x+p1", 2).integrate(lin, 0.0, 1.0, n, getattr(native.Rule, rule),
                                                    0, n, pool)
    assert list(v) == pytest.approx(_numpy_rows(lambda x, p0, p1: p0 * x + p1, lin, 0.0, 1.0, n,
                                                rule), rel=1e-13)
    gau = [[0.5], [1.0], [2.0], [7.5]]
    v = native.HostExprSweep("exp(-p0*x*x)", 1).integrate(np.array(gau), -1.0, 2.0, n,
                                                         getattr(native.Rule, rule), 0, n, pool)
    assert v.shape == (4,) and v.dtype == np.float64
    assert list(v) == pytest.approx(_numpy_rows(lambda x, p0: np.exp(-p0 * x * x), gau, -1.0, 2.0,
                                                n, rule), rel=1e-13)


def test_host_sweep_row_equals_host_expr(native):
    """A sweep row is HostExpr of the expression with the literal substituted (1e-14, the
    bound tests/test_expr_gpu.py uses between two per-sample algorithms)."""
    n = 100_003
    pool = native.HostPool(3)
    v = native.HostExprSweep("exp(-p0*x*x)", 1).integrate([[2.0], [0.5]], 0.0, 3.0, n,
                                                         native.Rule.mid, 0, n, pool)
    one = native.HostExpr("exp(-2.0*x*x)").integrate(0.0, 3.0, n, native.Rule.mid, 0, n, pool)
    assert v[0] == pytest.approx(one, rel=1e-14)
    assert v[1] != v[0]


def test_host_sweep_threads_and_rank_slices(native):
    from cuda_v_mpi_amd.parallel.decomposition import rank_slice

    n = 300_017
    rows = [[0.5], [1.0], [4.0]]
    hs = native.HostExprSweep("p0*exp(-p0*x)", 1)
    p5 = native.HostPool(5)
    v1 = hs.integrate(rows, 0.0, 2.0, n, native.Rule.left, 0, n, native.HostPool(1))
    v5 = hs.integrate(rows, 0.0, 2.0, n, native.Rule.left, 0, n, p5)
    assert list(v5) == pytest.approx(list(v1), rel=1e-15)
    parts = [hs.integrate(rows, 0.0, 2.0, n, native.Rule.left, *rank_slice(n, r, 3), p5)
             for r in range(3)]
    assert list(np.sum(parts, axis=0)) == pytest.approx(list(v5), rel=1e-15)


def test_host_sweep_argument_checks(native):
    pool = native.HostPool(1)
    hs = native.HostExprSweep("p0*x+p1", 2)
    assert hs.nparams == 2 and hs.expression == "p0*x+p1"
    assert hs.integrate([], 0.0, 1.0, 10, native.Rule.left, 0, 10, pool).shape == (0,)
    with pytest.raises(RuntimeError, match="nparams"):
        hs.integrate([[1.0, 2.0, 3.0]], 0.0, 1.0, 10, native.Rule.left, 0, 10, pool)
    with pytest.raises(RuntimeError, match="rows"):
        hs.integrate([[1.0, 2.0], [3.0]], 0.0, 1.0, 10, native.Rule.left, 0, 10, pool)
    with pytest.raises(RuntimeError, match="non-finite"):
        hs.integrate([[1.0, float("nan")]], 0.0, 1.0, 10, native.Rule.left, 0, 10, pool)
    with pytest.raises(RuntimeError, match="slice"):
        hs.integrate([[1.0, 2.0]], 0.0, 1.0, 10, native.Rule.left, 5, 6, pool)
    h0 = native.HostExprSweep("4.0/(1.0+x*x)", 0)  # no parameters: K identical rows
    v = h0.integrate([[], [], []], 0.0, 1.0, 1001, native.Rule.mid, 0, 1001, pool)
    assert v.shape == (3,) and v[0] == v[1] == v[2] == pytest.approx(np.pi, rel=1e-6)


def test_param_file_reader(native, tmp_path):
    f = tmp_path / "rows.txt"
    f.write_text("# width, offset\n1.0, 0.5\n\n2e0\t1   # trailing comment\n-3;0.5\n")
    rows = native.load_param_rows(str(f))
    assert rows.tolist() == [[1.0, 0.5], [2.0, 1.0], [-3.0, 0.5]]
    assert native.linspace_param_rows("p0=0.5:4:8").ravel().tolist() == \
        pytest.approx(np.linspace(0.5, 4.0, 8).tolist(), rel=1e-15)
    assert native.linspace_param_rows("p0=2:3:1").tolist() == [[2.0]]
    for bad in ("p1=0:1:3", "p0=0:1", "p0=0:1:0", "p0=0:1:2.5", "0:1:3"):
        with pytest.raises(RuntimeError, match="linspace"):
            native.linspace_param_rows(bad)


def test_integrate_expr_sweep_host_api(native):
    import math

    from cuda_v_mpi_amd import integrate_expr_sweep

    ps = [0.5, 1.0, 2.0]
    r = integrate_expr_sweep("p0*exp(-p0*x)", [[p] for p in ps], 0.0, 2.0, n=200_001, rule="mid",
                             backend="host", threads=2,
                             analytic=[1 - math.exp(-2 * p) for p in ps])
    assert r.rows == 3 and r.nparams == 1 and max(r.abs_err) < 1e-10
    assert r.subintervals_per_s == pytest.approx(3 * 200_001 / r.seconds)
    with pytest.raises(ValueError):
        integrate_expr_sweep("p0*x", [[1.0]], 0, 1, backend="cpu")


def _cli(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        pytest.skip("CLI not built")
    return subprocess.run([exe, "--device", "cpu", *args], capture_output=True, text=True,
                          timeout=120)


def test_cli_host_sweep(native, tmp_path):
    f = tmp_path / "rows.txt"
    f.write_text("# p0 p1\n1 0\n2, 1\n-3 0.5\n")
    p = _cli("--expr", "p0*x+p1", "--a", "0", "--b", "1", "--n", "4097", "--rule", "mid",
             "--threads", "2", "--params", str(f), "--json")
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.splitlines()[-1])
    want = native.HostExprSweep("p0*x+p1", 2).integrate(
        [[1, 0], [2, 1], [-3, 0.5]], 0.0, 1.0, 4097, native.Rule.mid, 0, 4097, native.HostPool(2))
    assert rec["rows"] == 3 and rec["nparams"] == 2 and rec["values"] == list(want)
    assert rec["ms_per_sweep"] > 0 and rec["subintervals_per_s"] > 0 and rec["device"] == "cpu"
    # without --json: one line per row, index, parameters, value
    p = _cli("--expr", "p0*x+p1", "--a", "0", "--b", "1", "--n", "4097", "--rule", "mid",
             "--params", str(f))
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 3 and lines[1].split() == ["1", "2", "1", "%.13g" % want[1]]
    p = _cli("--expr", "exp(-p0*x*x)", "--a", "0", "--b", "1", "--n", "1000", "--linspace",
             "p0=1:2:3", "--json")
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout.splitlines()[-1])["rows"] == 3


def test_python_cli_host_sweep(native, tmp_path):
    import sys

    f = tmp_path / "rows.txt"
    f.write_text("1 0\n2, 1\n")
    p = subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", "--expr", "p0*x+p1",
                        "--a", "0", "--b", "1", "--n", "1001", "--rule", "mid", "--params",
                        str(f), "--device", "cpu", "--json"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.splitlines()[-1])
    assert rec["rows"] == 2 and rec["nparams"] == 2
    assert rec["values"] == pytest.approx([0.5, 2.0], rel=1e-13)


def test_cli_sweep_bad_files(tmp_path):
    ragged = tmp_path / "ragged.txt"
    ragged.write_text("1 2\n3 4\n# comment\n5\n")
    p = _cli("--expr", "p0*x+p1", "--params", str(ragged), "--n", "100")
    assert p.returncode != 0 and "ragged.txt:4: row 2 has 1 values" in p.stderr
    empty = tmp_path / "empty.txt"
    empty.write_text("# nothing\n\n")
    p = _cli("--expr", "p0*x", "--params", str(empty), "--n", "100")
    assert p.returncode != 0 and "no parameter rows (row 0" in p.stderr
    p = _cli("--params", str(ragged), "--n", "100")  # a sweep needs --expr
    assert p.returncode != 0 and "--expr" in p.stderr
