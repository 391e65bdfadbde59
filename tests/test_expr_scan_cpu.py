"""CPU side of the running-integral tests (csrc/runtime/expr_scan.cpp): the inputs of
test_expr_scan_gpu.py keep their exactness budgets and their tile structure, the integer
reference agrees with rational arithmetic, and everything that needs no device works without
one: the output count, the guards, the generated source and its hipRTC compile for gfx950,
the torch form of integrate_expr_running and the CLI's --help."""
from __future__ import annotations

import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import expr_exact_cases as ec
import expr_scan_cases as sc
from cuda_v_mpi_amd.utils import exact_riemann as xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fraction_prefixes(c, rule, begin, count):
    """h * running sums of p(x_i) over samples begin .. begin + count - 1, in rationals."""
    h = Fraction(1, 2 ** c.at.k)
    out, run = [], Fraction(0)
    for i in range(begin, begin + count):
        x = Fraction(c.at.a_num + 2 * i + ec.OFF2[rule], 2 ** (c.at.k + 1))
        run += sum(Fraction(cj) * x ** j for j, cj in enumerate(c.coef))
        out.append(run * h)
    return out


@pytest.mark.parametrize("rule", ec.RULES)
def test_cumsum_reference_against_fractions(rule):
    """The int64 cumsum reference against brute force in rationals, at small n: whole values,
    every = 3 from an odd begin (the global-index phase), scale = 0.25, and a sum that starts
    below the slice (a carried-in rank)."""
    for c, begin, count in ((sc.CUBIC, 0, 40), (sc.QUADRATIC, 5, 50), (sc.LONG, 7, 33),
                            (sc.PAST_2_32, 2**33 + 1, 30)):
        want = _fraction_prefixes(c, rule, begin, count)
        got = sc.running_ref(c, rule, begin, count)
        assert [Fraction(float(v)) for v in got] == want, c.name
        idx = [i for i in range(begin, begin + count) if (i + 1) % 3 == 0]
        assert sc.selected(begin, count, 3).tolist() == idx
        got3 = sc.running_ref(c, rule, begin, count, every=3, scale=0.25)
        assert [Fraction(float(v)) for v in got3] == [want[i - begin] / 4 for i in idx], c.name
        assert Fraction(sc.total_ref(c, rule, begin, count)) == want[-1]
    c = sc.QUADRATIC
    whole = _fraction_prefixes(c, rule, 0, 60)
    got = sc.running_ref(c, rule, 20, 40, every=7, start=0)
    assert [Fraction(float(v)) for v in got] == [whole[i] for i in range(20, 60) if (i + 1) % 7 == 0]


def test_every_case_keeps_its_budget():
    """expr_budget_bits bounds every partial sum of a case's samples in any order: below 53
    every prefix is exact under any association. Pinned to one decimal."""
    for c in sc.ALL_CASES:
        b = ec.poly_budget(c.coef, c.at)
        print(f"{c.name}: {b:.2f} bits")
        assert b < xr.F64_BITS, c.name
        assert round(b, 1) == sc.BUDGETS[c.name], c.name
    # and the running values themselves get there: LONG's reach 47 bits
    p = sc._prefix_ints("long", "left")
    assert 46 < np.log2(float(np.abs(p).max())) < 47.9


def test_tile_census(native):
    """The structure the GPU tests rely on: under one tile, 8 tiles + 37, 512 + 3, more tiles
    than the prefix workgroup has threads (a thread walks two runs) and more than the sums
    pass has workgroups (a workgroup walks two tiles, the last run is one ragged tile)."""
    assert native.EXPR_SCAN_TILE == sc.TILE
    for c in sc.ALL_CASES:
        assert divmod(c.at.span[1], sc.TILE) == sc.TILE_CENSUS[c.name], c.name
        assert native.expr_scan_shape(c.at.span[1]) == sc.SHAPES[c.name], c.name
    tiles, run, runs = sc.SHAPES["long"]
    assert run == 1 and runs > sc.PREFIX_THREADS and -(-runs // sc.PREFIX_THREADS) == 2
    tiles, run, runs = sc.SHAPES["wide"]
    assert tiles > sc.MAX_RUNS and run == 2 and runs > sc.PREFIX_THREADS and tiles % run == 1
    # the shape is a function of the count alone, never more than 2048 runs
    assert native.expr_scan_shape(sc.MAX_RUNS * sc.TILE) == (2048, 1, 2048)
    assert native.expr_scan_shape(sc.MAX_RUNS * sc.TILE + 1) == (2049, 2, 1025)
    assert native.expr_scan_shape(native.EXPR_SCAN_MAX_TILES * sc.TILE) == (2**22, 2048, 2048)
    assert native.expr_scan_shape(0) == (0, 1, 0)
    assert sc.PAST_2_32.at.begin > 2**32
    assert ec.EDGE_BEGIN + max(sc.EDGE_COUNTS) <= sc.QUADRATIC.at.n


def test_outputs_against_brute_force(native):
    rng = random.Random(7)
    for _ in range(300):
        begin, count, every = rng.randrange(0, 200), rng.randrange(0, 200), rng.randrange(1, 50)
        want = sum(1 for i in range(begin, begin + count) if (i + 1) % every == 0)
        assert native.expr_scan_outputs(begin, count, every) == want, (begin, count, every)
        assert len(sc.selected(begin, count, every)) == want
    assert native.expr_scan_outputs(2**33 + 1, 5121, 1) == 5121
    assert native.expr_scan_outputs(2**63, 2**63 - 1, 2**62) == 1
    assert native.expr_scan_outputs(5, 100, 106) == 0
    with pytest.raises(RuntimeError, match="every must be >= 1"):
        native.expr_scan_outputs(0, 10, 0)
    with pytest.raises(RuntimeError, match="wraps"):
        native.expr_scan_outputs(2**64 - 1, 2, 1)


def test_check_refusals(native):
    """Every refusal of expr_scan_check names the numbers; what it accepts passes silently."""
    native.expr_scan_check(1000, 5, 995, 1, 995)
    native.expr_scan_check(1000, 5, 995, 37, 27)
    native.expr_scan_check(1000, 1000, 0, 1, 0)          # an empty slice at the end
    native.expr_scan_check(2**40, 2**33 + 1, 5121, 1, 5121)
    with pytest.raises(RuntimeError, match=r"samples \[5, 5 \+ 996\) lie outside \[0, n = 1000\)"):
        native.expr_scan_check(1000, 5, 996, 1, 996)
    with pytest.raises(RuntimeError, match="lie outside"):
        native.expr_scan_check(0, 0, 0, 1, 0)
    with pytest.raises(RuntimeError, match=r"samples \[18446744073709551615, .* wrap around"):
        native.expr_scan_check(1000, 2**64 - 1, 2, 1, 2)
    with pytest.raises(RuntimeError, match="every must be >= 1"):
        native.expr_scan_check(1000, 0, 1000, 0, 1000)
    with pytest.raises(RuntimeError, match=r"holds 26 values, .* every = 37 write 27"):
        native.expr_scan_check(1000, 5, 995, 37, 26)
    most = native.EXPR_SCAN_MAX_TILES * sc.TILE
    native.expr_scan_check(2**40, 3, most, 2**20, most // 2**20 + 1)
    with pytest.raises(RuntimeError, match=rf"{most + 1} samples are {native.EXPR_SCAN_MAX_TILES + 1} tiles"):
        native.expr_scan_check(2**40, 3, most + 1, 2**20, most)


def test_scan_source_and_expression_rules(native):
    src = native.expr_scan_source("exp(-x*x)")
    for name in ("miint_expr_scan_tile_sums", "miint_expr_scan_tile_prefix",
                 "miint_expr_scan_write"):
        assert f'extern "C" __global__' in src and name in src
    assert "return (exp(-x*x));" in src
    # what expr_check rejects, expr_scan_source rejects
    for bad in ("x; x", "x } {", 'x + "s"', "asm(x)", "__builtin_amdgcn_s_sleep(1)", "x <% 1", ""):
        with pytest.raises(RuntimeError):
            native.expr_source(bad)
        with pytest.raises(RuntimeError):
            native.expr_scan_source(bad)
        with pytest.raises(RuntimeError):
            native.expr_scan_compile(bad)


def test_scan_compiles_for_gfx950_without_a_device(native):
    code = native.expr_scan_compile("exp(-x*x)")
    assert code[:4] == b"\x7fELF" and len(code) > 4096
    assert native.expr_scan_compile("exp(-x*x)") == code       # cached
    assert native.expr_scan_compile("(7.0*x-5.0)*x+3.0") != code
    with pytest.raises(RuntimeError, match="does not compile"):
        native.expr_scan_compile("x + y")


def test_integrate_expr_running_cpu_backend():
    """The torch form: cumsum of the per-sample values. On the quadratic it has the bits of
    the integer reference for every rule, whole and decimated; x[j] is the upper limit."""
    from cuda_v_mpi_amd import RunningResult, integrate_expr_running

    c = sc.QUADRATIC
    h = 2.0 ** -c.at.k
    for rule in ec.RULES:
        for every in (1, 37):
            r = integrate_expr_running(c.expr, c.at.a, c.at.b, c.at.n, rule=rule, every=every,
                                       backend="cpu")
            assert isinstance(r, RunningResult) and r.values.dtype == torch.float64
            assert sc.same_bits(r.values.numpy(), sc.running_ref(c, rule, 0, c.at.n, every))
            assert r.total == sc.total_ref(c, rule, 0, c.at.n)
            j = np.arange(1, c.at.n // every + 1)
            assert sc.same_bits(r.x.numpy(), c.at.a + j * (every * h))
    # a transcendental integrand against the closed form: erf from its density
    import math

    # h = 2**-14: the midpoint rule's error is below 3 h^2 max|f''| / 24 = 1e-9
    r = integrate_expr_running("exp(-x*x)", 0.0, 3.0, 3 << 14, rule="mid", every=1 << 14,
                               backend="cpu")
    want = [math.sqrt(math.pi) / 2 * math.erf(x) for x in (1.0, 2.0, 3.0)]
    assert r.x.tolist() == [1.0, 2.0, 3.0]
    assert np.allclose(r.values.numpy(), want, rtol=0, atol=1e-9)
    assert abs(r.total - want[-1]) < 1e-9
    with pytest.raises(ValueError, match="cpu backend"):
        integrate_expr_running("x > 1.0 ? x : 0.0", 0, 1, 10, backend="cpu")
    with pytest.raises(ValueError, match="cpu backend"):
        integrate_expr_running("__import__(x)", 0, 1, 10, backend="cpu")
    with pytest.raises(ValueError, match="backend must be"):
        integrate_expr_running("x", 0, 1, 10, backend="host")
    with pytest.raises(ValueError, match="every >= 1"):
        integrate_expr_running("x", 0, 1, 10, every=0, backend="cpu")


def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


def test_cli_help_documents_running():
    p = _riemann("--help")
    assert p.returncode == 0 and p.stdout.startswith("usage: riemann")
    for word in ("--running", "--every K", "--running-out FILE", "10000"):
        assert word in p.stdout, word


def test_cli_running_refusals_need_no_device():
    """What the CLI refuses before it touches a device: more than 10 000 lines, the
    multi-rank forms, the host engine, a sweep, and the knobs without --running."""
    base = ("--expr", "x", "--a", "0", "--b", "1")
    p = _riemann(*base, "--n", "10001", "--running")
    assert p.returncode == 1 and "--every" in p.stderr and "--running-out" in p.stderr
    assert "10001 lines" in p.stderr
    for extra, word in ((("--gpus", "2"), "one-rank"), (("--loopback", "2"), "one-rank"),
                        (("--device", "cpu"), "no host engine"),
                        (("--linspace", "p0=0:1:3"), "one expression"),
                        (("--every", "0"), "--every must be >= 1")):
        p = _riemann(*base, "--n", "100", "--running", *extra)
        assert p.returncode == 1 and word in p.stderr, (extra, p.stderr)
    p = _riemann(*base, "--n", "100", "--every", "3")
    assert p.returncode == 1 and "belong to --running" in p.stderr
    p = _riemann("--n", "100", "--running")
    assert p.returncode == 1 and "--expr" in p.stderr
    p = subprocess.run([os.path.join(REPO, "build", "bin", "riemann"), *base, "--n", "100",
                        "--running"], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p.returncode == 1 and "one-rank" in p.stderr
