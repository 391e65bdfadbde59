"""Exact tests of the running-integral kernels (csrc/runtime/expr_scan.cpp, ExprScan): every
value written is compared bit for bit with an integer reference, no tolerance.

The expressions are polynomials in x with integer coefficients on h = 2**-k grids
(expr_scan_cases.py; test_expr_scan_cpu.py shows on any box that each keeps its budget), so
x = fma(idx, h, a), every Horner step, the thread's serial scan, the wave and workgroup scans,
the tile sums, the tile prefix, the rank carries and the final scaling by a power of two are
exact in any order: F_i must have the bits of the int64 cumsum. A sample dropped or doubled
at a thread, wave, workgroup or tile edge, a tile prefix off by one tile, a wrong output
position or decimation phase, a carry added twice: each moves a value by at least one unit.
One transcendental integrand is held to a derived rounding bound instead.
"""
from __future__ import annotations

import json
import math
import os
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import expr_exact_cases as ec
import expr_scan_cases as sc
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.parallel import loopback

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 8     # sentinel slots behind the outputs: a store past the output count shows


@pytest.fixture(scope="module")
def scanner(native, cuda):
    made = {}

    def get(expr: str):
        if expr not in made:
            made[expr] = native.ExprScan(expr, cuda.index)
        return made[expr]
    return get


def _run(native, es, at, rule, begin, count, every=1, scale=1.0, comm=None):
    """One launch into a NaN-filled buffer of outputs + PAD slots: (values, record); the PAD
    slots behind the outputs must come back untouched."""
    outputs = native.expr_scan_outputs(begin, count, every)
    out = torch.full((outputs + PAD,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the scan runs on its own stream
    rec = es.run(at.a, at.b, at.n, getattr(native.Rule, rule), begin, count, every,
                 out.data_ptr(), outputs, scale, comm)
    got = out.cpu().numpy()
    assert rec["outputs"] == outputs
    assert np.isnan(got[outputs:]).all(), "a store past the output count"
    return got[:outputs], rec


def _expect(got, want, what: str) -> None:
    got, want = np.asarray(got), np.asarray(want)
    same = sc.same_bits(got, want)
    if not same and got.shape == want.shape:
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        print(f"{what}: {len(bad)} of {len(want)} differ"
              + "".join(f"\n  [{i}] got {got[i]!r} want {want[i]!r}" for i in bad[:8]))
    assert same, f"{what}: {got.shape} values against {want.shape}"


# ------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("rule", ec.RULES)
@pytest.mark.parametrize("case", sc.POLY_CASES, ids=lambda c: c.name)
def test_whole_rule_exact(native, scanner, case, rule):
    """Under one tile, 8 tiles + 37, 512 + 3, 1027 + 5 (a prefix thread walks two runs) and
    2052 + 7 (a workgroup walks two tiles, the last run is one tile): every F_i, the total."""
    at = case.at
    got, rec = _run(native, scanner(case.expr), at, rule, 0, at.n)
    _expect(got, sc.running_ref(case, rule, 0, at.n), f"{case.name} {rule}")
    assert rec["total"] == sc.total_ref(case, rule, 0, at.n) == got[-1]
    assert rec["device_ms"] > 0


# ------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("rule", ec.RULES)
def test_edge_counts_exact(native, scanner, rule):
    c = sc.QUADRATIC
    for m in sc.EDGE_COUNTS:
        got, rec = _run(native, scanner(c.expr), c.at, rule, sc.EDGE_BEGIN, m)
        _expect(got, sc.running_ref(c, rule, sc.EDGE_BEGIN, m), f"count {m} {rule}")
        assert rec["total"] == sc.total_ref(c, rule, sc.EDGE_BEGIN, m), m


# ------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("case", [sc.QUADRATIC, sc.FULL_LANES], ids=lambda c: c.name)
def test_every_exact(native, scanner, case):
    """Decimation from an odd begin: the values, their count, the global-index phase (the
    reference selects (i + 1) % every == 0 on global i), tiles that hold no output
    (every >= 4096 leaves most without one), one output and none."""
    at = case.at
    begin, count = sc.EDGE_BEGIN, at.n - sc.EDGE_BEGIN
    for k, every in enumerate(sc.every_values(count)):
        rule = ec.RULES[k % 3]
        got, rec = _run(native, scanner(case.expr), at, rule, begin, count, every)
        want = sc.running_ref(case, rule, begin, count, every)
        assert len(want) == (begin + count) // every - begin // every
        _expect(got, want, f"{case.name} every {every} {rule}")
        assert rec["total"] == sc.total_ref(case, rule, begin, count), every
    tiles = -(-count // sc.TILE)
    assert native.expr_scan_outputs(begin, count, 10000) < tiles  # tiles without an output
    # no output at all: the total is still the slice's
    for m, every in ((4097, 5000), (100, 106), (count, at.n + 1)):
        assert native.expr_scan_outputs(begin, m, every) == 0
        got, rec = _run(native, scanner(case.expr), at, "mid", begin, m, every)
        assert got.size == 0 and rec["total"] == sc.total_ref(case, "mid", begin, m)
    # the phase follows the global index: the same every from another begin
    got, _ = _run(native, scanner(case.expr), at, "left", 36, 1000, 37)
    _expect(got, sc.running_ref(case, "left", 36, 1000, 37), "begin 36 every 37")
    assert len(got) == 28 and sc.selected(36, 1000, 37)[0] == 36


# ------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("rule", ec.RULES)
def test_scale_exact(native, scanner, rule):
    for c, every in ((sc.CUBIC, 1), (sc.QUADRATIC, 1), (sc.QUADRATIC, 37)):
        got, rec = _run(native, scanner(c.expr), c.at, rule, 0, c.at.n, every, 0.25)
        _expect(got, sc.running_ref(c, rule, 0, c.at.n, every, 0.25), f"{c.name} x 0.25")
        assert rec["total"] == sc.total_ref(c, rule, 0, c.at.n, 0.25)


# ------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("rule", ec.RULES)
def test_samples_past_32_bits_exact(native, scanner, rule):
    c = sc.PAST_2_32
    b, m = c.at.span
    for every in (1, 1000):
        got, rec = _run(native, scanner(c.expr), c.at, rule, b, m, every)
        _expect(got, sc.running_ref(c, rule, b, m, every), f"{c.name} every {every} {rule}")
        assert rec["total"] == sc.total_ref(c, rule, b, m)


# ------------------------------------------------------------------------------ 6
def test_rank_slices_exact(native, scanner):
    """Seven rank slices without a communicator: each is its own cumsum from its begin."""
    c = ec.SLICE_CASE
    for r, (b, m) in enumerate(ec.rank_slices(c.at.n)):
        rule = ec.RULES[r % 3]
        for every in (1, 37):
            got, rec = _run(native, scanner(c.expr), c.at, rule, b, m, every)
            _expect(got, sc.running_ref(c, rule, b, m, every), f"rank {r} every {every}")
            assert rec["total"] == sc.total_ref(c, rule, b, m), r


# ------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("every", [1, 37])
@pytest.mark.parametrize("world", ec.LOOPBACK_WORLDS)
def test_loopback_ranks_exact(native, cuda, scanner, world, every):
    """W loopback ranks hold consecutive slices: their outputs, concatenated in rank order,
    are the one-rank output (and the reference), the total is the same double everywhere."""
    c = sc.QUADRATIC
    for rule in ec.RULES:
        def body(rank, comm):
            es = native.ExprScan(c.expr, cuda.index)
            b, m = ec.rank_slices(c.at.n, world)[rank]
            got, rec = _run(native, es, c.at, rule, b, m, every, 1.0, comm)
            _expect(got, sc.running_ref(c, rule, b, m, every, start=0), f"rank {rank}")
            return got, rec["total"]
        out = loopback.run_ranks(world, body)
        one, rec = _run(native, scanner(c.expr), c.at, rule, 0, c.at.n, every)
        _expect(np.concatenate([v for v, _ in out]), one, f"world {world} every {every} {rule}")
        _expect(one, sc.running_ref(c, rule, 0, c.at.n, every), "one rank")
        assert [t for _, t in out] == [rec["total"]] * world
        assert rec["total"] == sc.total_ref(c, rule, 0, c.at.n)


# ------------------------------------------------------------------------------ 8
def test_object_reuse_exact(native, cuda):
    """One ExprScan across 3, 700 000 and 5 samples: the workspace grows and is kept."""
    c = sc.FULL_LANES
    es = native.ExprScan(c.expr, cuda.index)
    for m in (3, 700_000, 5):
        got, rec = _run(native, es, c.at, "mid", sc.EDGE_BEGIN, m)
        _expect(got, sc.running_ref(c, "mid", sc.EDGE_BEGIN, m), f"reuse {m}")
        assert rec["total"] == sc.total_ref(c, "mid", sc.EDGE_BEGIN, m)


def test_objects_own_their_loaded_module(native, cuda):
    """8 tiles + 37 samples: A and B for one expression, A destroyed, a fresh C."""
    c = sc.QUADRATIC

    def check(es, what):
        got, rec = _run(native, es, c.at, "mid", 0, c.at.n)
        _expect(got, sc.running_ref(c, "mid", 0, c.at.n), what)
        assert rec["total"] == sc.total_ref(c, "mid", 0, c.at.n), what
    ec.check_module_lifetime(lambda: native.ExprScan(c.expr, cuda.index), check)


# ------------------------------------------------------------------------------ 9, 10
GAUSS = "exp(-x*x)"
GAUSS_N = 3 * 4096 + 5          # h = 3 / 12293 is not a power of two: x rounds


def test_sample_coordinates_are_the_integrators(native, cuda, scanner):
    """One sample at a time: F = h f(x_i), bitwise what ExprIntegrator gives the sample, so
    x has its bits (first and last sample of threads, waves, tiles and the rule)."""
    ei = native.ExprIntegrator(GAUSS, cuda.index)
    es = scanner(GAUSS)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for rule in ec.RULES:
        rl = getattr(native.Rule, rule)
        for begin in (0, 1, 15, 16, 1023, 1024, 4095, 4096, 8191, 12288, GAUSS_N - 1):
            rec = es.run(0.0, 3.0, GAUSS_N, rl, begin, 1, 1, out.data_ptr(), 1)
            want = ei.integrate(0.0, 3.0, GAUSS_N, rl, begin, 1)
            assert rec["total"] == want and float(out.item()) == want, (rule, begin)


def test_gauss_reproducible_and_within_rounding_bound(native, scanner):
    """exp(-x*x) on [0, 3], 3 tiles + 5: two runs are bitwise equal, and every F_i is within
    (2 * 2**-52 + D * 2**-53) * h * sum_{j <= i} |f_j| of math.fsum prefixes of numpy's values
    times h, at x_j = fma(j + off, h, 0) formed exactly (in rationals, rounded once).

    The first term is one ulp of the device's exp and one of numpy's per sample. D = 40 is
    the number of additions on the longest path from a sample to a written value, read off
    expr_scan.cpp for any slice of at most 2048 tiles (runs of R = 1 tile; a longer slice
    adds R - 1 for L[t]):
      tile sums      3 (an accumulator takes 4 samples) + 2 ((a0 + a1) + (a2 + a3))
                     + 6 (wave butterfly) + 2 (four wave partials)                    = 13
      run sums       0 (L[t] = 0 and A[b] = 0 + S with one tile per run)              =  0
      tile prefix    1 (a thread's two runs) + 6 (wave scan) + 15 (the lower waves'
                     totals in order, then + exc) + 1 (the thread's second run)       = 23
      write          1 (B + L) + 1 (C + P[t]) + 1 (+ (wb + exc)) + 1 (+ run_k)        =  4
    The path through the tile's own samples is shorter (15 serial + 6 wave scan + 3 wave
    bases + 2 = 26). With 4 tiles the prefix really adds twice, not 23 times; that slack is
    far more than the three roundings the formula does not name (the kernel's multiplication
    by h, fsum's own rounding and the reference's multiplication)."""
    D = 40
    es = scanner(GAUSS)
    h = 3.0 / GAUSS_N
    at = types.SimpleNamespace(a=0.0, b=3.0, n=GAUSS_N)
    for rule in ec.RULES:
        got, rec = _run(native, es, at, rule, 0, GAUSS_N)
        again, rec2 = _run(native, es, at, rule, 0, GAUSS_N)
        assert sc.same_bits(got, again) and rec["total"] == rec2["total"]
        off2 = ec.OFF2[rule]
        x = np.array([float(Fraction(2 * j + off2, 2) * Fraction(h)) for j in range(GAUSS_N)])
        f = np.exp(-x * x).tolist()
        # fsum of every prefix is quadratic; the exact sum in rationals, rounded once, is the
        # same number (checked at two prefixes)
        ref, bound = np.empty(GAUSS_N), np.empty(GAUSS_N)
        acc, mag = Fraction(0), Fraction(0)
        for j, fj in enumerate(f):
            acc += Fraction(fj)
            mag += Fraction(abs(fj))
            ref[j] = float(acc) * h
            bound[j] = (2 * 2.0 ** -52 + D * 2.0 ** -53) * h * float(mag)
        assert ref[100] == math.fsum(f[:101]) * h and ref[-1] == math.fsum(f) * h
        err = np.abs(got - ref)
        print(f"{rule}: largest |F_i - ref| / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), rule
        assert abs(rec["total"] - ref[-1]) <= bound[-1]


# ------------------------------------------------------------------------------ 11
@pytest.mark.parametrize("rule", ec.RULES)
def test_python_api_matches_cpu_backend(cuda, rule):
    from cuda_v_mpi_amd import integrate_expr_running

    c = sc.QUADRATIC
    for every in (1, 37):
        cpu = integrate_expr_running(c.expr, c.at.a, c.at.b, c.at.n, rule=rule, every=every,
                                     backend="cpu")
        hip = integrate_expr_running(c.expr, c.at.a, c.at.b, c.at.n, rule=rule, every=every)
        assert hip.values.is_cuda and hip.x.is_cuda and hip.device_ms > 0
        _expect(hip.values.cpu().numpy(), cpu.values.numpy(), f"running {rule} every {every}")
        _expect(hip.x.cpu().numpy(), cpu.x.numpy(), "x")
        assert hip.total == cpu.total
        v, total = kernels.riemann_expr_scan(c.expr, c.at.a, c.at.b, c.at.n, rule=rule,
                                             every=every)
        assert v.dtype == torch.float64 and v.dim() == 1 and total == cpu.total
        _expect(v.cpu().numpy(), cpu.values.numpy(), "kernels.riemann_expr_scan")
    # a slice into a caller's buffer
    buf = torch.zeros(100, dtype=torch.float64, device=cuda)
    v, total = kernels.riemann_expr_scan(c.expr, c.at.a, c.at.b, c.at.n, rule=rule, every=37,
                                         i_begin=36, n_local=1000, out=buf)
    assert v.data_ptr() == buf.data_ptr() and v.numel() == 28
    _expect(v.cpu().numpy(), sc.running_ref(c, rule, 36, 1000, 37), "out=")
    assert total == sc.total_ref(c, rule, 36, 1000)
    with pytest.raises(RuntimeError, match="output buffer holds 10 values"):
        kernels.riemann_expr_scan(c.expr, c.at.a, c.at.b, c.at.n, every=37, out=buf[:10])


# ------------------------------------------------------------------------------ 12
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_cli_running(cuda, tmp_path):
    c = sc.QUADRATIC
    base = ("--expr", c.expr, "--a", repr(c.at.a), "--b", repr(c.at.b), "--n", str(c.at.n),
            "--rule", "mid", "--running")
    h = 2.0 ** -c.at.k
    p = _riemann(*base, "--every", "37", "--json")
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    want = sc.running_ref(c, "mid", 0, c.at.n, 37)
    rows = [l.split() for l in lines[:-1]]
    assert len(rows) == len(want) == 886 and all(len(r) == 2 for r in rows)
    _expect([float(r[1]) for r in rows], want, "cli values")
    _expect([float(r[0]) for r in rows], [c.at.a + (j + 1) * (37 * h) for j in range(886)], "cli x")
    js = json.loads(lines[-1])
    assert js["total"] == sc.total_ref(c, "mid", 0, c.at.n) and js["outputs"] == 886
    assert js["every"] == 37 and js["device_ms"] > 0 and js["running"] is True
    # every value to a file, raw little-endian fp64
    path = tmp_path / "running.f64"
    p = _riemann(*base, "--running-out", str(path), "--json")
    assert p.returncode == 0, p.stderr
    _expect(np.fromfile(path, dtype="<f8"), sc.running_ref(c, "mid", 0, c.at.n), "cli file")
    assert json.loads(p.stdout.strip().splitlines()[-1])["outputs"] == c.at.n
    # more than 10 000 lines are refused, naming the two ways out
    p = _riemann(*base)
    assert p.returncode == 1 and "--every" in p.stderr and "--running-out" in p.stderr
