"""CPU tests of the lattice rule (ExprLattice, csrc/runtime/expr_lattice.cpp): the numpy model
(cuda_v_mpi_amd/utils/lattice_rule.py) against brute force in rationals, the built-in table of
Korobov multipliers against the search that chose it, the truth cases on the model, the exact
cases' budgets, the compile, every refusal and every CLI conflict. No device needed."""
from __future__ import annotations

import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_lattice_cases as lc
from cuda_v_mpi_amd import LatticeResult, integrate_expr_nd, native
from cuda_v_mpi_amd.utils import lattice_rule as lr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the model, brute force
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("m,d", [(2, 1), (4, 2), (6, 3)])
def test_points_against_rationals(m, d, periodic):
    """Every coordinate of every point of two shifts, from the definitions in Fractions."""
    n = 1 << m
    z = lc.z_for(m, d)
    words = lc.words_for(2, d)
    box = [(-1.0, 1.0), (0.25, 0.75), (2.0, -2.0)][:d]
    for row in words:
        u = lr.fractions_u32(m, z, row)
        t = lr.unit_coords(u, periodic)
        x = lr.coords(t, box)
        numer = lr.numerators(u, periodic)
        for i in range(n):
            for j in range(d):
                uu = ((((i * z[j]) % n) << (32 - m)) + int(row[j])) % (1 << 32)
                assert int(u[i, j]) == uu
                tau = Fraction(2 * uu + 1, 1 << 33)          # the centred fraction (u + 1/2) / 2^32
                want = tau if periodic else 1 - abs(2 * tau - 1)
                assert Fraction(int(numer[i, j]), lr.denominator(periodic)) == want
                assert Fraction(float(t[i, j])) == want and 0 < want < 1
                lo, hi = box[j]
                assert Fraction(float(x[i, j])) == Fraction(lo) + (Fraction(hi) - Fraction(lo)) * want


def test_tent_identity_over_the_top_16_bits():
    """t = 1 - |2 tau - 1| exactly, over all 2^16 values of the top 16 bits of u (the low 16
    bits all 0, all 1 and one pattern between)."""
    top = np.arange(1 << 16, dtype=np.uint64) << np.uint64(16)
    for low in (0, 0xFFFF, 0x5A5A):
        u = (top | np.uint64(low)).astype(np.uint32)
        numer = lr.numerators(u, False).astype(np.int64)          # over 2^32
        tau2 = 2 * u.astype(np.int64) + 1                         # 2 tau - 1 = (tau2 - 2^32) / 2^32
        assert np.array_equal(numer, (1 << 32) - np.abs(tau2 - (1 << 32)))
        t = lr.unit_coords(u, False)
        assert np.array_equal(t * 2.0 ** 32, numer.astype(np.float64))
        assert t.min() > 0.0 and t.max() < 1.0


def test_shifts_are_splitmix64():
    m = native()
    mask = (1 << 64) - 1
    for seed, rows, d in ((0, 3, 16), (12345678901234567890, 5, 3), (7, 1, 1)):
        got = m.lattice_shifts(seed, rows, d)
        assert got.shape == (rows, d) and got.dtype == np.uint32
        assert np.array_equal(got, lr.lattice_shifts(seed, rows, d))
        for r in range(rows):
            for j in range(d):
                q = r * 16 + j
                zz = (seed + (q + 1) * 0x9E3779B97F4A7C15) & mask
                zz = ((zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9) & mask
                zz = ((zz ^ (zz >> 27)) * 0x94D049BB133111EB) & mask
                zz ^= zz >> 31
                assert int(got[r, j]) == zz >> 32


def test_estimates_value_and_error_in_the_stated_order():
    out = lr.finish([1.0, 2.0, 4.0], 0.5, 4)
    est = [0.5 * 1.0 / 4, 0.5 * 2.0 / 4, 0.5 * 4.0 / 4]
    value = ((est[0] + est[1]) + est[2]) / 3
    q = ((est[0] - value) ** 2 + (est[1] - value) ** 2) + (est[2] - value) ** 2
    assert out["estimates"].tolist() == est and out["value"] == value
    assert out["err_est"] == math.sqrt(q / 6.0)
    assert lr.finish([3.0], 1.0, 1)["err_est"] == math.inf


# ------------------------------------------------------------------ 2. the table
BUILTIN = range(native().LATTICE_BUILTIN_M_MIN, native().LATTICE_BUILTIN_M_MAX + 1)


def test_table_covers_10_to_24_and_is_admissible():
    m = native()
    assert m.LATTICE_BUILTIN_M_MIN == 10 and m.LATTICE_BUILTIN_M_MAX >= 24
    for lm in BUILTIN:
        a = m.lattice_multiplier(lm)
        assert a % 8 in (3, 5) and a < 1 << lm
        z = m.lattice_generator(lm, 16)
        assert z == lr.korobov(a, lm, 16) and z[0] == 1
        assert len(set(z)) == 16 and all(v % 2 == 1 and v < 1 << lm for v in z)
        assert m.lattice_generator(lm, 5) == z[:5]


def test_search_returns_the_committed_multipliers():
    """tools/lattice_search.py, run again for m = 10 ... 14 (one process)."""
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "lattice_search.py"), "--m",
                        "10", "14", "--json"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    recs = [json.loads(line) for line in p.stdout.splitlines()]
    assert [rec["m"] for rec in recs] == [10, 11, 12, 13, 14]
    for rec in recs:
        assert rec["a"] == native().lattice_multiplier(rec["m"])
        assert rec["e2"] == lr.criterion(rec["a"], rec["m"])
        assert rec["candidates"] == 64 and rec["seed"] == 2024


@pytest.mark.parametrize("m", [10, 12, 14, 16])
def test_committed_multiplier_beats_the_poor_ones(m):
    """a = 3 and a = 5 are admissible and known to be poor: a sanity check, not a measurement."""
    e2 = lr.criterion(native().lattice_multiplier(m), m)
    assert 0 < e2 <= lr.criterion(3, m) and e2 <= lr.criterion(5, m)


def test_criterion_against_the_plain_sum():
    """The halved sum (points i and n - i share a product) against all n points in Fractions of
    the B2 arguments."""
    m, a = 6, 27
    n = 1 << m
    z = lr.korobov(a, m, 16)
    total = 0.0
    for i in range(n):
        prod = 1.0
        for j in range(16):
            t = ((i * z[j]) % n) / n
            prod *= 1.0 + (2.0 * math.pi ** 2 / (j + 1) ** 2) * (t * t - t + 1.0 / 6.0)
        total += prod
    assert lr.criterion(a, m) == pytest.approx(total / n - 1.0, rel=1e-12)


# ------------------------------------------------------------------ 3. the truth cases
@pytest.mark.parametrize("m", lc.TRUTH_LEVELS)
@pytest.mark.parametrize("case", lc.TRUTHS, ids=repr)
def test_model_stays_within_three_standard_errors(case, m):
    r = lc.truth_model(case, m)
    truth = case.truth()
    print(case, m, "value", r["value"], "truth", truth, "err_est", r["err_est"], "in se",
          abs(r["value"] - truth) / r["err_est"])
    assert r["estimates"].shape == (lc.TRUTH_SHIFTS,) and r["evals"] == 16 << m
    assert 0 < r["err_est"] < math.inf
    assert abs(r["value"] - truth) <= 3 * r["err_est"]


def test_truth_cases_cover_the_dimensions():
    assert sorted(c.d for c in lc.TRUTHS) == [3, 4, 6, 8, 16]


def test_model_converges_with_the_level():
    """Four more levels cut the standard error of the smooth cases by more than 4 (plain Monte
    Carlo's factor for 16 times the points)."""
    for case in (lc.GAUSS6, lc.COS8, lc.EXP16, lc.PROD4):
        assert lc.truth_model(case, 16)["err_est"] < lc.truth_model(case, 12)["err_est"] / 4


# ------------------------------------------------------------------ 4. the exact cases
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("case", lc.EXACTS, ids=repr)
def test_exact_budgets(case, periodic):
    """The largest numerator times the point count stays below 2^53: at m = 10 for the whole
    rule (the largest exact level on the device), at m = 12 and m = 30 for the slices used."""
    assert lc.budget(case, periodic, 1 << 10) < 1 << 53
    if case.d <= 3:
        assert lc.budget(case, periodic, 1 << 12) < 1 << 53


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("case", lc.EXACTS, ids=repr)
def test_integer_reference_equals_the_model(case, periodic):
    """The model's fp64 sums of an exact case are the integer reference's, bit for bit, and so
    are the rationals behind them at m = 4."""
    m = 4 if case.d == 16 else 6
    z = lc.z_for(m, case.d)
    words = lc.words_for(3, case.d)
    f = {"abs1": lambda x: np.abs(x[:, 0] - 0.25),
         "absdiff": lambda x: np.abs(x[:, 0] - x[:, 1]),
         "max3": lambda x: x.max(axis=1),
         "simplex": lambda x: (x[:, 0] + x[:, 1] + x[:, 2] < 1.5).astype(np.float64),
         "linear16": lambda x: (x * np.arange(1.0, 17.0)).sum(axis=1)}[case.name]
    got = lr.lattice_model(f, case.box, m, z=z, shift_words=words, periodic=periodic)
    want = lc.exact_reference(case, m, z, words, periodic)
    assert got["sums"].tolist() == want["sums"]
    assert got["estimates"].tolist() == want["estimates"].tolist()
    assert got["value"] == want["value"] and got["err_est"] == want["err_est"]
    numer = lr.exact_points(m, z, words, case.box, periodic)
    assert numer.shape == (3, 1 << m, case.d)
    big_d = lr.denominator(periodic)
    for r in range(3):
        total = Fraction(0)
        for i in range(1 << m):
            x = [Fraction(lo) + (Fraction(hi) - Fraction(lo)) * Fraction(int(numer[r, i, j]), big_d)
                 for j, (lo, hi) in enumerate(case.box)]
            total += {"abs1": lambda: abs(x[0] - Fraction(1, 4)),
                      "absdiff": lambda: abs(x[0] - x[1]),
                      "max3": lambda: max(x),
                      "simplex": lambda: Fraction(int(x[0] + x[1] + x[2] < Fraction(3, 2))),
                      "linear16": lambda: sum((j + 1) * v for j, v in enumerate(x))}[case.name]()
        assert Fraction(want["sums"][r]) == total


# ------------------------------------------------------------------ 5. the compile
@pytest.mark.parametrize("periodic", [False, True])
def test_compiles_for_gfx950_at_d_1_and_16(periodic):
    m = native()
    for case in (lc.ABS1, lc.LINEAR16):
        src = m.expr_lattice_source(case.expr, case.d, periodic)
        for name in ("miint_lattice_partials", "miint_lattice_close", "miint_lattice_finish"):
            assert name in src
        assert ("0x1p-33" in src) == periodic and ("0x7FFFFFFFu" in src) != periodic
        code = m.expr_lattice_compile(case.expr, case.d, periodic)
        assert code[:4] == b"\x7fELF" and len(code) > 4096


def test_a_variable_past_the_box_fails_in_the_compiler():
    m = native()
    with pytest.raises(RuntimeError, match="x3"):
        m.expr_lattice_compile("x0+x3", 3)
    with pytest.raises(RuntimeError, match="not allowed"):
        m.expr_lattice_source("x0; x1", 2)


def test_launch_shape_never_depends_on_the_shifts():
    m = native()
    assert m.lattice_shape(1 << 16, 1) == (1, 1) and m.lattice_shape(1 << 16, 17) == (1, 17)
    assert m.lattice_shape(1 << 24, 64) == (256, 8) and m.lattice_shape(1 << 24, 1) == (256, 1)
    assert m.lattice_shape(1 << 30, 4096) == (2048, 1)
    assert m.lattice_shape(1000, 5, 3) == (3, 5) and m.lattice_shape(0, 2) == (1, 2)


# ------------------------------------------------------------------ 6. every refusal
BOX2 = [(0.0, 1.0), (0.0, 1.0)]


def _opt(**kw):
    return native().LatticeOptions(**kw)


@pytest.mark.parametrize("box,m,opts,begin,count,scale,message", [
    ([], 12, {}, 0, 1, 1.0, "d = 0 must be 1..16"),
    ([(0.0, 1.0)] * 17, 12, {}, 0, 1, 1.0, "d = 17 must be 1..16"),
    (BOX2, 1, {"z": [1, 1]}, 0, 1, 1.0, "m = 1 must be 2..30"),
    (BOX2, 31, {"z": [1, 1]}, 0, 1, 1.0, "m = 31 must be 2..30"),
    ([(0.0, math.inf), (0.0, 1.0)], 12, {}, 0, 1, 1.0, "side 0 of the box"),
    ([(0.0, 1.0), (math.nan, 1.0)], 12, {}, 0, 1, 1.0, "side 1 of the box"),
    ([(-1e308, 1e308), (0.0, 1.0)], 12, {}, 0, 1, 1.0, "side 0 of the box"),
    (BOX2, 12, {}, 0, 1, math.inf, "scale = inf must be finite"),
    (BOX2, 12, {"shifts": 0}, 0, 1, 1.0, "shifts = 0 must be 1..4096"),
    (BOX2, 12, {"shifts": 4097}, 0, 1, 1.0, "shifts = 4097 must be 1..4096"),
    (BOX2, 12, {"shift_words": [1, 2, 3]}, 0, 1, 1.0, "3 shift words are not 1..4096 rows of d = 2"),
    (BOX2, 12, {"z": [1, 2]}, 0, 1, 1.0, r"z\[1\] = 2 must be odd and below n = 4096"),
    (BOX2, 12, {"z": [4097, 1]}, 0, 1, 1.0, r"z\[0\] = 4097 must be odd and below n = 4096"),
    (BOX2, 12, {"z": [1, 3, 5]}, 0, 1, 1.0, "3 generating entries for d = 2"),
    (BOX2, 9, {}, 0, 1, 1.0, "no built-in generating vector for m = 9"),
    (BOX2, 27, {}, 0, 1, 1.0, "no built-in generating vector for m = 27"),
    (BOX2, 12, {}, 4096, 1, 1.0, r"slice \[4096, 4096 \+ 1\) outside \[0, 4096\)"),
    (BOX2, 12, {}, 1, 2 ** 64 - 1, 1.0, "outside"),
])
def test_refusals_name_the_numbers(box, m, opts, begin, count, scale, message):
    with pytest.raises(RuntimeError, match=message):
        native().lattice_check(box, m, _opt(**opts), begin, count, scale)


@pytest.mark.parametrize("opts,message", [
    ({}, "rtol = 0.000000 and atol = 0.000000 must be finite and >= 0, and not both 0"),
    ({"rtol": -1.0}, "must be finite and >= 0"),
    ({"rtol": math.nan}, "must be finite and >= 0"),
    ({"rtol": 1e-6, "m_min": 9}, "m_min = 9 must lie in 10..m_max"),
    ({"rtol": 1e-6, "m_min": 15, "m_max": 14}, "m_min = 15 must lie in 10..m_max = 14"),
    ({"rtol": 1e-6, "z": [1, 3]}, "takes the built-in vectors"),
    ({"rtol": 1e-6, "shifts": 0}, "shifts = 0"),
])
def test_walk_refusals_name_the_numbers(opts, message):
    with pytest.raises(RuntimeError, match=message):
        native().lattice_check_walk(BOX2, _opt(**opts))


def test_accepted_calls_and_defaults():
    m = native()
    o = m.LatticeOptions()
    assert (o.shifts, o.seed, o.m_min, o.m_max, o.rtol, o.atol) == (16, 0, 12, 0, 0.0, 0.0)
    assert list(o.z) == [] and list(o.shift_words) == []
    m.lattice_check(BOX2, 12, o, 0, 4096)
    m.lattice_check(BOX2, 2, _opt(z=[1, 3]), 3, 1)
    m.lattice_check([(1.0, 0.0), (2.0, 2.0)], 30, _opt(z=[1, (1 << 30) - 1], shifts=4096), 0, 1 << 30)
    m.lattice_check_walk(BOX2, _opt(atol=1e-3, m_max=99))       # clamped to the table's last m
    assert (m.LATTICE_MAX_DIM, m.LATTICE_MIN_M, m.LATTICE_MAX_M, m.LATTICE_MAX_SHIFTS) == \
        (16, 2, 30, 4096)


def test_python_refusals_come_before_any_device_call():
    from cuda_v_mpi_amd.ops import kernels

    with pytest.raises(RuntimeError, match="m = 1 must be 2..30"):
        kernels.lattice_expr("x0", [(0, 1)], m=1)
    with pytest.raises(RuntimeError, match="not both 0"):
        kernels.lattice_expr("x0", [(0, 1)], rtol=0.0)
    with pytest.raises(ValueError, match="not both and not neither"):
        integrate_expr_nd("x0", [(0, 1)])
    with pytest.raises(ValueError, match="not both and not neither"):
        integrate_expr_nd("x0", [(0, 1)], m=12, rtol=1e-3)
    with pytest.raises(ValueError, match="backend"):
        integrate_expr_nd("x0", [(0, 1)], m=12, backend="host")
    with pytest.raises(ValueError, match=r"z\[0\] = 2"):
        integrate_expr_nd("x0", [(0, 1)], m=12, z=[2], backend="cpu")


# ------------------------------------------------------------------ 7. the cpu backend
def test_cpu_backend_runs_the_model_on_expr_torch():
    case = lc.GAUSS6
    want = lc.truth_model(case, 12)
    r = integrate_expr_nd(case.expr, case.box, m=12, seed=case.seed, backend="cpu")
    assert isinstance(r, LatticeResult) and r.backend == "cpu" and not r.converged
    assert (r.m, r.n, r.shifts, r.evals, r.levels) == (12, 4096, 16, 16 * 4096, 1)
    assert r.value == pytest.approx(want["value"], rel=1e-13)
    assert r.err_est == pytest.approx(want["err_est"], rel=1e-6)
    assert json.loads(json.dumps(r.as_dict()))["estimates"] == r.estimates


def test_cpu_backend_walks_to_a_tolerance():
    case = lc.GAUSS6
    r = integrate_expr_nd(case.expr, case.box, rtol=1e-6, seed=case.seed, backend="cpu")
    assert r.converged and r.err_est <= 1e-6 * abs(r.value)
    assert r.levels == r.m - 12 + 1 and r.evals == sum(16 << k for k in range(12, r.m + 1))
    assert abs(r.value - case.truth()) <= 4 * r.err_est
    r = integrate_expr_nd("x0*x1", [(0, 1), (0, 1)], rtol=1e-30, m_min=10, m_max=11, backend="cpu")
    assert not r.converged and (r.m, r.levels) == (11, 2) and math.isfinite(r.value)


def test_model_reversed_and_empty_sides():
    f = lc.PROD4.f
    fwd = lr.lattice_model(f, [(0.0, 2.0)] * 4, 10, shifts=2)
    rev = lr.lattice_model(f, [(2.0, 0.0)] + [(0.0, 2.0)] * 3, 10, shifts=2)
    assert rev["vol_scale"] == -fwd["vol_scale"] and rev["value"] == pytest.approx(-16.0, rel=1e-3)
    flat = lr.lattice_model(f, [(1.0, 1.0)] + [(0.0, 2.0)] * 3, 10, shifts=2)
    assert flat["value"] == 0.0 and flat["err_est"] == 0.0


# ------------------------------------------------------------------ 8. the command lines
def _riemann(*args, env=None):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def _python_cli(*args):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=120)


BASE = ("--expr", "x0*x1", "--box", "0:1,0:1")
CONFLICTS = [(("--a", "0"), "--a"), (("--b", "1"), "--b"), (("--n", "100"), "--n"),
             (("--rule", "mid"), "--rule"), (("--running",), "--running"),
             (("--ya", "0", "--yb", "1"), "--ya"), (("--params", "rows.txt"), "--params"),
             (("--linspace", "p0=0:1:3"), "--linspace"), (("--panels", "64"), "--panels"),
             (("--max-depth", "3"), "--max-depth"), (("--max-intervals", "64"), "--max-intervals"),
             (("--device", "cpu"), "--device cpu")]


@pytest.mark.parametrize("extra,named", CONFLICTS, ids=[c[1] for c in CONFLICTS])
def test_native_cli_names_the_conflict(extra, named):
    for mode in (("--m", "12"), ("--rtol", "1e-6")):
        p = _riemann(*BASE, *mode, *extra)
        assert p.returncode == 1 and named in p.stderr and p.stdout == "", (p.stdout, p.stderr)


@pytest.mark.parametrize("flag", [("--m", "12"), ("--shifts", "4"), ("--seed", "3"),
                                  ("--z", "1,3"), ("--periodic",), ("--m-max", "14")])
def test_native_cli_lattice_flags_belong_to_box(flag):
    p = _riemann("--expr", "x", "--a", "0", "--b", "1", "--n", "1e4", *flag)
    assert p.returncode == 1 and flag[0] + " belongs to --box" in p.stderr
    p = _riemann(*flag)
    assert p.returncode == 1 and "belongs to --box" in p.stderr


def test_native_cli_refuses_bad_numbers_before_any_device_call():
    for args, named in (
            ((*BASE,), "--m M"), ((*BASE, "--m", "12", "--rtol", "1e-6"), "one of the two"),
            ((*BASE, "--m", "12", "--m-max", "14"), "--m-max belongs"),
            ((*BASE, "--rtol", "1e-6", "--z", "1,3"), "--z is the generating vector of one --m"),
            ((*BASE, "--m", "1.5"), "--m must be a whole number"),
            ((*BASE, "--m", "31", "--z", "1,3"), "m = 31 must be 2..30"),
            ((*BASE, "--m", "9"), "no built-in generating vector for m = 9"),
            ((*BASE, "--m", "12", "--z", "1,2"), "z[1] = 2 must be odd"),
            ((*BASE, "--m", "12", "--z", "1,x"), "--z wants odd whole numbers"),
            ((*BASE, "--m", "12", "--shifts", "0"), "shifts = 0"),
            ((*BASE, "--m", "12", "--shifts", "5000"), "shifts = 5000"),
            ((*BASE, "--rtol", "0"), "not both 0"),
            ((*BASE, "--rtol", "abc"), "--rtol must be a number"),
            (("--expr", "x0", "--box", "0:1,0", "--m", "12"), "--box wants"),
            (("--expr", "x0", "--box", "0:inf", "--m", "12"), "side 0 of the box"),
            (("--expr", "x0", "--box", ",".join(["0:1"] * 17), "--m", "12"), "d = 17"),
            (("--expr", "x0+x1", "--box", "0:1", "--m", "12"), "x1"),
            (("--box", "0:1", "--m", "12"), "--box is the box of an --expr integrand")):
        p = _riemann(*args)
        assert p.returncode == 1 and named in p.stderr and p.stdout == "", (args, p.stderr)


def test_native_cli_help_names_the_lattice_path():
    p = _riemann("--help")
    assert p.returncode == 0
    for word in ("--box A0:B0,A1:B1,...", "--m M", "--shifts R", "--seed S", "--periodic",
                 "--z Z0,Z1,...", "--m-max", "lattice", "err_est"):
        assert word in p.stdout, word


def _python_cli_refusal(*args) -> str:
    """The message `python -m cuda_v_mpi_amd integrate ARGS` exits with (in this process)."""
    from cuda_v_mpi_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["integrate", *args])
    assert e.value.code not in (0, None)
    return str(e.value.code)


def test_python_cli_names_the_conflict():
    for extra, named in ((("--a", "0"), "--a"), (("--n", "100"), "--n"), (("--rule", "mid"), "--rule"),
                         (("--ya", "0"), "--ya"), (("--params", "rows.txt"), "--params"),
                         (("--linspace", "p0=0:1:3"), "--linspace"), (("--panels", "4"), "--panels"),
                         (("--max-depth", "3"), "--max-depth"),
                         (("--max-intervals", "9"), "--max-intervals"),
                         (("--device", "cpu"), "--device cpu")):
        msg = _python_cli_refusal(*BASE, "--m", "12", *extra)
        assert named in msg and "does not go with it" in msg
    for flag in (("--m", "12"), ("--shifts", "4"), ("--seed", "3"), ("--z", "1,3"), ("--periodic",),
                 ("--m-max", "14")):
        assert flag[0] + " belongs to --box" in _python_cli_refusal("--expr", "x", "--a", "0",
                                                                    "--b", "1", *flag)
    assert "one of the two" in _python_cli_refusal(*BASE)
    assert "--box is the box of an --expr integrand" in _python_cli_refusal("--box", "0:1", "--m",
                                                                            "12")
    p = _python_cli(*BASE, "--m", "12", "--n", "5")          # and as a process: status and stderr
    assert p.returncode != 0 and "--n does not go with it" in p.stderr and p.stdout == ""


def test_python_cli_runs_the_model():
    p = _python_cli("--expr", "x0*x1*x2*x3", "--box", "0:2,0:2,0:2,0:2", "--m", "12", "--backend",
                    "cpu", "--analytic", "16")
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.splitlines()[-1])
    want = lc.truth_model(lc.PROD4, 12)
    assert rec["value"] == pytest.approx(want["value"], rel=1e-13) and rec["shifts"] == 16
    assert rec["abs_err"] == abs(rec["value"] - 16.0) and len(rec["estimates"]) == 16
