"""GPU tests of the lattice rule (ExprLattice, csrc/runtime/expr_lattice.cpp): the device against
an integer reference bit for bit on integrands whose samples sum exactly, against the numpy
model of the same rule (cuda_v_mpi_amd/utils/lattice_rule.py; its own checks are in
test_expr_lattice_cpu.py) to a rounding bound on smooth ones, and against closed forms.

The rounding bound of a smooth estimate. est_r = (c / n) S_r with c = vol * scale and S_r the
sum of the n samples. The device and the model form the same points (every t is exact, and
x_j = fma(t, w_j, a_j) is one rounding in both) and differ in two places. With u = 2^-53 and
A_r the sum of |f| over shift r's points (the model reports it):
  * f itself. The expressions here combine the d coordinates in at most 2 d operations before
    and a few after one library call (exp, cos: 2 u on the device, 1 u in numpy); the compiler
    may contract a multiply-add on the device, which moves each of them by at most u. For
    exp(-sum (x_j - 1/2)^2), exp(sum x_j / 16) and the product the argument's error enters f
    relatively, times an argument of at most 1.5: at most (4 d + 8) u |f| per sample. For
    cos(sum x_j) the argument's absolute error of 4 d u enters f absolutely while the mean of |f|
    is 0.3 or more: the case's K = 4 multiplies the 4 d. The indicator takes no rounding unless a
    point lies within 4 u of the sphere, which none of the 2^20 points here does.
  * the order of the sum. The device: a lane adds count / (256 gx) samples into four chains, so
    at most n / 1024 additions deep at gx = 1, then 2 to join the chains, 6 butterfly steps, 2 for
    the four waves, and in the closing workgroup a run of at most ceil(gx / 256) = 1 partial and
    8 more: n / 1024 + 19. The model: numpy's pairwise sum of at most 2^16 samples, blocks of 128
    in 8 chains and 9 levels above them, at most 16 + 3 + 9 = 28, and fsum of the chunks. Each
    addition rounds by at most u times the sum of |f| it has seen: (n / 1024 + 47) u A_r; the
    tests use n / 1024 + 64.
So |est_r - model_r| <= (|c| / n) u A_r (4 d K + 8 + n / 1024 + 64) + 2 u |est_r|, the last
term for the two roundings of the scaling. `value` is held to 4 err_est plus the largest such
bound of its shifts: three standard errors are the CPU test's, the fourth is the margin for the
summation order alone."""
from __future__ import annotations

import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_lattice_cases as lc
from cuda_v_mpi_amd import integrate_expr_nd
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.parallel import loopback
from cuda_v_mpi_amd.utils import lattice_rule as lr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _bits(v) -> list:
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def _within_ulps(got: float, want: float, ulps: int = 4) -> bool:
    if got == want:
        return True
    return abs(got - want) <= ulps * math.ulp(max(abs(got), abs(want)))


def _check_exact(r, want):
    print("value", r.value, want["value"], "err_est", r.err_est, want["err_est"])
    assert _bits(r.estimates) == _bits(want["estimates"])
    assert _within_ulps(r.value, want["value"]) and _within_ulps(r.err_est, want["err_est"])


# ------------------------------------------------------------------ 1. exact, bit for bit
# (case, m, shifts, periodic, grid, begin, count, scale)
EXACT_RUNS = [
    (lc.ABS1, 4, 1, False, 0, 0, None, 1.0),
    (lc.ABS1, 8, 2, True, 3, 0, None, 1.0),
    (lc.ABS1, 10, 5, False, 1, 0, None, 1.0),
    (lc.ABSDIFF, 10, 5, False, 0, 0, None, 1.0),
    (lc.ABSDIFF, 10, 17, True, 3, 0, None, 1.0),
    (lc.ABSDIFF, 4, 2, True, 0, 0, None, 1.0),
    (lc.MAX3, 8, 5, False, 1, 1, 200, 1.0),          # fewer points than lanes, an odd begin
    (lc.MAX3, 12, 2, True, 1, 3, 4089, 1.0),         # 15 or 16 per lane: both loops, ends in a run
    (lc.MAX3, 8, 1, False, 0, 77, 1, 3.0),           # a count of 1, a scale
    (lc.SIMPLEX, 10, 17, False, 3, 1, 700, 1.0),     # ends inside a wave of the third workgroup
    (lc.SIMPLEX, 10, 5, True, 0, 1023, 1, 1.0),      # the last point alone
    (lc.SIMPLEX, 8, 2, False, 3, 0, None, 1.0),
    (lc.LINEAR16, 4, 2, False, 0, 0, None, 1.0),
    (lc.LINEAR16, 10, 17, True, 3, 0, None, 1.0),
    (lc.LINEAR16, 10, 5, False, 0, 0, None, -0.375),
    (lc.LINEAR16, 8, 1, True, 1, 5, 250, 1.0),
]
LARGEST_PARTIALS = max(run[2] * max(run[4], 1) for run in EXACT_RUNS)   # R x gx: 17 x 3


@pytest.mark.parametrize("run", EXACT_RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_exact_against_the_integer_reference(cuda, run):
    case, m, rows, periodic, grid, begin, count, scale = run
    z, words = lc.z_for(m, case.d), lc.words_for(rows, case.d)
    points = (1 << m) - begin if count is None else count
    assert lc.budget(case, periodic, points) < 1 << 53
    r, est = kernels.lattice_expr(case.expr, case.box, m=m, periodic=periodic, z=z,
                                  shift_words=words, begin=begin, count=count, scale=scale,
                                  grid=grid)
    want = lc.exact_reference(case, m, z, words, periodic, begin, count, scale)
    _check_exact(r, want)
    assert (r.m, r.n, r.shifts, r.evals, r.levels) == (m, 1 << m, rows, rows * points, 1)
    assert est.dtype == torch.float64 and _bits(est.numpy()) == _bits(r.estimates)


@pytest.mark.parametrize("which", ["last_4096", "odd_tail", "product_passes_2_32"])
def test_exact_slices_at_m_30(cuda, which):
    """i z_j reaches 2^59 here: a start product taken in 32 bits, or in fp64 below its 53 bits,
    misses the reference."""
    m, n = 30, 1 << 30
    if which == "last_4096":
        case, periodic, z, begin, count = lc.MAX3, False, lc.z_for(m, 3), n - 4096, 4096
    elif which == "odd_tail":
        case, periodic, z, begin, count = lc.ABSDIFF, True, [n - 1, n - 3], n - 4095, 4095
    else:   # z_0 = 1048583: i z_0 first passes 2^32 at i = 4096
        case, periodic, z, begin, count = lc.MAX3, True, [1048583, 3, n - 1], 4000, 4096
        assert (begin + 95) * z[0] < 1 << 32 <= (begin + 96) * z[0]
    words = lc.words_for(2, case.d)
    assert lc.budget(case, periodic, count) < 1 << 53
    r, _ = kernels.lattice_expr(case.expr, case.box, m=m, periodic=periodic, z=z,
                                shift_words=words, begin=begin, count=count)
    _check_exact(r, lc.exact_reference(case, m, z, words, periodic, begin, count))


@pytest.mark.parametrize("world,m", [(2, 8), (3, 4), (8, 2)])
def test_exact_over_loopback_ranks(native, cuda, world, m):
    """The ranks split the points and all-reduce the shifts' sums; with 8 ranks and 4 points
    four ranks are idle. Every rank holds the whole rule's result."""
    case, periodic = lc.ABSDIFF, world == 3
    z, words = lc.z_for(m, case.d), lc.words_for(5, case.d)
    opt = native.LatticeOptions(z=z, shift_words=[int(w) for w in words.ravel()])
    slices = lc.rank_slices(1 << m, world)
    assert (world == 8) == any(c == 0 for _, c in slices)

    def body(rank, comm):
        el = native.ExprLattice(case.expr, case.d, periodic, cuda.index)
        b, c = slices[rank]
        return el.integrate(list(case.box), m, opt, b, c, 1.0, comm)
    want = lc.exact_reference(case, m, z, words, periodic)
    for r in loopback.run_ranks(world, body):
        _check_exact(r, want)


def test_reversed_and_empty_sides(cuda):
    case = lc.MAX3                                            # its second side runs from 2 to -2
    z, words = lc.z_for(8, 3), lc.words_for(2, 3)
    r, _ = kernels.lattice_expr(case.expr, case.box, m=8, z=z, shift_words=words)
    flipped = (case.box[0], (-2.0, 2.0), case.box[2])
    f, _ = kernels.lattice_expr(case.expr, flipped, m=8, z=z, shift_words=words)
    assert r.value < 0 < f.value                              # the volume changes sign
    e, _ = kernels.lattice_expr(case.expr, (case.box[0], (2.0, 2.0), case.box[2]), m=8, z=z,
                                shift_words=words)
    assert e.value == 0.0 and e.err_est == 0.0 and e.estimates.tolist() == [0.0, 0.0]
    assert e.device_ms == 0.0 and e.evals == 0                # nothing was launched


# ------------------------------------------------------------------ 2. shift independence
def test_a_shifts_estimate_never_depends_on_its_company(cuda):
    """gx depends on the points only: shift r's estimate is bitwise the same alone and among 17,
    for a smooth integrand whose sum does depend on the order."""
    case = lc.GAUSS6
    words = lr.lattice_shifts(99, 17, case.d)
    all17, _ = kernels.lattice_expr(case.expr, case.box, m=10, shift_words=words)
    again, _ = kernels.lattice_expr(case.expr, case.box, m=10, shift_words=words)
    assert _bits(all17.estimates) == _bits(again.estimates)
    assert _bits([all17.value, all17.err_est]) == _bits([again.value, again.err_est])
    for r in (0, 1, 7, 16):
        one, _ = kernels.lattice_expr(case.expr, case.box, m=10, shift_words=words[r])
        assert one.shifts == 1 and one.err_est == math.inf
        assert _bits(one.estimates) == _bits(all17.estimates[r:r + 1])
        assert _bits([one.value]) == _bits(all17.estimates[r:r + 1])
    swapped, _ = kernels.lattice_expr(case.expr, case.box, m=10, shift_words=words[::-1].copy())
    assert _bits(swapped.estimates) == _bits(all17.estimates[::-1])
    assert len(set(_bits(all17.estimates))) == 17


# ------------------------------------------------------------------ 3. smooth cases
def rounding_bound(case, model, r: int) -> float:
    """The bound of the module docstring for shift r's estimate."""
    n, d = model["n"], case.d
    per_sample = 4 * d * case.cond + 8 + n / 1024 + 64
    return (abs(model["vol_scale"]) / n * U * model["abs_sums"][r] * per_sample
            + 2 * U * abs(model["estimates"][r]))


@pytest.mark.parametrize("m", lc.TRUTH_LEVELS)
@pytest.mark.parametrize("case", lc.TRUTHS, ids=repr)
def test_smooth_against_the_model_and_the_truth(cuda, case, m):
    model = lc.truth_model(case, m)
    r, _ = kernels.lattice_expr(case.expr, case.box, m=m, shifts=lc.TRUTH_SHIFTS, seed=case.seed)
    bounds = [rounding_bound(case, model, k) for k in range(lc.TRUTH_SHIFTS)]
    diffs = np.abs(r.estimates - model["estimates"])
    truth = case.truth()
    print(case, m, "value", r.value, "truth", truth, "err_est", r.err_est, "in se",
          abs(r.value - truth) / r.err_est, "worst est diff / bound",
          float((diffs / np.array(bounds)).max()), "bound", max(bounds))
    assert np.all(diffs <= np.array(bounds))
    assert r.err_est == pytest.approx(model["err_est"], rel=1e-6)
    assert abs(r.value - truth) <= 4 * r.err_est + max(bounds)
    assert (r.m, r.shifts, r.evals) == (m, 16, 16 << m)


# ------------------------------------------------------------------ 4. the tolerance walk
def test_walk_converges_with_the_models_work(cuda):
    case = lc.GAUSS6
    want = lr.lattice_to_tolerance(case.f, case.box, rtol=1e-6, seed=case.seed)
    r, _ = kernels.lattice_expr(case.expr, case.box, rtol=1e-6, seed=case.seed)
    print(r.as_dict(), "model", {k: want[k] for k in ("value", "err_est", "m", "levels", "evals")})
    assert r.converged and want["converged"] and r.err_est <= 1e-6 * abs(r.value)
    assert (r.levels, r.evals, r.m) == (want["levels"], want["evals"], want["m"])
    assert r.evals == sum(16 << k for k in range(12, r.m + 1))
    assert abs(r.value - case.truth()) <= 4 * r.err_est + 1e-13


def test_walk_reports_a_miss(cuda):
    case = lc.BALL3
    r, _ = kernels.lattice_expr(case.expr, case.box, rtol=1e-9, m_max=14, seed=case.seed)
    print(r.as_dict())
    assert not r.converged and math.isfinite(r.value) and math.isfinite(r.err_est)
    assert (r.m, r.levels, r.evals) == (14, 3, 16 * (4096 + 8192 + 16384))
    assert abs(r.value - case.truth()) <= 4 * r.err_est
    res = integrate_expr_nd(case.expr, case.box, rtol=1e-9, m_max=14, seed=case.seed)
    assert not res.converged and _bits([res.value]) == _bits([r.value])


def test_singular_faces_are_never_evaluated(cuda):
    """1 / sqrt(x0 x1) is infinite on two faces of the unit square; every t lies strictly inside
    (0, 1), so every sample is finite (one infinite sample would make an estimate infinite)."""
    case = lc.INV_SQRT2
    r, _ = kernels.lattice_expr(case.expr, case.box, rtol=1e-3, m_max=14)
    print(r.as_dict())
    assert np.all(np.isfinite(r.estimates)) and math.isfinite(r.value) and r.value > 0
    words = np.array([[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0x80000000, 0x7FFFFFFF]], dtype=np.uint32)
    for periodic in (False, True):
        c, _ = kernels.lattice_expr(case.expr, case.box, m=10, shift_words=words, periodic=periodic)
        assert np.all(np.isfinite(c.estimates))


# ------------------------------------------------------------------ 5. the partials buffer
def test_nothing_is_written_past_the_partials(native, cuda):
    """The caller's partials buffer at the file's largest R x gx (17 shifts x 3 workgroups),
    followed by a canary."""
    case, m, rows, grid = lc.SIMPLEX, 10, 17, 3
    need = rows * grid
    assert need == LARGEST_PARTIALS and native.lattice_shape(1 << m, rows, grid) == (grid, rows)
    z, words = lc.z_for(m, case.d), lc.words_for(rows, case.d)
    opt = native.LatticeOptions(z=z, shift_words=[int(w) for w in words.ravel()])
    buf = torch.full((need + 64,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    el = native.ExprLattice(case.expr, case.d, False, cuda.index, grid)
    el.use_partials(buf.data_ptr(), need)
    r = el.integrate(list(case.box), m, opt)
    host = buf.cpu().numpy()
    assert np.all(host[need:] == -7.0) and np.all(host[:need] >= 0.0)
    _check_exact(r, lc.exact_reference(case, m, z, words, False))
    # the partials are the workgroups' sums: a shift's three add up to its S_r
    sums = host[:need].reshape(rows, grid).sum(axis=1)
    assert sums.tolist() == lc.exact_reference(case, m, z, words, False)["sums"]
    el.use_partials(buf.data_ptr(), need - 1)
    with pytest.raises(RuntimeError, match="fewer than shifts x gx = 17 x 3"):
        el.integrate(list(case.box), m, opt)
    el.use_partials(0, 0)
    _check_exact(el.integrate(list(case.box), m, opt), lc.exact_reference(case, m, z, words, False))


# ------------------------------------------------------------------ 6. the four surfaces
def test_four_surfaces_agree_bit_for_bit(native, cuda):
    case, m = lc.GAUSS6, 12
    el = native.ExprLattice(case.expr, case.d)
    obj = el.integrate(list(case.box), m, native.LatticeOptions(seed=case.seed))
    ker, est = kernels.lattice_expr(case.expr, case.box, m=m, seed=case.seed)
    api = integrate_expr_nd(case.expr, case.box, m=m, seed=case.seed)
    exe = os.path.join(REPO, "build", "bin", "riemann")
    box = ",".join(f"{lo!r}:{hi!r}" for lo, hi in case.box)
    p = subprocess.run([exe, "--expr", case.expr, "--box", box, "--m", str(m), "--seed",
                        str(case.seed), "--json", "--analytic", repr(case.truth())],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.splitlines()[-1])
    want = _bits(obj.estimates)
    assert _bits(ker.estimates) == want and _bits(api.estimates) == want
    assert _bits(rec["estimates"]) == want
    for v, e in ((ker.value, ker.err_est), (api.value, api.err_est)):
        assert _bits([v, e]) == _bits([obj.value, obj.err_est])
    assert rec["value_bits"] == struct.pack(">d", obj.value).hex()
    assert rec["err_est_bits"] == struct.pack(">d", obj.err_est).hex()
    assert (rec["m"], rec["n"], rec["shifts"], rec["d"], rec["evals"]) == (m, 1 << m, 16, 6, 16 << m)
    assert rec["abs_err"] == abs(obj.value - case.truth()) and rec["device_ms"] > 0
    assert api.backend == "hip" and api.evals == 16 << m


@pytest.mark.parametrize("ranks", [["--loopback", "3"]])
def test_cli_splits_the_points_over_ranks(cuda, ranks):
    """Three loopback ranks: the value agrees with one rank's to rounding (the ranks' sums meet in
    another order) and the record names the transport."""
    case, m = lc.PROD4, 12
    exe = os.path.join(REPO, "build", "bin", "riemann")
    args = [exe, "--expr", case.expr, "--box", "0:2,0:2,0:2,0:2", "--m", str(m), "--json"]
    one = json.loads(subprocess.run(args, capture_output=True, text=True,
                                    timeout=120).stdout.splitlines()[-1])
    p = subprocess.run(args + ranks, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.splitlines()[-1])
    assert rec["gpus"] == 3 and rec["comm"] == "loopback" and one["comm"] == "none"
    assert rec["value"] == pytest.approx(one["value"], rel=1e-14)
    assert rec["estimates"] == pytest.approx(one["estimates"], rel=1e-14)
    assert abs(rec["value"] - 16.0) <= 4 * rec["err_est"]
