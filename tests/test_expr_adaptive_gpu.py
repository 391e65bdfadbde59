"""GPU tests of adaptive integration (ExprAdaptive, csrc/runtime/expr_adaptive.cpp): the device
against closed-form truths and against the numpy model of the same rule
(cuda_v_mpi_amd/utils/adaptive_quad.py; its own checks are in test_expr_adaptive_cpu.py).

The value's bound. A converged run is held to

    |value - truth| <= max(tol, err_est) + 96 * 2^-52 * resabs

The first term is what the rule promises. The second is rounding, which the estimate does not
see (the model's |x - 1/3| run has err_est 3e-17 and a true error of 5e-16). With u = 2^-53 and
R_i the rule's integral of |f| over interval i (resabs is their sum), from the kernels' own
order of summation:
  * K_i: f to 2 u relative (the device library's bound for the functions used here), the pair sum
    u, eight chained fma u each, the product with hw u: 12 u R_i;
  * the round's sum of the accepted K: a 64-lane butterfly (6 additions), the four waves (2),
    then in the closing workgroup a run of at most ceil(workgroups / 256) <= 64 partials and
    another butterfly and four waves (8): at most 80 u R of the round;
  * the rounds, added in order: at most 61 additions, 61 u R;
  * the truth, rounded to a double: u |truth| <= u R.
Together 154 u R = 77 * 2^-52 R; the tests use 96. What f makes of a rounded argument
(cos(200 x) turns a node's u into 200 u of f) is not rounding of the sums and is not in the
slack: for the cases here it stays an order of magnitude inside tol."""
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

import expr_adaptive_cases as ac
from cuda_v_mpi_amd import integrate_expr_adaptive, native
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v: float) -> str:
    return struct.pack(">d", v).hex()


def _identities(r, panels):
    assert r.intervals == panels + r.splits
    assert r.evals == 15 * (r.intervals + r.splits)


def _partition(lo, hi, a, b, n):
    """n intervals running from a to b, each one's upper end the next one's lower end, bit for
    bit."""
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    assert lo.shape == hi.shape == (n,)
    assert lo[0] == a and hi[-1] == b
    assert np.array_equal(hi[:-1], lo[1:])
    return lo, hi


# ------------------------------------------------------------------ 1. smooth, one round
@pytest.mark.parametrize("panels", [1, 3, 64, 257])
@pytest.mark.parametrize("case", ac.SMOOTH, ids=repr)
def test_smooth_integrands_take_one_round(case, panels):
    """257 panels put one lane alone in a second workgroup."""
    want = ac.model(case, panels=panels)
    r = kernels.quad_expr(case.expr, case.a, case.b, panels=panels)
    print(case, panels, r.as_dict(), "model rounds", want["rounds"], "splits", want["splits"])
    if want["rounds"] == 1 and want["splits"] == 0:
        assert r.rounds == 1 and r.splits == 0 and r.intervals == panels
    _identities(r, panels)
    if r.converged:
        assert abs(r.value - case.truth) <= ac.value_bound(r)
    assert r.converged == want["converged"]
    # one panel of 4/(1+x*x) misses 1e-10 in the model and is bisected: the device follows
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]


# ------------------------------------------------------------------ 2 and 4. tolerance met
@pytest.mark.parametrize("panels", [ac.PANELS, ac.FEW_PANELS])
@pytest.mark.parametrize("rtol", ac.RTOLS)
@pytest.mark.parametrize("case", ac.TOLERANCE, ids=repr)
def test_tolerance_met_with_the_models_work(case, rtol, panels):
    """Converged, the value within the bound of the module docstring, and the work placed as
    the model places it: evals within [0.8, 1.25] of the model's. A lost or doubled child, or a
    split of everything, lands far outside; a borderline decision that the device library
    rounds the other way moves one small subtree."""
    want = ac.model(case, rtol=rtol, panels=panels)
    r = kernels.quad_expr(case.expr, case.a, case.b, rtol=rtol, panels=panels)
    print(case, rtol, panels, r.as_dict(), "model evals", want["evals"], "rounds",
          want["rounds"], "|value - truth|", abs(r.value - case.truth), "bound", ac.value_bound(r))
    assert r.converged and not r.capped and r.nonfinite == 0
    assert abs(r.value - case.truth) <= ac.value_bound(r)
    _identities(r, panels)
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]


# ------------------------------------------------------------------ 3. several workgroups
def test_interleaved_splits_across_workgroups():
    """cos(2000 x) from one panel: 11 rounds, 1011 intervals and a list of up to 998 in the
    model, so the scatter's prefix crosses workgroups with splits and acceptances mixed in each.
    All edges are dyadic, so the widths add up to b - a exactly."""
    case, args = ac.COS2000, ac.COS2000_ARGS
    want = ac.model(case, **args)
    r, lo, hi = kernels.quad_expr(case.expr, case.a, case.b, return_intervals=True, **args)
    print(r.as_dict(), "model", {k: want[k] for k in ("rounds", "intervals", "evals", "peak")})
    assert r.converged and abs(r.value - case.truth) <= ac.value_bound(r)
    _identities(r, 1)
    lo, hi = _partition(lo, hi, case.a, case.b, r.intervals)
    assert np.all(hi > lo) and np.all(np.diff(lo) > 0)
    assert math.fsum(hi - lo) == case.b - case.a
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]
    assert abs(int(r.rounds) - want["rounds"]) <= 1 and r.intervals >= 600
    # the same partition as the model wherever no decision was borderline: most edges shared
    shared = np.intersect1d(lo, want["lo"]).size
    assert shared >= 0.8 * max(lo.size, want["lo"].size)


# ------------------------------------------------------------------ 5. honest failures
def test_endpoint_singularity_reports_non_convergence():
    want = ac.model(ac.INV_SQRT, rtol=1e-13, panels=ac.PANELS)
    r = kernels.quad_expr(ac.INV_SQRT.expr, 0.0, 1.0, rtol=1e-13, panels=ac.PANELS)
    print(r.as_dict(), "model", {k: want[k] for k in ("rounds", "evals", "forced", "floor")})
    assert not r.converged and r.forced >= 1 and r.rounds == 60 + 1
    assert abs(r.value - 2.0) <= 1e-9 and not r.capped and r.nonfinite == 0
    _identities(r, ac.PANELS)


def test_nan_integrand_is_accepted_and_counted():
    r = kernels.quad_expr(ac.SQRT_NEG.expr, -1.0, 1.0, panels=ac.PANELS)
    print(r.as_dict())
    assert r.nonfinite >= 1 and math.isnan(r.value) and not r.converged and r.rounds <= 3
    _identities(r, ac.PANELS)


def test_cap_stops_the_run_and_writes_nothing_past_the_buffer():
    """max_intervals = panels = 64: the first split would pass the cap. The caller's interval
    buffer is followed by a canary."""
    m = native()
    case = ac.RESONANCE
    opt = m.AdaptOptions(panels=64, max_intervals=64)
    buf = torch.full((64 + 64, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ea = m.ExprAdaptive(case.expr, 0)
    r = ea.integrate(case.a, case.b, opt, buf.data_ptr(), 64)
    print(r.as_dict(), "truth", case.truth)
    assert r.capped and not r.converged and math.isfinite(r.value)
    assert r.intervals <= 64 and abs(r.value - case.truth) <= 10 * r.err_est
    _identities(r, 64)
    host = buf.cpu().numpy()
    assert np.all(host[64:] == -7.0)
    _partition(torch.from_numpy(host[:r.intervals, 0]), torch.from_numpy(host[:r.intervals, 1]),
               case.a, case.b, r.intervals)
    with pytest.raises(RuntimeError, match="fewer than max_intervals = 64"):
        ea.integrate(case.a, case.b, opt, buf.data_ptr(), 63)


def test_max_depth_zero_accepts_everything_in_one_round():
    r = kernels.quad_expr(ac.RESONANCE.expr, -1.0, 1.0, max_depth=0, panels=ac.PANELS)
    assert r.rounds == 1 and r.splits == 0 and r.intervals == ac.PANELS and r.forced >= 1
    assert not r.converged and r.evals == 15 * ac.PANELS


# ------------------------------------------------------------------ 6. reproducible
def test_bitwise_reproducible_across_calls_and_objects():
    m = native()
    case, args = ac.COS2000, ac.COS2000_ARGS
    opt = m.AdaptOptions(**args)
    cap = opt.max_intervals

    def run(ea):
        buf = torch.zeros((cap, 2), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        r = ea.integrate(case.a, case.b, opt, buf.data_ptr(), cap)
        return _bits(r.value), _bits(r.err_est), r.intervals, buf[:r.intervals].cpu().numpy()

    first = m.ExprAdaptive(case.expr, 0)
    one = run(first)
    small = first.integrate(0.0, 0.001, m.AdaptOptions(panels=3))   # a small problem between
    assert small.rounds >= 1 and small.intervals >= 3
    for other in (run(first), run(m.ExprAdaptive(case.expr, 0))):
        assert other[:3] == one[:3] and np.array_equal(other[3], one[3])
    again = first.integrate(0.0, 0.001, m.AdaptOptions(panels=3))
    assert _bits(again.value) == _bits(small.value) and again.evals == small.evals


# ------------------------------------------------------------------ 7. a > b, a == b
def test_reversed_range_negates_and_empty_range_is_zero():
    case = ac.RESONANCE
    fwd, flo, fhi = kernels.quad_expr(case.expr, -1.0, 0.5, rtol=1e-8, panels=ac.PANELS,
                                      return_intervals=True)
    rev, rlo, rhi = kernels.quad_expr(case.expr, 0.5, -1.0, rtol=1e-8, panels=ac.PANELS,
                                      return_intervals=True)
    assert _bits(rev.value) == _bits(-fwd.value) and _bits(rev.err_est) == _bits(fwd.err_est)
    assert rev.evals == fwd.evals and rev.converged and fwd.converged
    _partition(rlo, rhi, 0.5, -1.0, rev.intervals)
    assert torch.equal(rlo.flip(0), fhi) and torch.equal(rhi.flip(0), flo)
    z = kernels.quad_expr(case.expr, 0.25, 0.25)
    assert _bits(z.value) == _bits(0.0) and z.evals == 0 and z.rounds == 0 and z.converged


# ------------------------------------------------------------------ 8. surfaces agree
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


FLAGS = ("--expr", ac.RESONANCE.expr, "--a", "-1", "--b", "1", "--rtol", "1e-9", "--panels", "32")


@pytest.fixture(scope="module")
def surface_value():
    """kernels.quad_expr's result for FLAGS: what every other surface has to print."""
    return kernels.quad_expr(ac.RESONANCE.expr, -1.0, 1.0, rtol=1e-9, panels=32)


def test_python_api_and_native_cli_agree_bit_for_bit(surface_value):
    r = surface_value
    api = integrate_expr_adaptive(ac.RESONANCE.expr, -1.0, 1.0, rtol=1e-9, panels=32,
                                  backend="hip")
    assert _bits(api.value) == _bits(r.value) and api.evals == r.evals and api.converged
    p = _riemann(*FLAGS, "--json")
    assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds", "intervals",
              "splits", "floor", "forced", "nonfinite", "capped", "device_ms"):
        assert k in js, k
    assert _bits(js["value"]) == _bits(r.value) and js["evals"] == r.evals
    assert js["value_bits"] == _bits(r.value) and js["err_est"] == r.err_est


def test_python_cli_agrees_bit_for_bit(surface_value):
    r = surface_value
    p = subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *FLAGS], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert _bits(js["value"]) == _bits(r.value) and js["rounds"] == r.rounds


def test_native_cli_prints_the_value_and_warns_when_not_converged():
    """The plain form prints the value alone; not converged: one warning line on stderr."""
    r = kernels.quad_expr(ac.INV_SQRT.expr, 0.0, 1.0, rtol=1e-13)
    p = _riemann("--expr", ac.INV_SQRT.expr, "--a", "0", "--b", "1", "--rtol", "1e-13")
    assert p.returncode == 0
    assert len([l for l in p.stderr.splitlines() if "not converged" in l]) == 1, p.stderr
    assert not r.converged and _bits(float(p.stdout.strip())) == _bits(r.value)
