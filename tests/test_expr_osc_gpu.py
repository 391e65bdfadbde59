"""GPU tests of the oscillatory integrator (ExprAdaptiveOsc): the device against the numpy
model of utils/adaptive_osc.py on the cases of expr_osc_cases.py, from 4 and from 64 panels with
max_intervals = 4096. With omega = 0 every field and the partition agree bit for bit (sincos(0)
is exact and the cases' f are exact operations); otherwise the structure agrees and the values
to rounding. Then the small properties and the Fourier tail."""
from __future__ import annotations

import functools
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_osc_cases as oc
from cuda_v_mpi_amd import integrate_expr_oscillatory, native
from cuda_v_mpi_amd.utils import adaptive_osc as ao

pytestmark = pytest.mark.gpu

MAX_INTERVALS = 4096
COUNTERS = ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite", "capped",
            "converged")
# |value_gpu - value_model| <= B * 2^-52 * resabs. The largest ratio measured on an MI355X over
# every omega != 0 case from 4 and from 64 panels was RATIO_MEASURED (profiles/r27/expr_osc.md);
# B is 8 x that and, as a condition, never above 4096. The ratio was 0 in 25 of the 26 runs (the
# device's sincos and numpy's agreed to the bit there) and 4.149e-05 for lorentz-cos-w10000 from
# 4 panels.
RATIO_MEASURED = 4.149e-5
B = 8 * RATIO_MEASURED


def bits(v: float) -> str:
    return struct.pack("<d", float(v)).hex()


@functools.lru_cache(maxsize=None)
def model(case, panels):
    return ao.osc_model(oc.f_numpy(case.expr), case.a, case.b, case.omega, case.kind,
                        rtol=case.rtol, atol=case.atol, panels=panels,
                        max_intervals=MAX_INTERVALS)


def device(case, panels, **kw):
    from cuda_v_mpi_amd.ops import kernels

    args = dict(rtol=case.rtol, atol=case.atol, panels=panels, max_intervals=MAX_INTERVALS)
    args.update(kw)
    r, lo, hi = kernels.quad_expr_osc(case.expr, case.a, case.b, case.omega, case.kind,
                                      return_intervals=True, **args)
    return r, np.stack([lo.cpu().numpy(), hi.cpu().numpy()], axis=1)


@pytest.mark.parametrize("panels", oc.PANELS)
@pytest.mark.parametrize("case", oc.ZERO, ids=lambda c: c.id)
def test_omega_zero_is_the_model_bit_for_bit(case, panels):
    r, part = device(case, panels)
    want = model(case, panels)
    for key in ("value", "err_est", "resabs", "tol"):
        assert bits(getattr(r, key)) == bits(want[key]), key
    for key in COUNTERS:
        assert getattr(r, key) == want[key], key
    assert part.shape == want["partition"].shape
    assert part.tobytes() == want["partition"].tobytes()
    if case.kind == "sin":
        assert r.value == 0.0 and r.err_est == 0.0 and r.rounds == 1


@pytest.mark.parametrize("panels", oc.PANELS)
@pytest.mark.parametrize("case", [c for c in oc.FINITE if c.omega != 0.0], ids=lambda c: c.id)
def test_omega_nonzero_against_the_model_and_the_truth(case, panels):
    assert B <= 4096
    r, part = device(case, panels)
    want = model(case, panels)
    for key in ("rounds", "intervals", "splits", "evals", "capped"):
        assert getattr(r, key) == want[key], key
    assert part.tobytes() == want["partition"].tobytes()
    ratio = abs(r.value - want["value"]) / (2.0 ** -52 * r.resabs)
    truth = oc.truth(case)
    print(f"{case.id} from {panels}: ratio {ratio:.4g} true error {abs(r.value - truth):.3e} "
          f"tol {r.tol:.3e} rounds {r.rounds} evals {r.evals} device_ms {r.device_ms:.4f}")
    assert ratio <= B
    assert abs(r.value - truth) <= r.tol
    assert r.omega == case.omega and r.kind == case.kind and r.cycles == 0
    if case.name in ("kink", "sqrt") and case.kind == "cos":
        assert r.rounds > 21      # rows of the weight table past depth 20


def test_small_properties():
    from cuda_v_mpi_amd.ops import kernels

    m = native()
    case = oc.Case("lorentz", oc.LORENTZ, 0.0, 10.0, 50.0, "sin")
    up, part = device(case, 4)
    again, part2 = device(case, 4)
    for key in ("value", "err_est", "resabs", "tol"):
        assert bits(getattr(up, key)) == bits(getattr(again, key))
    assert part.tobytes() == part2.tobytes()
    down, back = device(oc.Case("lorentz", oc.LORENTZ, 10.0, 0.0, 50.0, "sin"), 4)
    assert bits(down.value) == bits(-up.value) and bits(down.err_est) == bits(up.err_est)
    assert back.tobytes() == part[::-1, ::-1].tobytes()
    other = kernels.quad_expr_osc(oc.LORENTZ, 0.0, 10.0, 50.0, "cos", panels=4,
                                  max_intervals=MAX_INTERVALS)
    assert other.kind == "cos" and other.value != up.value
    # an object of its own: a == b launches nothing; another omega re-uploads the table
    eo = m.ExprAdaptiveOsc(oc.LORENTZ, 0)
    opt = m.AdaptOptions(rtol=1e-10, panels=4, max_intervals=MAX_INTERVALS)
    same = eo.integrate(2.0, 2.0, 50.0, "cos", opt)
    assert (same.value, same.rounds, same.evals, same.converged) == (0.0, 0, 0, True)
    assert eo.table_uploads == 0
    first = eo.integrate(0.0, 10.0, 50.0, "sin", opt)
    assert eo.table_uploads == 1 and bits(first.value) == bits(up.value)
    eo.integrate(0.0, 10.0, 50.0, "sin", opt)
    assert eo.table_uploads == 1
    second = eo.integrate(0.0, 10.0, 1.0, "sin", opt)
    assert eo.table_uploads == 2
    fresh = m.ExprAdaptiveOsc(oc.LORENTZ, 0).integrate(0.0, 10.0, 1.0, "sin", opt)
    assert bits(second.value) == bits(fresh.value) and second.rounds == fresh.rounds
    third = eo.integrate(0.0, 10.0, 50.0, "sin", opt)
    assert eo.table_uploads == 3 and bits(third.value) == bits(up.value)
    # a non-finite f at an end is counted, as the model counts it
    end = kernels.quad_expr_osc("1.0/sqrt(x)", 0.0, 1.0, 10.0, "cos", panels=4,
                                max_intervals=MAX_INTERVALS)
    want = ao.osc_model(lambda x: 1.0 / np.sqrt(x), 0.0, 1.0, 10.0, "cos", panels=4,
                        max_intervals=MAX_INTERVALS)
    assert end.nonfinite == want["nonfinite"] == 1 and not end.converged
    assert end.reason.startswith("f was not finite on 1 intervals")


@pytest.mark.parametrize("case", oc.TAILS_GPU, ids=lambda c: c.id)
def test_tail_against_the_model_and_the_truth(case):
    r = integrate_expr_oscillatory(case.expr, case.a, math.inf, case.omega, case.kind,
                                   rtol=0.0, atol=case.atol)
    want = ao.osc_tail_model(oc.f_numpy(case.expr), case.a, case.omega, case.kind,
                             atol=case.atol)
    truth = oc.tail_truth(case)
    print(f"{case.id}: true error {abs(r.value - truth):.3e} cycles {r.cycles} device_ms "
          f"{r.device_ms:.4f}")
    assert r.converged and r.range == "upper" and r.backend == "hip"
    assert abs(r.value - truth) <= case.atol
    assert r.cycles == want["cycles"] and r.extrapolated == want["extrapolated"]
    assert r.evals == want["evals"]
