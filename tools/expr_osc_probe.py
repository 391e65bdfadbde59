#!/usr/bin/env python3
"""The oscillatory integrator (ExprAdaptiveOsc) against ExprAdaptive on the typed product
f(x) * cos(W * x) with the same options (profiles/r27/expr_osc.md).

The finite cases of tests/expr_osc_cases.py at their own tolerance from 64 panels (the default
max_intervals = 2^22): device time (events around back-to-back calls, the rounds' syncs inside),
end to end (a host clock around synchronous calls), rounds, evals, the true error and whether the
run converged or capped; beside each, interleaved, ExprAdaptive on the product typed into the
expression. Two Fourier tails (the sum of the cycles' device times, end to end). The cost of a
one-round call from 65536 panels (max_depth = 0) for both classes, interleaved. The registers and
scratch of both twins for every case's f. The largest |value - model| / (2^-52 resabs) over the
omega != 0 cases from 4 and from 64 panels with max_intervals = 4096, which the GPU tests bound.

    python tools/expr_osc_probe.py [--md profiles/r27/expr_osc.md] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from expr_adaptive2d_probe import kernel_resources, med, spread   # noqa: E402

PANELS = 64


def product(case) -> str:
    return f"({case.expr})*{case.kind}({case.omega!r}*x)"


def timed(time_call, run_call, rounds, iters):
    dev, e2e = [], []
    for _ in range(rounds):
        dev.append(time_call(iters))
        t0 = time.perf_counter()
        for _ in range(iters):
            run_call()
        e2e.append((time.perf_counter() - t0) / iters * 1e3)
    return {"device_ms": med(dev), "device_spread": spread(dev), "e2e_ms": med(e2e),
            "e2e_spread": spread(e2e)}


def main() -> int:
    import math

    import expr_osc_cases as oc
    from cuda_v_mpi_amd._native import native
    from cuda_v_mpi_amd.utils import adaptive_osc as ao

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    out = {"rounds_of_timing": a.rounds, "iters": a.iters, "panels": PANELS, "cases": {},
           "tails": {}, "resources": {}}
    for expr in sorted({c.expr for c in oc.FINITE}):
        code = m.expr_osc_compile(expr)
        out["resources"][expr] = {k: kernel_resources(code, f"miint_osc_eval_{k}")
                                  for k in ("cos", "sin")}
    out["resources_gk"] = kernel_resources(m.expr_adapt_compile(oc.LORENTZ), "miint_adapt_eval")
    if m.device_count() < 1:
        raise SystemExit("expr_osc_probe needs a HIP device for the timings")
    objs: dict = {}

    def osc(expr):
        if expr not in objs:
            objs[expr] = m.ExprAdaptiveOsc(expr, 0)
        return objs[expr]

    for case in oc.FINITE:
        opt = m.AdaptOptions(rtol=case.rtol, atol=case.atol, panels=PANELS)
        eo, ea = osc(case.expr), m.ExprAdaptive(product(case), 0)
        truth = oc.truth(case)
        args = (case.a, case.b, case.omega, case.kind)
        r, g = eo.integrate(*args, opt), ea.integrate(case.a, case.b, opt)
        heavy = g.evals > 5_000_000
        it = 2 if heavy else a.iters
        rec = {"expr": case.expr, "a": case.a, "b": case.b, "omega": case.omega,
               "kind": case.kind, "truth": truth, "product": product(case)}
        for name, res, tcall, rcall in (
                ("osc", r, lambda n: eo.time(*args, opt, n), lambda: eo.integrate(*args, opt)),
                ("gk", g, lambda n: ea.time(case.a, case.b, opt, n),
                 lambda: ea.integrate(case.a, case.b, opt))):
            rec[name] = dict(timed(tcall, rcall, a.rounds, it), value=res.value,
                             abs_err=abs(res.value - truth), err_est=res.err_est, tol=res.tol,
                             converged=res.converged, capped=res.capped, rounds=res.rounds,
                             evals=res.evals, intervals=res.intervals)
        out["cases"][case.id] = rec
        del ea
    for case in oc.TAILS_GPU:
        eo = osc(case.expr)
        opt = m.AdaptOptions(rtol=0.0, atol=case.atol)
        r = eo.integrate_tail(case.a, case.omega, case.kind, opt)
        dev, e2e = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            q = eo.integrate_tail(case.a, case.omega, case.kind, opt)
            e2e.append((time.perf_counter() - t0) * 1e3)
            dev.append(q.device_ms)
        truth = oc.tail_truth(case)
        out["tails"][case.id] = dict(
            expr=case.expr, a=case.a, omega=case.omega, kind=case.kind, truth=truth,
            abs_err=abs(r.value - truth), err_est=r.err_est, converged=r.converged,
            cycles=r.cycles, extrapolated=r.extrapolated, evals=r.evals, rounds=r.rounds,
            device_ms=med(dev), device_spread=spread(dev), e2e_ms=med(e2e),
            e2e_spread=spread(e2e))
    # one round from 65536 panels, the two classes interleaved
    one = m.AdaptOptions(rtol=1e-10, panels=65536, max_depth=0)
    eo, ea = osc(oc.LORENTZ), m.ExprAdaptive(oc.LORENTZ, 0)
    calls = {"ExprAdaptive": lambda n: ea.time(0.0, 10.0, one, n),
             "ExprAdaptiveOsc cos W=50": lambda n: eo.time(0.0, 10.0, 50.0, "cos", one, n),
             "ExprAdaptiveOsc sin W=1e4": lambda n: eo.time(0.0, 10.0, 1e4, "sin", one, n)}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        for c in calls.values():
            c(20)
    ms = {k: [] for k in calls}
    for _ in range(max(a.rounds, 5)):
        for k, c in calls.items():
            ms[k].append(c(50))
    out["one_round"] = {k: {"device_ms": med(v), "device_spread": spread(v)}
                        for k, v in ms.items()}
    # the figure the GPU tests bound
    worst, where = 0.0, ""
    for case in oc.FINITE:
        if case.omega == 0.0:
            continue
        for panels in oc.PANELS:
            opt = m.AdaptOptions(rtol=case.rtol, atol=case.atol, panels=panels,
                                 max_intervals=4096)
            r = osc(case.expr).integrate(case.a, case.b, case.omega, case.kind, opt)
            want = ao.osc_model(oc.f_numpy(case.expr), case.a, case.b, case.omega, case.kind,
                                rtol=case.rtol, atol=case.atol, panels=panels,
                                max_intervals=4096)
            ratio = abs(r.value - want["value"]) / (math.ldexp(1.0, -52) * r.resabs)
            if ratio > worst:
                worst, where = ratio, f"{case.id} from {panels}"
    out["model_ratio"] = {"largest": worst, "where": where}
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(markdown(out))
    print(text)
    return 0


def markdown(out) -> str:
    ls = ["# Oscillatory weights: ExprAdaptiveOsc (r27)", "",
          f"One MI355X, `tools/expr_osc_probe.py`, one process, from {out['panels']} panels, "
          "max_intervals 2^22, every case at the tolerance `tests/expr_osc_cases.py` holds it to "
          "(rtol 1e-10; `gauss` with atol 1e-14). Device time is events around back-to-back calls "
          "(`time()`: the rounds' syncs and the host's reads are inside), end to end is a host "
          f"clock around synchronous calls; {out['iters']} calls a round (2 where the "
          f"Gauss-Kronrod run passes 5e6 evaluations), {out['rounds_of_timing']} rounds, the two "
          "classes interleaved; a figure is the median of the rounds, the spread max - min. "
          "`ExprAdaptive` integrates the product typed into the expression with the same "
          "options.", "",
          "| case | class | rounds | evals | intervals | true error | tol | converged | capped | "
          "device ms (spread) | end to end ms (spread) |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, c in out["cases"].items():
        for cls, key in (("ExprAdaptiveOsc", "osc"), (f"ExprAdaptive on `{c['product']}`", "gk")):
            q = c[key]
            ls.append(f"| {name} | {cls} | {q['rounds']} | {q['evals']} | {q['intervals']} | "
                      f"{q['abs_err']:.2e} | {q['tol']:.2e} | {'yes' if q['converged'] else 'no'} "
                      f"| {'yes' if q['capped'] else 'no'} | {q['device_ms']:.4f} "
                      f"({q['device_spread']:.4f}) | {q['e2e_ms']:.4f} ({q['e2e_spread']:.4f}) |")
    ls += ["", "## The Fourier tail on (a, inf), atol 1e-10, 16 panels a cycle", "",
           "| case | cycles | extrapolated | rounds | evals | true error | err_est | converged | "
           "device ms, the cycles' sum (spread) | end to end ms (spread) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for name, q in out["tails"].items():
        ls.append(f"| {name}: `{q['expr']}` from {q['a']:g} | {q['cycles']} | "
                  f"{'yes' if q['extrapolated'] else 'no'} | {q['rounds']} | {q['evals']} | "
                  f"{q['abs_err']:.2e} | {q['err_est']:.2e} | "
                  f"{'yes' if q['converged'] else 'no'} | {q['device_ms']:.4f} "
                  f"({q['device_spread']:.4f}) | {q['e2e_ms']:.4f} ({q['e2e_spread']:.4f}) |")
    ls += ["", "## One round from 65536 panels (max_depth = 0), `1.0/(1.0+x*x)` on [0, 10]", "",
           "Events around 50 back-to-back calls, the three calls interleaved after 1 s of the "
           "same work. The oscillatory call also computes and sends one row of the weight table "
           "when omega or the range changed; here it is cached after the first call.", "",
           "| call | device ms (spread) |", "|---|---|"]
    for k, r in out["one_round"].items():
        ls.append(f"| {k} | {r['device_ms']:.4f} ({r['device_spread']:.4f}) |")
    ls += ["", "## The device against the numpy model", "",
           "The largest |value_gpu - value_model| / (2^-52 resabs) over every omega != 0 case from "
           f"4 and from 64 panels with max_intervals 4096: **{out['model_ratio']['largest']:.4g}** "
           f"({out['model_ratio']['where']}). `tests/test_expr_osc_gpu.py` bounds it at 8 x that.",
           "", "The largest absolute error of `osc_weights` against 50-digit values over par in "
           "{0, 1e-8, 1e-3, 0.5, 2, 7, 24, 25, 100, 1e3, 1e5, 1e7} and their negatives, measured "
           "on the host: 2.64e-17 (`tests/test_expr_osc_cpu.py` bounds it at 4 x that; 2^-48 is "
           "3.55e-15).", "",
           "## The twins' registers (code object notes)", "",
           "| f | kernel | VGPRs | SGPRs | scratch bytes | VGPR spills | SGPR spills |",
           "|---|---|---|---|---|---|---|"]
    for expr, both in out["resources"].items():
        for kind, r in both.items():
            ls.append(f"| `{expr}` | `miint_osc_eval_{kind}` | {r.get('vgpr_count')} | "
                      f"{r.get('sgpr_count')} | {r.get('private_segment_fixed_size')} | "
                      f"{r.get('vgpr_spill_count')} | {r.get('sgpr_spill_count')} |")
    r = out["resources_gk"]
    ls.append(f"| `1.0/(1.0+x*x)` | `miint_adapt_eval` | {r.get('vgpr_count')} | "
              f"{r.get('sgpr_count')} | {r.get('private_segment_fixed_size')} | "
              f"{r.get('vgpr_spill_count')} | {r.get('sgpr_spill_count')} |")
    return "\n".join(ls) + "\n"


if __name__ == "__main__":
    sys.exit(main())
