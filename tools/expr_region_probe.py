#!/usr/bin/env python3
"""Double integrals between two curves (ExprAdaptiveRegion) against the routes there were before
it: an indicator on the bounding box through ExprAdaptive2D (which runs to its cap) and through
ExprIntegrator2D's midpoint rule on n x n samples (profiles/r26/expr_region.md).

The cases of tests/expr_region_cases.py at their own tolerance (rtol = 1e-10; `crossing` at
atol = 1e-10) from 64 x 64 panels: end to end (a host clock around synchronous calls) and device
time (events around back-to-back calls, the rounds' syncs inside), rounds, evals and the true
error. For the cases over the disc, beside them, the indicator `(x*x+y*y<1.0)?f:0.0` on
[-1, 1]^2: through ExprAdaptive2D at the same tolerance with max_intervals = 4096 and 2^20, and
through ExprIntegrator2D at n = 4096 ... 32768 per axis. Those two classes are the parent
commit's: this change leaves their generated source byte for byte as it was. Then what the map
costs: one round (max_depth = 0) from 64 x 64 panels of exp(-(x*x+y*y)) over [0, 3] x [0, 3] as a
rectangle, as a region with the constant limits 0.0 and 3.0, and over the part of the disc above
[-0.5, 0.5] with the sqrt limits, interleaved; and the evaluation kernel's registers and
scratch for every case's triple. Everything that is timed alternates, ROUNDS times each, after
the clocks have settled on the same work.

    python tools/expr_region_probe.py [--md profiles/r26/expr_region.md] [--out FILE.json]
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

FIXED_N = (4096, 8192, 16384, 32768)
INDICATOR_CAPS = (4096, 1 << 20)
DISC_BOX = (-1.0, 1.0, -1.0, 1.0)


def timed(obj, args, opt, rounds, iters):
    """Median and spread of the device ms per call and of the end-to-end ms per call."""
    dev, e2e = [], []
    for _ in range(rounds):
        dev.append(obj.time(*args, opt, iters))
        t0 = time.perf_counter()
        for _ in range(iters):
            obj.integrate(*args, opt)
        e2e.append((time.perf_counter() - t0) / iters * 1e3)
    return {"device_ms": med(dev), "device_spread": spread(dev), "e2e_ms": med(e2e),
            "e2e_spread": spread(e2e)}


def settle(calls, seconds=1.0):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for call in calls:
            call()


def main() -> int:
    import expr_region_cases as rc
    from cuda_v_mpi_amd._native import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    out = {"rounds_of_timing": a.rounds, "iters": a.iters, "cases": {}, "indicator": {}}
    out["resources"] = {c.name: dict(kernel_resources(m.expr_region_compile(*c.triple),
                                                      "miint_region_eval"), triple=c.triple)
                        for c in rc.ALL}
    out["resources_rectangle"] = kernel_resources(m.expr_adapt2d_compile(rc.CONSTANT.expr),
                                                  "miint_adapt2d_eval")
    if m.device_count() < 1:
        raise SystemExit("expr_region_probe needs a HIP device for the timings")
    for case in rc.ALL:
        opt = m.Adapt2DOptions(**case.args)
        er = m.ExprAdaptiveRegion(*case.triple, 0)
        r = er.integrate(*case.xrange, opt)
        settle([lambda: er.time(*case.xrange, opt, 3)])
        out["cases"][case.name] = dict(
            timed(er, case.xrange, opt, a.rounds, a.iters), triple=case.triple,
            xrange=list(case.xrange), truth=case.truth, value=r.value,
            abs_err=abs(r.value - case.truth), err_est=r.err_est, tol=r.tol,
            converged=r.converged, rounds=r.rounds, evals=r.evals, intervals=r.intervals,
            splits_x=r.splits_x, splits_y=r.splits_y)
        del er
        if case.y_hi != rc.DISC.y_hi:
            continue
        # the routes before: the indicator on the bounding box
        expr = f"(x*x+y*y<1.0)?({case.expr}):0.0"
        ea = m.ExprAdaptive2D(expr, 0)
        ei = m.ExprIntegrator2D(expr, 0, 0)
        ind = {"expr": expr, "adaptive": [], "fixed": []}
        for cap in INDICATOR_CAPS:
            o = m.Adapt2DOptions(max_intervals=cap, **case.args)
            q = ea.integrate(*DISC_BOX, o)
            settle([lambda: ea.time(*DISC_BOX, o, 1)], 0.5)
            ind["adaptive"].append(dict(
                timed(ea, DISC_BOX, o, a.rounds, 2), max_intervals=cap,
                abs_err=abs(q.value - case.truth), err_est=q.err_est, capped=q.capped,
                converged=q.converged, rounds=q.rounds, evals=q.evals, intervals=q.intervals))
        for n in FIXED_N:
            args = (-1.0, 1.0, n, -1.0, 1.0, n, m.Rule.mid, 0, n)
            v = ei.integrate(*args)
            ei.time(*args, 2)
            ms = [ei.time(*args, 3) for _ in range(a.rounds)]
            ind["fixed"].append({"n": n, "abs_err": abs(v - case.truth), "device_ms": med(ms),
                                 "device_spread": spread(ms)})
        out["indicator"][case.name] = ind
        del ea, ei
    # what the map costs: one round from 64 x 64 panels, the three calls interleaved
    g = rc.CONSTANT
    one = m.Adapt2DOptions(rtol=1e-10, max_depth=0)
    rect = m.ExprAdaptive2D(g.expr, 0)
    const = m.ExprAdaptiveRegion(*g.triple, 0)
    root = m.ExprAdaptiveRegion(g.expr, rc.DISC.y_lo, rc.DISC.y_hi, 0)
    calls = {"rectangle": lambda n: rect.time(0.0, 3.0, 0.0, 3.0, one, n),
             "constant limits": lambda n: const.time(0.0, 3.0, one, n),
             "sqrt limits": lambda n: root.time(-0.5, 0.5, one, n)}
    shown = {"rectangle": rect.integrate(0.0, 3.0, 0.0, 3.0, one),
             "constant limits": const.integrate(0.0, 3.0, one),
             "sqrt limits": root.integrate(-0.5, 0.5, one)}
    settle([lambda c=c: c(20) for c in calls.values()])
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, c in calls.items():
            ms[k].append(c(50))
    out["one_round"] = {k: {"rounds": shown[k].rounds, "evals": shown[k].evals,
                            "device_ms": med(v), "device_spread": spread(v)}
                        for k, v in ms.items()}
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
    ls = ["# Double integrals between two curves (r26)", "",
          "One MI355X, `tools/expr_region_probe.py`, one process, 64 x 64 panels, every case at "
          "the tolerance `tests/expr_region_cases.py` holds it to (rtol 1e-10; `crossing` at atol "
          f"1e-10). Device time is events around {out['iters']} back-to-back calls "
          "(`ExprAdaptiveRegion::time`: the rounds' syncs and the host's reads are inside), end "
          f"to end is a host clock around {out['iters']} synchronous calls, "
          f"{out['rounds_of_timing']} rounds each after 1 s of the same work; a figure is the "
          "median of the rounds, the spread max - min.", "",
          "## `ExprAdaptiveRegion`", "",
          "| case | f | y limits | x range | rounds | evals | rectangles | splits x / v | "
          "true error | tol | converged | device ms (spread) | end to end ms (spread) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, c in out["cases"].items():
        f, lo, hi = c["triple"]
        ls.append(f"| {name} | `{f}` | `{lo}` .. `{hi}` | [{c['xrange'][0]:g}, "
                  f"{c['xrange'][1]:g}] | {c['rounds']} | {c['evals']} | {c['intervals']} | "
                  f"{c['splits_x']} / {c['splits_y']} | {c['abs_err']:.2e} | {c['tol']:.2e} | "
                  f"{'yes' if c['converged'] else 'no'} | {c['device_ms']:.4f} "
                  f"({c['device_spread']:.4f}) | {c['e2e_ms']:.4f} ({c['e2e_spread']:.4f}) |")
    ls += ["", "## The routes before: the indicator `(x*x+y*y<1.0)?f:0.0` on [-1, 1]^2", "",
           "`ExprAdaptive2D` and `ExprIntegrator2D` are unchanged by this feature (their "
           "generated source is byte for byte the parent commit's), so these rows are the "
           "parent's routes measured in the same process.", "",
           "### Through `ExprAdaptive2D`, the same tolerance, from 64 x 64 panels", "",
           "| case | max_intervals | capped | rounds | evals | rectangles | true error | "
           "err_est | device ms (spread) | end to end ms (spread) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for name, ind in out["indicator"].items():
        for q in ind["adaptive"]:
            ls.append(f"| {name} | {q['max_intervals']} | {'yes' if q['capped'] else 'no'} | "
                      f"{q['rounds']} | {q['evals']} | {q['intervals']} | {q['abs_err']:.2e} | "
                      f"{q['err_est']:.2e} | {q['device_ms']:.4f} ({q['device_spread']:.4f}) | "
                      f"{q['e2e_ms']:.4f} ({q['e2e_spread']:.4f}) |")
    ls += ["", "### Through `ExprIntegrator2D`, midpoint rule, n x n samples", "",
           "| case | " + " | ".join(f"n = {n}: true error | device ms (spread)" for n in FIXED_N)
           + " |", "|---|" + "---|---|" * len(FIXED_N)]
    for name, ind in out["indicator"].items():
        ls.append(f"| {name} | " + " | ".join(
            f"{q['abs_err']:.2e} | {q['device_ms']:.3f} ({q['device_spread']:.3f})"
            for q in ind["fixed"]) + " |")
    ls += ["", "## What the map costs: one round", "",
           "`exp(-(x*x+y*y))`, 64 x 64 panels, max_depth = 0 (one round, 921 600 evaluations), "
           "events around 50 back-to-back calls, the three calls interleaved: the rectangle "
           "[0, 3] x [0, 3] through `ExprAdaptive2D`, the same as a region with the limits "
           "`0.0` .. `3.0`, and the part of the disc above [-0.5, 0.5] with the limits "
           "`-sqrt(1.0-x*x)` .. `sqrt(1.0-x*x)`.", "",
           "| call | rounds | evals | device ms (spread) |", "|---|---|---|---|"]
    for k, r in out["one_round"].items():
        ls.append(f"| {k} | {r['rounds']} | {r['evals']} | {r['device_ms']:.4f} "
                  f"({r['device_spread']:.4f}) |")
    ls += ["", "## The evaluation kernel's registers (code object notes, `miint_region_eval`)", "",
           "| case | VGPRs | SGPRs | scratch bytes | VGPR spills | SGPR spills |",
           "|---|---|---|---|---|---|"]
    rows = list(out["resources"].items()) + [
        ("the rectangle's `miint_adapt2d_eval`, `exp(-(x*x+y*y))`", out["resources_rectangle"])]
    for name, r in rows:
        ls.append(f"| {name} | {r.get('vgpr_count')} | {r.get('sgpr_count')} | "
                  f"{r.get('private_segment_fixed_size')} | {r.get('vgpr_spill_count')} | "
                  f"{r.get('sgpr_spill_count')} |")
    return "\n".join(ls) + "\n"


if __name__ == "__main__":
    sys.exit(main())
