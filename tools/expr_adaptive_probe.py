#!/usr/bin/env python3
"""Adaptive integration of a run-time expression (ExprAdaptive) against the route there was
before it: guess n, run ExprIntegrator's midpoint rule, look at the error
(profiles/r21/expr_adaptive.md).

Three integrands at rtol = 1e-10: a resonance 1.0/(x*x+1e-8) on [-1, 1], the smooth exp(-x*x)
on [0, 3] and the endpoint singularity 1.0/sqrt(x) on [0, 1]. For each, the adaptive call from
256, 4096 and 65536 panels: end to end (a host clock around synchronous calls) and device time
(events around back-to-back calls, the rounds' syncs inside), rounds, evals and the true error.
Beside them the fixed-n route: the smallest n of 1e4, 1e5, ..., 1e9 whose midpoint sum meets
the same tolerance against the closed form, and its time. Everything that is timed alternates,
ROUNDS times each, after the clocks have settled on the same work. Last, the device's counts
beside the numpy model's for the cases of tests/test_expr_adaptive_gpu.py.

    python tools/expr_adaptive_probe.py [--md profiles/r21/expr_adaptive.md] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

RTOL = 1e-10
PANELS = (256, 4096, 65536)
FIXED_N = tuple(10 ** k for k in range(4, 10))


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def main() -> int:
    import expr_adaptive_cases as ac
    from cuda_v_mpi_amd._native import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    if m.device_count() < 1:
        raise SystemExit("expr_adaptive_probe needs a HIP device")
    cases = [ac.RESONANCE, ac.GAUSS3, ac.INV_SQRT]
    out = {"rtol": RTOL, "rounds_of_timing": a.rounds, "iters": a.iters, "cases": {}}
    for case in cases:
        ea = m.ExprAdaptive(case.expr, 0)
        ei = m.ExprIntegrator(case.expr, 0)
        tol = RTOL * abs(case.truth)
        opts = {p: m.AdaptOptions(rtol=RTOL, panels=p) for p in PANELS}
        # the fixed-n route: the smallest n that meets the tolerance
        fixed = []
        for n in FIXED_N:
            v = ei.integrate(case.a, case.b, n, m.Rule.mid, 0, n)
            fixed.append({"n": n, "abs_err": abs(v - case.truth)})
        reached = next((f["n"] for f in fixed if f["abs_err"] <= tol), None)
        n_fixed = reached or FIXED_N[-1]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:   # settle the clocks on the timed work
            for p in PANELS:
                ea.time(case.a, case.b, opts[p], 5)
            ei.time(case.a, case.b, n_fixed, m.Rule.mid, 0, n_fixed, 2)
        rec = {"truth": case.truth, "tol": tol, "fixed_errors": fixed, "fixed_n": reached,
               "adaptive": {}}
        dev = {p: [] for p in PANELS}
        e2e = {p: [] for p in PANELS}
        dev_f, e2e_f = [], []
        for _ in range(a.rounds):
            for p in PANELS:
                dev[p].append(ea.time(case.a, case.b, opts[p], a.iters))
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    ea.integrate(case.a, case.b, opts[p])
                e2e[p].append((time.perf_counter() - t0) / a.iters * 1e3)
            dev_f.append(ei.time(case.a, case.b, n_fixed, m.Rule.mid, 0, n_fixed, 5))
            t0 = time.perf_counter()
            for _ in range(5):
                ei.integrate(case.a, case.b, n_fixed, m.Rule.mid, 0, n_fixed)
            e2e_f.append((time.perf_counter() - t0) / 5 * 1e3)
        for p in PANELS:
            r = ea.integrate(case.a, case.b, opts[p])
            rec["adaptive"][p] = {
                "value": r.value, "abs_err": abs(r.value - case.truth), "err_est": r.err_est,
                "converged": r.converged, "rounds": r.rounds, "evals": r.evals,
                "intervals": r.intervals, "forced": r.forced, "floor": r.floor,
                "device_ms": med(dev[p]), "device_spread": spread(dev[p]),
                "e2e_ms": med(e2e[p]), "e2e_spread": spread(e2e[p]),
                "device_us_per_round": med(dev[p]) * 1e3 / r.rounds,
                "e2e_us_per_round": med(e2e[p]) * 1e3 / r.rounds}
        rec["fixed"] = {"n": n_fixed, "reached": reached is not None,
                        "device_ms": med(dev_f), "device_spread": spread(dev_f),
                        "e2e_ms": med(e2e_f), "e2e_spread": spread(e2e_f)}
        out["cases"][case.name] = dict(rec, expr=case.expr, a=case.a, b=case.b)
        del ea, ei
    # the device's counts beside the model's, for the cases the GPU tests hold to [0.8, 1.25]
    counts = []
    runs = [(c, dict(rtol=r, panels=p)) for c in ac.TOLERANCE for r in ac.RTOLS
            for p in (4096, ac.FEW_PANELS)] + [(ac.COS2000, ac.COS2000_ARGS)]
    for case, args in runs:
        want = ac.model(case, **args)
        r = m.ExprAdaptive(case.expr, 0).integrate(case.a, case.b, m.AdaptOptions(**args))
        counts.append({"case": case.name, "rtol": args["rtol"], "panels": args["panels"],
                       "device_evals": r.evals, "model_evals": want["evals"],
                       "device_rounds": r.rounds, "model_rounds": want["rounds"],
                       "device_splits": r.splits, "model_splits": want["splits"],
                       "abs_err": abs(r.value - case.truth), "tol": r.tol})
    out["counts"] = counts
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
    ls = ["# Adaptive integration of a run-time expression (r21)", "",
          f"One MI355X, `tools/expr_adaptive_probe.py`, one process, rtol = {out['rtol']:g}. "
          f"Device time is events around {out['iters']} back-to-back calls (`ExprAdaptive::time`: "
          "the rounds' syncs and the host's reads are inside), end to end is a host clock around "
          f"{out['iters']} synchronous calls. The panel counts and the fixed-n route alternate, "
          f"{out['rounds_of_timing']} rounds each, after 1 s of the same work; a figure is the "
          "median of the rounds, the spread max - min.", "",
          "## Adaptive, by panel count", "",
          "| integrand | panels | rounds | evals | true error | tol | converged | device ms "
          "(spread) | end to end ms (spread) | device us / round | end to end us / round |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, c in out["cases"].items():
        for p, r in c["adaptive"].items():
            ls.append(f"| `{c['expr']}` on [{c['a']:g}, {c['b']:g}] | {p} | {r['rounds']} | "
                      f"{r['evals']} | {r['abs_err']:.2e} | {c['tol']:.2e} | "
                      f"{'yes' if r['converged'] else 'no'} | {r['device_ms']:.4f} "
                      f"({r['device_spread']:.4f}) | {r['e2e_ms']:.4f} ({r['e2e_spread']:.4f}) | "
                      f"{r['device_us_per_round']:.1f} | {r['e2e_us_per_round']:.1f} |")
    ls += ["", "## The route before: `ExprIntegrator`, midpoint rule, n guessed", "",
           "True error of the midpoint sum at each n; the first n that meets the same tolerance "
           "is timed (1e9 where none does).", "",
           "| integrand | " + " | ".join(f"n = {n:.0e}" for n in FIXED_N) + " | smallest n | "
           "device ms (spread) | end to end ms (spread) |",
           "|---|" + "---|" * (len(FIXED_N) + 3)]
    for name, c in out["cases"].items():
        errs = " | ".join(f"{f['abs_err']:.1e}" for f in c["fixed_errors"])
        fx = c["fixed"]
        ls.append(f"| `{c['expr']}` | {errs} | "
                  f"{('%.0e' % fx['n']) if fx['reached'] else 'not reached at 1e9'} | "
                  f"{fx['device_ms']:.4f} ({fx['device_spread']:.4f}) | "
                  f"{fx['e2e_ms']:.4f} ({fx['e2e_spread']:.4f}) |")
    ls += ["", "## Device and model counts (the cases of tests/test_expr_adaptive_gpu.py)", "",
           "| case | rtol | panels | evals device / model | rounds device / model | splits "
           "device / model | true error | tol |", "|---|---|---|---|---|---|---|---|"]
    for r in out["counts"]:
        ls.append(f"| {r['case']} | {r['rtol']:g} | {r['panels']} | {r['device_evals']} / "
                  f"{r['model_evals']} | {r['device_rounds']} / {r['model_rounds']} | "
                  f"{r['device_splits']} / {r['model_splits']} | {r['abs_err']:.1e} | "
                  f"{r['tol']:.1e} |")
    return "\n".join(ls) + "\n"


if __name__ == "__main__":
    sys.exit(main())
