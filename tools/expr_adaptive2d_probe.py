#!/usr/bin/env python3
"""Adaptive double integrals of a run-time expression (ExprAdaptive2D) against the route there
was before it: guess n, run ExprIntegrator2D's midpoint rule on n x n samples, look at the error
(profiles/r25/expr_adaptive2d.md).

The converged cases of tests/expr_adaptive2d_cases.py at rtol = 1e-10 from 64 x 64 panels: end
to end (a host clock around synchronous calls) and device time (events around back-to-back
calls, the rounds' syncs inside), rounds, evals and the true error. Beside each the fixed-n
route at n = 256, 512, ..., 32768 per axis: the true error at each n, the first n that meets
the tolerance rtol |truth| and the first that meets the adaptive run's own true error, and the
time of the former (of n = 32768 where none does). Then a one-round call from 64 x 64 panels
beside ExprAdaptive's one-round call from 65536 panels (about the same evaluations), the eval
kernel's registers and scratch, and the hipRTC compile beside the 1-D adaptive compile of the
same expression. Everything that is timed alternates, ROUNDS times each, after the clocks have
settled on the same work.

    python tools/expr_adaptive2d_probe.py [--md profiles/r25/expr_adaptive2d.md] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

RTOL = 1e-10
FIXED_N = tuple(256 << k for k in range(8))    # 256 .. 32768 per axis
RESOURCE_EXPRS = ("1.0/(x*x+y*y+0.01)", "exp(-(x*x+y*y))")


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def kernel_resources(code: bytes, kernel: str) -> dict:
    """vgpr_count, sgpr_count, scratch bytes and spills of one kernel, from the code object's
    notes (llvm-readelf of the ROCm installation). No device needed."""
    exe = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        notes = subprocess.run([exe, "--notes", f.name], capture_output=True, text=True,
                               check=True).stdout
    for block in notes.split(".name:")[1:]:
        if block.split()[0] == kernel:
            found = dict(re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|"
                                    r"vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block))
            return {k: int(v) for k, v in found.items()}
    raise SystemExit(f"no kernel {kernel} in the code object")


def compile_seconds(m, tag: int) -> dict:
    """One cold hipRTC compile of each family for an expression no cache has seen (the
    constant carries `tag`)."""
    out = {}
    for name, expr2, expr1 in (("rational", f"1.0/(x*x+y*y+0.{tag}1)", f"1.0/(x*x+x*x+0.{tag}1)"),
                               ("exp", f"exp(-(x*x+y*y)*1.{tag})", f"exp(-(x*x+x*x)*1.{tag})")):
        t0 = time.perf_counter()
        code2 = m.expr_adapt2d_compile(expr2)
        t1 = time.perf_counter()
        code1 = m.expr_adapt_compile(expr1)
        t2 = time.perf_counter()
        out[name] = {"expr2d": expr2, "expr1d": expr1, "adaptive2d_s": t1 - t0,
                     "adaptive1d_s": t2 - t1, "adaptive2d_bytes": len(code2),
                     "adaptive1d_bytes": len(code1)}
    return out


def main() -> int:
    import expr_adaptive2d_cases as ac
    from cuda_v_mpi_amd._native import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    out = {"rtol": RTOL, "rounds_of_timing": a.rounds, "iters": a.iters, "cases": {}}
    out["resources"] = {e: kernel_resources(m.expr_adapt2d_compile(e), "miint_adapt2d_eval")
                        for e in RESOURCE_EXPRS}
    out["compile"] = compile_seconds(m, int(time.time()) % 100000)
    if m.device_count() < 1:
        raise SystemExit("expr_adaptive2d_probe needs a HIP device for the timings")
    cases = [ac.GAUSS, ac.PEAK, ac.RIDGE, ac.DIAGONAL, ac.CORNER, ac.EDGE, ac.LOG_CORNER]
    opt = m.Adapt2DOptions(rtol=RTOL)
    for case in cases:
        ea = m.ExprAdaptive2D(case.expr, 0)
        ei = m.ExprIntegrator2D(case.expr, 0, 0)
        box = case.box
        tol = RTOL * abs(case.truth)
        r = ea.integrate(*box, opt)
        err = abs(r.value - case.truth)
        fixed = []
        for n in FIXED_N:
            v = ei.integrate(box[0], box[1], n, box[2], box[3], n, m.Rule.mid, 0, n)
            fixed.append({"n": n, "abs_err": abs(v - case.truth)})
        meets_tol = next((f["n"] for f in fixed if f["abs_err"] <= tol), None)
        meets_err = next((f["n"] for f in fixed if f["abs_err"] <= err), None)
        n_fixed = meets_tol or FIXED_N[-1]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:   # settle the clocks on the timed work
            ea.time(*box, opt, 3)
            ei.time(box[0], box[1], n_fixed, box[2], box[3], n_fixed, m.Rule.mid, 0, n_fixed, 2)
        dev, e2e, dev_f, e2e_f = [], [], [], []
        for _ in range(a.rounds):
            dev.append(ea.time(*box, opt, a.iters))
            t0 = time.perf_counter()
            for _ in range(a.iters):
                ea.integrate(*box, opt)
            e2e.append((time.perf_counter() - t0) / a.iters * 1e3)
            dev_f.append(ei.time(box[0], box[1], n_fixed, box[2], box[3], n_fixed, m.Rule.mid, 0,
                                 n_fixed, 3))
            t0 = time.perf_counter()
            for _ in range(3):
                ei.integrate(box[0], box[1], n_fixed, box[2], box[3], n_fixed, m.Rule.mid, 0,
                             n_fixed)
            e2e_f.append((time.perf_counter() - t0) / 3 * 1e3)
        out["cases"][case.name] = {
            "expr": case.expr, "box": list(box), "truth": case.truth, "tol": tol,
            "adaptive": {"value": r.value, "abs_err": err, "err_est": r.err_est,
                         "converged": r.converged, "rounds": r.rounds, "evals": r.evals,
                         "intervals": r.intervals, "splits_x": r.splits_x,
                         "splits_y": r.splits_y, "floor": r.floor, "forced": r.forced,
                         "device_ms": med(dev), "device_spread": spread(dev),
                         "e2e_ms": med(e2e), "e2e_spread": spread(e2e),
                         "device_us_per_round": med(dev) * 1e3 / r.rounds,
                         "e2e_us_per_round": med(e2e) * 1e3 / r.rounds},
            "fixed_errors": fixed,
            "fixed": {"n": n_fixed, "meets_tol": meets_tol, "meets_adaptive_error": meets_err,
                      "device_ms": med(dev_f), "device_spread": spread(dev_f),
                      "e2e_ms": med(e2e_f), "e2e_spread": spread(e2e_f)}}
        del ea, ei
    # one round: 64 x 64 rectangles (921 600 evaluations) beside 65536 intervals (983 040)
    e2 = m.ExprAdaptive2D("exp(-(x*x+y*y))", 0)
    e1 = m.ExprAdaptive("exp(-x*x)", 0)
    o2, o1 = m.Adapt2DOptions(rtol=1e-6), m.AdaptOptions(rtol=1e-6)
    r2, r1 = e2.integrate(0.0, 3.0, 0.0, 3.0, o2), e1.integrate(0.0, 3.0, o1)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        e2.time(0.0, 3.0, 0.0, 3.0, o2, 20)
        e1.time(0.0, 3.0, o1, 20)
    d2, d1 = [], []
    for _ in range(a.rounds):
        d2.append(e2.time(0.0, 3.0, 0.0, 3.0, o2, 50))
        d1.append(e1.time(0.0, 3.0, o1, 50))
    out["one_round"] = {"adaptive2d": {"rounds": r2.rounds, "evals": r2.evals,
                                       "device_ms": med(d2), "device_spread": spread(d2)},
                        "adaptive1d": {"rounds": r1.rounds, "evals": r1.evals,
                                       "device_ms": med(d1), "device_spread": spread(d1)}}
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
    ls = ["# Adaptive double integrals of a run-time expression (r25)", "",
          f"One MI355X, `tools/expr_adaptive2d_probe.py`, one process, rtol = {out['rtol']:g}, "
          "64 x 64 panels. Device time is events around "
          f"{out['iters']} back-to-back calls (`ExprAdaptive2D::time`: the rounds' syncs and the "
          "host's reads are inside), end to end is a host clock around "
          f"{out['iters']} synchronous calls. The adaptive call and the fixed-n route alternate, "
          f"{out['rounds_of_timing']} rounds each, after 1 s of the same work; a figure is the "
          "median of the rounds, the spread max - min.", "",
          "## Adaptive", "",
          "| integrand | rounds | evals | rectangles | splits x / y | true error | tol | "
          "converged | device ms (spread) | end to end ms (spread) | device us / round | "
          "end to end us / round |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in out["cases"].values():
        r, b = c["adaptive"], c["box"]
        ls.append(f"| `{c['expr']}` on [{b[0]:g}, {b[1]:g}] x [{b[2]:g}, {b[3]:g}] | "
                  f"{r['rounds']} | {r['evals']} | {r['intervals']} | {r['splits_x']} / "
                  f"{r['splits_y']} | {r['abs_err']:.2e} | {c['tol']:.2e} | "
                  f"{'yes' if r['converged'] else 'no'} | {r['device_ms']:.4f} "
                  f"({r['device_spread']:.4f}) | {r['e2e_ms']:.4f} ({r['e2e_spread']:.4f}) | "
                  f"{r['device_us_per_round']:.1f} | {r['e2e_us_per_round']:.1f} |")
    ls += ["", "## The route before: `ExprIntegrator2D`, midpoint rule, n x n samples, n guessed",
           "", "True error of the midpoint sum at each n per axis. `meets tol`: the first n whose "
           "error is within rtol |truth|; `meets adaptive`: the first whose error is within the "
           "adaptive run's own true error. The time is that of `meets tol`, or of n = 32768 "
           "(2^30 samples) where no n does.", "",
           "| integrand | " + " | ".join(f"n = {n}" for n in FIXED_N) + " | meets tol | meets "
           "adaptive | timed n | device ms (spread) | end to end ms (spread) |",
           "|---|" + "---|" * (len(FIXED_N) + 5)]
    for c in out["cases"].values():
        errs = " | ".join(f"{f['abs_err']:.1e}" for f in c["fixed_errors"])
        fx = c["fixed"]
        ls.append(f"| `{c['expr']}` | {errs} | {fx['meets_tol'] or 'none'} | "
                  f"{fx['meets_adaptive_error'] or 'none'} | {fx['n']} | "
                  f"{fx['device_ms']:.4f} ({fx['device_spread']:.4f}) | "
                  f"{fx['e2e_ms']:.4f} ({fx['e2e_spread']:.4f}) |")
    o = out["one_round"]
    ls += ["", "## One round", "",
           "`exp(-(x*x+y*y))` on [0, 3]^2 from 64 x 64 rectangles beside `exp(-x*x)` on [0, 3] "
           "from 65536 intervals, rtol 1e-6, events around 50 back-to-back calls.", "",
           "| call | rounds | evals | device ms (spread) |", "|---|---|---|---|"]
    for name, key in (("ExprAdaptive2D", "adaptive2d"), ("ExprAdaptive", "adaptive1d")):
        r = o[key]
        ls.append(f"| {name} | {r['rounds']} | {r['evals']} | {r['device_ms']:.4f} "
                  f"({r['device_spread']:.4f}) |")
    ls += ["", "## The eval kernel's registers (code object notes, `miint_adapt2d_eval`)", "",
           "| integrand | VGPRs | SGPRs | scratch bytes | VGPR spills |", "|---|---|---|---|---|"]
    for e, r in out["resources"].items():
        ls.append(f"| `{e}` | {r.get('vgpr_count')} | {r.get('sgpr_count')} | "
                  f"{r.get('private_segment_fixed_size')} | {r.get('vgpr_spill_count')} |")
    ls += ["", "## hipRTC compile, cold, on the probe's host", "",
           "| integrand | 2-D adaptive s | bytes | 1-D adaptive s | bytes |", "|---|---|---|---|---|"]
    for c in out["compile"].values():
        ls.append(f"| `{c['expr2d']}` (1-D: `{c['expr1d']}`) | {c['adaptive2d_s']:.2f} | "
                  f"{c['adaptive2d_bytes']} | {c['adaptive1d_s']:.2f} | {c['adaptive1d_bytes']} |")
    return "\n".join(ls) + "\n"


if __name__ == "__main__":
    sys.exit(main())
