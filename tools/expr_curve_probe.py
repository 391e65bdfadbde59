#!/usr/bin/env python3
"""Per-row ranges in adaptive sweeps and the running integral to a tolerance (ExprAdaptiveSweep::
integrate_ranges, ExprAdaptiveCurve) against the routes there were before them
(profiles/r29/expr_curve.md). The routes alternate inside every pass; medians over the passes.

  * ranged against shared: K = 8 and 4096 rows of 1.0/((x-p0)*(x-p0)+p1) at rtol = 1e-10 with
    [-1, 1] given per row, against the same rows on the shared [-1, 1]: what the twin kernels
    and the upload of the ranges cost;
  * ranged against the route before: the same ranged rows against K one-row calls;
  * the curve: exp(-x*x) on [0, 3] and 1.0/sqrt(x) on [0, 1] at M = 1000 and 65536 equal cells,
    against M ExprAdaptive calls (the curve's own panels per call) and against ExprScan (the
    midpoint rule, n = M, 4 M, 16 M, ... up to 2^30) at the first n whose every grid point is
    within the tolerance the curve reports for it, or "not reached";
  * the prefix kernel alone at M = 2^20;
  * the registers and scratch of the twin row kernel, from the code object.

    python tools/expr_curve_probe.py [--md FILE.md] [--out FILE.json] [--passes N]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from expr_adaptive_sweep_probe import EXPR, RTOL, code_object_registers, family  # noqa: E402

CURVES = (("exp(-x*x)", 0.0, 3.0, lambda x: math.sqrt(math.pi) / 2.0 * math.erf(x)),
          ("1.0/sqrt(x)", 0.0, 1.0, lambda x: 2.0 * math.sqrt(x)))
SCAN_MAX_N = 1 << 30


def med(v):
    return statistics.median(v)


def main() -> int:
    import numpy as np

    from cuda_v_mpi_amd._native import native
    from cuda_v_mpi_amd.ops import kernels

    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    regs = code_object_registers(m.expr_adapt_sweep_ranges_compile())
    regs["miint_asweep_row"] = code_object_registers(
        m.expr_adapt_sweep_compile(EXPR, 2)).get("miint_asweep_row", {})
    out = {"rtol": RTOL, "passes": a.passes, "registers": regs, "sweep": [], "curve": []}
    if m.device_count() < 1:
        raise SystemExit("expr_curve_probe needs a HIP device")

    def clocked(call):
        t0 = time.perf_counter()
        r = call()
        return r, (time.perf_counter() - t0) * 1e3

    # ------------------------------------------------------------- ranged against shared
    es = m.ExprAdaptiveSweep(EXPR, 2, 0)
    for k in (8, 4096):
        rows = family(k)
        lo, hi = [-1.0] * k, [1.0] * k
        o = m.AdaptSweepOptions(rtol=RTOL, panels=16, max_intervals=1024)
        one = m.AdaptSweepOptions(rtol=RTOL, panels=16, max_intervals=1024, max_total=1024)
        es.integrate(rows, -1.0, 1.0, o), es.integrate_ranges(rows, lo, hi, o)   # warm
        t = {key: [] for key in ("shared_dev", "shared_e2e", "ranged_dev", "ranged_e2e",
                                 "loop_dev", "loop_e2e")}
        for p in range(a.passes):
            s, ms = clocked(lambda: es.integrate(rows, -1.0, 1.0, o))
            t["shared_dev"].append(s.device_ms), t["shared_e2e"].append(ms)
            r, ms = clocked(lambda: es.integrate_ranges(rows, lo, hi, o))
            t["ranged_dev"].append(r.device_ms), t["ranged_e2e"].append(ms)
            if k <= 8 or p == 0:   # the route before: K one-row calls
                t0, dev, rounds = time.perf_counter(), 0.0, 0
                for i in range(k):
                    q = es.integrate(rows[i:i + 1], -1.0, 1.0, one)
                    dev += q.device_ms
                    rounds += q.call_rounds
                t["loop_dev"].append(dev), t["loop_e2e"].append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(np.asarray(getattr(s, f)), np.asarray(getattr(r, f)))
                   for f in ("value", "err_est", "evals", "rounds"))
        out["sweep"].append(dict(rows=k, bitwise_equal=bool(same), call_rounds=int(r.call_rounds),
                                 loop_rounds=int(rounds), call_evals=int(r.call_evals),
                                 **{key: med(v) for key, v in t.items()},
                                 **{key + "_spread": max(v) - min(v) for key, v in t.items()}))

    # ------------------------------------------------------------- the curve
    for expr, x0, x1, truth in CURVES:
        ec = m.ExprAdaptiveCurve(expr, 0)
        ea = m.ExprAdaptive(expr, 0)
        for cells in (1000, 65536):
            x = x0 + ((x1 - x0) * np.arange(cells + 1, dtype=np.float64)) / cells
            x[-1] = x1
            o = m.AdaptSweepOptions(rtol=RTOL)
            used = m.adapt_curve_check(x, o)
            ec.integrate(x, o)   # warm
            t = {key: [] for key in ("curve_dev", "curve_e2e", "loop_dev", "loop_e2e")}
            for p in range(a.passes):
                r, ms = clocked(lambda: ec.integrate(x, o))
                t["curve_dev"].append(r.device_ms), t["curve_e2e"].append(ms)
                if p == 0:   # M ExprAdaptive calls on the curve's own panels, once
                    ao = m.AdaptOptions(rtol=RTOL, panels=used.panels,
                                        max_intervals=used.max_intervals)
                    t0, dev, rounds, acc, worst = time.perf_counter(), 0.0, 0, 0.0, 0.0
                    for c in range(cells):
                        q = ea.integrate(float(x[c]), float(x[c + 1]), ao)
                        dev += q.device_ms
                        rounds += q.rounds
                        acc += q.value
                        worst = max(worst, abs(acc - truth(float(x[c + 1]))))
                    t["loop_dev"].append(dev)
                    t["loop_e2e"].append((time.perf_counter() - t0) * 1e3)
            want = np.array([truth(float(v)) for v in x])
            err = np.abs(r.value - want)
            rec = dict(expr=expr, cells=cells, panels=int(used.panels),
                       max_intervals=int(used.max_intervals), call_rounds=int(r.call_rounds),
                       call_evals=int(r.call_evals), peak=int(r.peak),
                       unconverged=int(r.unconverged), worst_err=float(err.max()),
                       worst_err_over_tol=float((err[1:] / r.tol[1:]).max()),
                       total_tol=float(r.total_tol), loop_rounds=int(rounds),
                       loop_worst_err=float(worst), **{key: med(v) for key, v in t.items()},
                       curve_dev_spread=max(t["curve_dev"]) - min(t["curve_dev"]))
            # ExprScan, the midpoint rule: the first n that puts every point within the curve's tol
            rec["scan"] = "not reached"
            every = 1
            while cells * every <= SCAN_MAX_N:
                values, s = kernels._expr_scan(expr, x0, x1, cells * every, "mid", every, 0,
                                               None, None)
                f = np.concatenate([[0.0], values.cpu().numpy()])
                worst = float(np.abs(f - want).max())
                if np.all(np.abs(f - want)[1:] <= r.tol[1:]):
                    rec["scan"] = dict(n=cells * every, device_ms=float(s["device_ms"]),
                                       worst_err=worst)
                    break
                rec["scan_last"] = dict(n=cells * every, device_ms=float(s["device_ms"]),
                                        worst_err=worst)
                every *= 4
            out["curve"].append(rec)
        if expr == CURVES[0][0]:
            out["prefix_kernel_ms_at_2^20"] = ec.time_prefix(1 << 20, 20)

    text = json.dumps(out, indent=1, default=float)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(markdown(out))
    return 0


def markdown(out: dict) -> str:
    lines = ["# Per-row ranges and the running integral to a tolerance", "",
             f"One MI355X, rtol = {out['rtol']:g}, medians over {out['passes']} passes, the "
             "routes alternating inside a pass (tools/expr_curve_probe.py).", "",
             "## Ranged sweep against the shared range and against K one-row calls", "",
             "| rows | shared device ms | ranged device ms | shared end to end ms | ranged end to "
             "end ms | K calls device ms | K calls end to end ms | rounds (call / K calls) | "
             "bitwise equal |", "|---|---|---|---|---|---|---|---|---|"]
    for s in out["sweep"]:
        lines.append(f"| {s['rows']} | {s['shared_dev']:.3f} | {s['ranged_dev']:.3f} | "
                     f"{s['shared_e2e']:.3f} | {s['ranged_e2e']:.3f} | {s['loop_dev']:.2f} | "
                     f"{s['loop_e2e']:.2f} | {s['call_rounds']} / {s['loop_rounds']} | "
                     f"{s['bitwise_equal']} |")
    lines += ["", "## The curve", "",
              "| f | M | panels | rounds | evals | curve device ms | curve end to end ms | M "
              "ExprAdaptive calls, end to end ms (rounds) | ExprScan (mid) | worst err / tol | "
              "cells not converged |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in out["curve"]:
        scan = c["scan"]
        if isinstance(scan, dict):
            scan = f"n = {scan['n']}: {scan['device_ms']:.3f} ms"
        else:
            last = c.get("scan_last", {})
            scan = (f"not reached (n = {last.get('n')}: {last.get('device_ms', 0):.3f} ms, worst "
                    f"error {last.get('worst_err', float('nan')):.2e})")
        lines.append(f"| `{c['expr']}` | {c['cells']} | {c['panels']} | {c['call_rounds']} | "
                     f"{c['call_evals']} | {c['curve_dev']:.3f} | {c['curve_e2e']:.3f} | "
                     f"{c['loop_e2e']:.1f} ({c['loop_rounds']}) | {scan} | "
                     f"{c['worst_err_over_tol']:.3f} | {c['unconverged']} |")
    lines += ["", f"The prefix kernel alone at M = 2^20: {out['prefix_kernel_ms_at_2^20']:.4f} ms.",
              "", "## Registers", "",
              "| kernel | VGPRs | SGPRs | scratch bytes | spilled VGPRs |", "|---|---|---|---|---|"]
    for name, r in out["registers"].items():
        lines.append(f"| {name} | {r.get('vgpr_count')} | {r.get('sgpr_count')} | "
                     f"{r.get('private_segment_fixed_size')} | {r.get('vgpr_spill_count')} |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    sys.exit(main())
