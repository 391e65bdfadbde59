#!/usr/bin/env python3
"""Adaptive sweeps (ExprAdaptiveSweep) against the route there was before them: one
ExprAdaptive call per row (profiles/r23/expr_adaptive_sweep.md).

The family is 1.0/((x-p0)*(x-p0)+p1) on [-1, 1] at rtol = 1e-10, K rows with p0 spread over
[-0.9, 0.9] and p1 cycling through 1e-2, 1e-4, ..., 1e-10. ExprAdaptive takes no parameters, so
the loop keeps one object per p1 (five compiles, outside the clock) and moves p0 into the range:
row k is 1.0/(x*x+p1) on [-1 - p0, 1 - p0], the same integral. That form is the easier one: with
the peak at 0 the argument x is exact, while x - p0 carries the rounding of x, which at p1 =
1e-10 reaches the rule's noise floor and costs those rows several times the evaluations (the
numpy model shows the same). The comparison therefore favours the loop. What is timed, the two
routes alternating:
  * the claim: K = 4096, one sweep call against the K calls (at 65536 and at 16 panels), device
    time (the results' device_ms: events around the rounds) and end to end (a host clock);
  * the same at K = 8 and K = 2^16 from 16 panels (the loop at 2^16 once);
  * one row: K = 1 against ExprAdaptive on the same integrand and options, us per round;
  * the tail: a sweep of the 4096 rows cut off after 1, 2, 3 and 5 rounds (max_depth), which are
    the rounds with every row active, and a sweep of the 8 hardest rows alone, whose rounds are
    what the last rounds of the big run hold;
  * the initial total: 2^16, 2^18 and 2^20 initial intervals for the 4096 rows;
  * the registers and scratch of the kernels with 8 parameters, from the code object.

    python tools/expr_adaptive_sweep_probe.py [--md FILE.md] [--out FILE.json]
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
EXPR = "1.0/((x-p0)*(x-p0)+p1)"
P1 = (1e-2, 1e-4, 1e-6, 1e-8, 1e-10)
EXPR8 = "p0+p1*x+p2*x*x+p3*sin(p4*x)+p5*exp(-p6*x*x)+p7"


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def family(k: int):
    import numpy as np

    p0 = np.linspace(-0.9, 0.9, k) if k > 1 else np.array([0.0])
    p1 = np.array([P1[i % len(P1)] for i in range(k)])
    return np.stack([p0, p1], axis=1)


def truth(rows):
    import mpmath as mp

    out = []
    for s, e in rows:
        r = mp.sqrt(mp.mpf(float(e)))
        out.append(float((mp.atan((1 - mp.mpf(float(s))) / r)
                          - mp.atan((-1 - mp.mpf(float(s))) / r)) / r))
    return out


def code_object_registers(code: bytes) -> dict:
    """vgpr_count, sgpr_count and the scratch bytes of every kernel from the code object's
    metadata (llvm-readelf of the ROCm installation); empty when there is none."""
    tool = None
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/llvm-readelf", "lib/llvm/bin/llvm-readelf"):
        if os.path.exists(os.path.join(root, sub)):
            tool = os.path.join(root, sub)
    if tool is None:
        return {}
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        notes = subprocess.run([tool, "--notes", f.name], capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\w+)", block)
        if not name:
            continue
        out[name.group(1)] = {
            key: int(hit.group(1)) for key in ("vgpr_count", "sgpr_count",
                                               "private_segment_fixed_size", "vgpr_spill_count")
            for hit in [re.search(r"\." + key + r":\s+(\d+)", block)] if hit}
    return out


def main() -> int:
    import numpy as np

    from cuda_v_mpi_amd._native import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-large", action="store_true", help="leave out K = 2^16")
    a = ap.parse_args()
    m = native()
    out = {"rtol": RTOL, "expr": EXPR, "rounds_of_timing": a.rounds,
           "registers_8_parameters": code_object_registers(m.expr_adapt_sweep_compile(EXPR8, 8))}
    if m.device_count() < 1:
        raise SystemExit("expr_adaptive_sweep_probe needs a HIP device")
    es = m.ExprAdaptiveSweep(EXPR, 2, 0)
    singles = [m.ExprAdaptive(f"1.0/(x*x+{e:g})", 0) for e in P1]

    def sweep(rows, **opts):
        o = m.AdaptSweepOptions(rtol=RTOL, **opts)
        t0 = time.perf_counter()
        r = es.integrate(rows, -1.0, 1.0, o)
        return r, (time.perf_counter() - t0) * 1e3

    def loop(rows, panels):
        o = m.AdaptOptions(rtol=RTOL, panels=panels)
        dev, rounds, evals, worst, values = 0.0, 0, 0, 0, []
        t0 = time.perf_counter()
        for k, (s, _) in enumerate(rows):
            r = singles[k % len(P1)].integrate(-1.0 - s, 1.0 - s, o)
            dev += r.device_ms
            rounds += r.rounds
            evals += r.evals
            worst = max(worst, r.rounds)
            values.append(r.value)
        return dict(e2e_ms=(time.perf_counter() - t0) * 1e3, device_ms=dev, rounds=rounds,
                    evals=evals, most_rounds=worst, values=values)

    def compare(k, loop_panels, passes, loop_passes, max_total):
        print(f"K = {k} ...", file=sys.stderr, flush=True)
        rows = family(k)
        want = truth(rows[:64])
        sweep(rows, panels=16, max_total=max_total)          # warm: buffers, clocks
        loop(rows[:min(k, 256)], 16)
        sw_dev, sw_e2e, lp = [], [], {p: {"device_ms": [], "e2e_ms": []} for p in loop_panels}
        last = {}
        for i in range(passes):
            r, ms = sweep(rows, panels=16, max_total=max_total)
            sw_dev.append(r.device_ms)
            sw_e2e.append(ms)
            if i < loop_passes:
                for p in loop_panels:
                    last[p] = loop(rows, p)
                    lp[p]["device_ms"].append(last[p]["device_ms"])
                    lp[p]["e2e_ms"].append(last[p]["e2e_ms"])
        rec = {"rows": k, "max_total": max_total,
               "sweep": {"panels": 16, "device_ms": med(sw_dev), "device_spread": spread(sw_dev),
                         "e2e_ms": med(sw_e2e), "e2e_spread": spread(sw_e2e), "passes": passes,
                         "call_rounds": r.call_rounds, "call_evals": r.call_evals, "peak": r.peak,
                         "not_converged": int((~r.converged).sum()),
                         "capped": int(r.capped.sum()),
                         "rows_with_floor": int((r.floor > 0).sum()),
                         "worst_err_over_tol_first_64": max(
                             abs(v - t) / tl for v, t, tl in zip(r.value[:64], want, r.tol[:64]))},
               "loop": {}}
        for p in loop_panels:
            rec["loop"][p] = {
                "device_ms": med(lp[p]["device_ms"]), "device_spread": spread(lp[p]["device_ms"]),
                "e2e_ms": med(lp[p]["e2e_ms"]), "e2e_spread": spread(lp[p]["e2e_ms"]),
                "passes": len(lp[p]["e2e_ms"]), "rounds_summed": last[p]["rounds"],
                "most_rounds": last[p]["most_rounds"], "evals": last[p]["evals"],
                "device_ratio": med(lp[p]["device_ms"]) / med(sw_dev),
                "e2e_ratio": med(lp[p]["e2e_ms"]) / med(sw_e2e)}
        return rec

    out["claim"] = compare(4096, (65536, 16), a.rounds, a.rounds, 1 << 22)
    out["k8"] = compare(8, (16,), a.rounds, a.rounds, 1 << 22)
    if not a.skip_large:
        out["k65536"] = compare(1 << 16, (16,), 3, 1, 1 << 25)

    print("one row, the tail, the initial total ...", file=sys.stderr, flush=True)
    # one row against ExprAdaptive: the same integrand and options
    one = {}
    row = np.array([[0.0, 1e-8]])
    for panels in (16, 65536):
        so = m.AdaptSweepOptions(rtol=RTOL, panels=panels, max_intervals=1 << 22)
        ao = m.AdaptOptions(rtol=RTOL, panels=panels)
        ds, da = [], []
        for _ in range(a.rounds):
            ds.append(es.time(row, -1.0, 1.0, so, 10))
            da.append(singles[3].time(-1.0, 1.0, ao, 10))
        rs = es.integrate(row, -1.0, 1.0, so)
        ra = singles[3].integrate(-1.0, 1.0, ao)
        one[panels] = {
            "sweep": {"device_ms": med(ds), "device_spread": spread(ds),
                      "rounds": int(rs.call_rounds), "evals": int(rs.call_evals),
                      "us_per_round": med(ds) * 1e3 / rs.call_rounds, "launches_per_round": 4},
            "adaptive": {"device_ms": med(da), "device_spread": spread(da), "rounds": ra.rounds,
                         "evals": ra.evals, "us_per_round": med(da) * 1e3 / ra.rounds,
                         "launches_per_round": 5}}
    out["one_row"] = one

    # the tail: rounds with every row active, and rounds with a handful left
    rows = family(4096)
    early = {}
    for depth in (0, 1, 2, 4):
        o = m.AdaptSweepOptions(rtol=RTOL, panels=16, max_depth=depth)
        t = [es.time(rows, -1.0, 1.0, o, 5) for _ in range(a.rounds)]
        r = es.integrate(rows, -1.0, 1.0, o)
        early[depth] = {"device_ms": med(t), "device_spread": spread(t),
                        "rounds": int(r.call_rounds), "evals": int(r.call_evals),
                        "peak": int(r.peak)}
    hardest = rows[rows[:, 1] == 1e-10][:8]
    o = m.AdaptSweepOptions(rtol=RTOL, panels=16)
    t = [es.time(hardest, -1.0, 1.0, o, 10) for _ in range(a.rounds)]
    r = es.integrate(hardest, -1.0, 1.0, o)
    out["tail"] = {"early": early,
                   "us_per_round_all_active": (early[4]["device_ms"] - early[0]["device_ms"])
                   * 1e3 / (early[4]["rounds"] - early[0]["rounds"]),
                   "late": {"rows": 8, "device_ms": med(t), "device_spread": spread(t),
                            "rounds": int(r.call_rounds),
                            "us_per_round": med(t) * 1e3 / r.call_rounds}}

    # the initial total
    initial = {}
    for panels in (16, 64, 256):
        dev, e2e = [], []
        for _ in range(a.rounds):
            r, ms = sweep(rows, panels=panels)
            dev.append(r.device_ms)
            e2e.append(ms)
        initial[4096 * panels] = {"panels": panels, "device_ms": med(dev),
                                  "device_spread": spread(dev), "e2e_ms": med(e2e),
                                  "e2e_spread": spread(e2e), "rounds": int(r.call_rounds),
                                  "evals": int(r.call_evals), "peak": int(r.peak)}
    out["initial_total"] = initial

    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(markdown(out))
    print(text)
    return 0


def markdown(out) -> str:
    ls = ["# Adaptive sweeps of a run-time expression (r23)", "",
          f"One MI355X, `tools/expr_adaptive_sweep_probe.py`, one process. `{out['expr']}` on "
          f"[-1, 1] at rtol = {out['rtol']:g}; K rows, p0 spread over [-0.9, 0.9], p1 cycling "
          "through 1e-2 ... 1e-10. The sweep is one `ExprAdaptiveSweep` call from 16 panels a "
          "row. The loop is the route before: one `ExprAdaptive` call per row (one object per "
          "p1, compiled outside the clock; p0 moved into the range). Device time is the "
          "results' `device_ms` (events around the rounds, summed over the loop's calls), end to "
          "end a host clock around the call or the whole loop. The routes alternate in one "
          "process; a figure is the median of the passes, the spread max - min. The loop's form "
          "of the integrand is the easier one (the peak at 0: x - p0 carries the rounding of x, "
          "which at p1 = 1e-10 reaches the rule's noise floor and costs the sweep's rows more "
          "evaluations, in the numpy model too), so the ratios understate the like-for-like "
          "gain.", "",
          "## One sweep against K calls", "",
          "| K | route | panels | rounds | evals | device ms (spread) | end to end ms (spread) | "
          "loop / sweep, device | loop / sweep, end to end |", "|---|---|---|---|---|---|---|---|---|"]
    for key in ("k8", "claim", "k65536"):
        if key not in out:
            continue
        c = out[key]
        s = c["sweep"]
        ls.append(f"| {c['rows']} | sweep | 16 | {s['call_rounds']} | {s['call_evals']} | "
                  f"{s['device_ms']:.3f} ({s['device_spread']:.3f}) | {s['e2e_ms']:.3f} "
                  f"({s['e2e_spread']:.3f}) | 1 | 1 |")
        for p, l in c["loop"].items():
            ls.append(f"| {c['rows']} | loop ({l['passes']} passes) | {p} | {l['rounds_summed']} "
                      f"summed, {l['most_rounds']} at most | {l['evals']} | {l['device_ms']:.1f} "
                      f"({l['device_spread']:.1f}) | {l['e2e_ms']:.1f} ({l['e2e_spread']:.1f}) | "
                      f"{l['device_ratio']:.1f} | {l['e2e_ratio']:.1f} |")
    ls += ["", "Rows not converged in the sweeps (capped; rows with intervals accepted at the noise "
           "floor): "
           + ", ".join(f"K = {out[k]['rows']}: {out[k]['sweep']['not_converged']} "
                       f"({out[k]['sweep']['capped']}; {out[k]['sweep']['rows_with_floor']})"
                       for k in ("k8", "claim", "k65536") if k in out)
           + "; max_total = " + ", ".join(str(out[k]["max_total"])
                                          for k in ("k8", "claim", "k65536") if k in out)
           + "; the worst |value - truth| / tol over the first 64 rows: "
           + ", ".join(f"{out[k]['sweep']['worst_err_over_tol_first_64']:.2g}"
                       for k in ("k8", "claim", "k65536") if k in out) + ".", "",
           "## One row: K = 1 against `ExprAdaptive`", "",
           "`1.0/(x*x+1e-8)` (p0 = 0, p1 = 1e-8), the same options; events around 10 "
           "back-to-back calls.", "",
           "| panels | route | launches / round | rounds | device ms (spread) | us / round |",
           "|---|---|---|---|---|---|"]
    for p, c in out["one_row"].items():
        for route in ("sweep", "adaptive"):
            r = c[route]
            ls.append(f"| {p} | {route} | {r['launches_per_round']} | {r['rounds']} | "
                      f"{r['device_ms']:.4f} ({r['device_spread']:.4f}) | {r['us_per_round']:.1f} |")
    t = out["tail"]
    ls += ["", "## The tail", "",
           "The 4096 rows cut off by max_depth (every row is active in these rounds), and the 8 "
           "hardest rows alone (what the last rounds of the big run hold: the row kernels walk "
           "the compacted list of active rows).", "",
           "| run | rounds | evals | longest list | device ms (spread) |", "|---|---|---|---|---|"]
    for d, r in t["early"].items():
        ls.append(f"| 4096 rows, max_depth = {d} | {r['rounds']} | {r['evals']} | {r['peak']} | "
                  f"{r['device_ms']:.4f} ({r['device_spread']:.4f}) |")
    lt = t["late"]
    ls += [f"| 8 hardest rows | {lt['rounds']} | | | {lt['device_ms']:.4f} "
           f"({lt['device_spread']:.4f}) |", "",
           f"A round with every row active: {t['us_per_round_all_active']:.1f} us (max_depth 4 "
           f"against 0); a round with 8 rows left: {lt['us_per_round']:.1f} us.", "",
           "## The initial total, 4096 rows", "",
           "| initial intervals | panels | rounds | evals | longest list | device ms (spread) | "
           "end to end ms (spread) |", "|---|---|---|---|---|---|---|"]
    for total, r in out["initial_total"].items():
        ls.append(f"| {total} | {r['panels']} | {r['rounds']} | {r['evals']} | {r['peak']} | "
                  f"{r['device_ms']:.3f} ({r['device_spread']:.3f}) | {r['e2e_ms']:.3f} "
                  f"({r['e2e_spread']:.3f}) |")
    ls += ["", "## Registers, 8 parameters", "",
           "`p0+p1*x+p2*x*x+p3*sin(p4*x)+p5*exp(-p6*x*x)+p7`, from the code object's metadata.",
           "", "| kernel | VGPRs | SGPRs | scratch bytes | spilled VGPRs |", "|---|---|---|---|---|"]
    for name, r in out["registers_8_parameters"].items():
        ls.append(f"| {name} | {r.get('vgpr_count')} | {r.get('sgpr_count')} | "
                  f"{r.get('private_segment_fixed_size')} | {r.get('vgpr_spill_count')} |")
    return "\n".join(ls) + "\n"


if __name__ == "__main__":
    sys.exit(main())
