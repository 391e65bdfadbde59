#!/usr/bin/env python3
"""The running integral of a runtime integrand (ExprScan) on one GPU, one process
(profiles/r15/expr_scan.md):

  scan    4.0/(1.0+x*x) on [0, 1] and exp(-x*x) on [0, 3] at n = 1e8 and 1e9, every = 1 (a
          value per sample: 8 B stored per sample) and every = 10000 (tiles without a selected
          sample are not re-evaluated): device ms per scan, GB/s stored, and the ratio to two
          ExprIntegrator passes over the same n (the scan evaluates f once for the tile sums
          and once more wherever it writes)
  torch   n = 1e8: what a user could do before: evaluate the samples into a tensor with
          torch, torch.cumsum, scale; device ms and the ratio to the scan with every = 1

Every timing: device events, each shape warmed first, the clocks settled by 0.1 s of the same
work, windows of at least 0.25 s, the sides alternating, three repeats; the spread is
(max - min) / median of the repeats.

  python tools/expr_scan_probe.py [--n 1e8,1e9] [--out FILE.jsonl] [--md FILE.md]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 3
WINDOW_S = 0.25
CASES = (("4.0/(1.0+x*x)", 0.0, 1.0), ("exp(-x*x)", 0.0, 3.0))
EVERY = (1, 10000)


def summary(v):
    return {"median": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v),
            "reps": v}


def iters_for(ms_one: float) -> int:
    return max(3, int(math.ceil(WINDOW_S * 1e3 / max(ms_one, 1e-3))))


def settle(fn, seconds: float = 0.1) -> None:
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()


def scan_rows(m, torch, sizes):
    out = []
    for expr, a, b in CASES:
        es, ei = m.ExprScan(expr, 0), m.ExprIntegrator(expr, 0)
        for n in sizes:
            buf = torch.empty(n, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            sides = {"integrate": lambda it: ei.time(a, b, n, m.Rule.mid, 0, n, it)}
            for every in EVERY:
                cap = m.expr_scan_outputs(0, n, every)
                sides[every] = (lambda it, every=every, cap=cap:
                                es.time(a, b, n, m.Rule.mid, 0, n, every, buf.data_ptr(), cap, it))
            its = {}
            for k, fn in sides.items():  # warm, calibrate, settle
                its[k] = iters_for(fn(3))
                settle(lambda: fn(3))
            ms = {k: [] for k in sides}
            for _ in range(REPS):
                for k, fn in sides.items():  # alternating
                    ms[k].append(fn(its[k]))
            two = 2 * statistics.median(ms["integrate"])
            for every in EVERY:
                med = statistics.median(ms[every])
                rec = {"case": "scan", "expr": expr, "n": n, "every": every,
                       "outputs": m.expr_scan_outputs(0, n, every), "iters": its[every],
                       "ms_per_scan": summary(ms[every]),
                       "integrate_ms": summary(ms["integrate"]),
                       "gb_per_s_stored": 8.0 * m.expr_scan_outputs(0, n, every) / (med * 1e6),
                       "ratio_to_two_integrations": med / two,
                       "ratio_to_one_integration": 2 * med / two,
                       "samples_per_s": n / (med * 1e-3)}
                print(json.dumps(rec), flush=True)
                out.append(rec)
            del buf
    return out


def torch_rows(m, torch, n):
    """torch.cumsum over a torch-evaluated sample tensor against the scan, every = 1."""
    out = []
    forms = {"4.0/(1.0+x*x)": lambda x: 4.0 / (1.0 + x * x), "exp(-x*x)": lambda x: torch.exp(-x * x)}
    for expr, a, b in CASES:
        h = (b - a) / n
        es = m.ExprScan(expr, 0)
        buf = torch.empty(n, dtype=torch.float64, device="cuda")

        def by_torch(it):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(it):
                x = a + (torch.arange(n, dtype=torch.float64, device="cuda") + 0.5) * h
                r = torch.cumsum(forms[expr](x), dim=0) * h
            e1.record()
            torch.cuda.synchronize()
            by_torch.last = r
            return e0.elapsed_time(e1) / it

        def by_scan(it):
            return es.time(a, b, n, m.Rule.mid, 0, n, 1, buf.data_ptr(), n, it)

        its = {}
        for name, fn in (("torch", by_torch), ("scan", by_scan)):
            its[name] = iters_for(fn(3))
            settle(lambda: fn(3))
        ms = {"torch": [], "scan": []}
        for _ in range(REPS):
            ms["torch"].append(by_torch(its["torch"]))
            ms["scan"].append(by_scan(its["scan"]))
        diff = float((by_torch.last - buf).abs().max() / by_torch.last[-1].abs())
        rec = {"case": "torch", "expr": expr, "n": n, "torch_ms": summary(ms["torch"]),
               "scan_ms": summary(ms["scan"]),
               "torch_over_scan": statistics.median(ms["torch"]) / statistics.median(ms["scan"]),
               "max_diff_rel_to_total": diff}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del buf
    return out


def markdown(recs) -> str:
    lines = ["# Running integral of a runtime integrand: ExprScan on one MI355X", "",
             "Written by `tools/expr_scan_probe.py` (device events, warmed, clocks settled, windows",
             "of at least 0.25 s, sides alternating, 3 repeats; spread = (max - min) / median).",
             "Midpoint rule. `2 x integrate` is two `ExprIntegrator.time` passes over the same n:",
             "the scan evaluates f for the tile sums and again wherever it writes.", "",
             "| expression | n | every | ms per scan | spread | GB/s stored | integrate ms | scan / (2 x integrate) | scan / integrate |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        if r["case"] == "scan":
            lines.append(f"| `{r['expr']}` | {r['n']:.0e} | {r['every']} | "
                         f"{r['ms_per_scan']['median']:.3f} | {r['ms_per_scan']['spread']:.3f} | "
                         f"{r['gb_per_s_stored']:.1f} | {r['integrate_ms']['median']:.3f} | "
                         f"{r['ratio_to_two_integrations']:.2f} | "
                         f"{r['ratio_to_one_integration']:.2f} |")
    lines += ["", "Against `torch.cumsum` over a torch-evaluated sample tensor (every = 1):", "",
              "| expression | n | torch ms | spread | scan ms | spread | torch / scan | max diff / total |",
              "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        if r["case"] == "torch":
            lines.append(f"| `{r['expr']}` | {r['n']:.0e} | {r['torch_ms']['median']:.3f} | "
                         f"{r['torch_ms']['spread']:.3f} | {r['scan_ms']['median']:.3f} | "
                         f"{r['scan_ms']['spread']:.3f} | {r['torch_over_scan']:.1f} | "
                         f"{r['max_diff_rel_to_total']:.1e} |")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", default="1e8,1e9")
    ap.add_argument("--torch-n", default="1e8")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    import torch

    from cuda_v_mpi_amd._native import native

    m = native()
    if m.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("expr_scan_probe: needs a HIP device")
    recs = scan_rows(m, torch, [int(float(s)) for s in a.n.split(",")])
    recs += torch_rows(m, torch, int(float(a.torch_n)))
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in recs)),
                       (a.md, markdown(recs))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
