#!/usr/bin/env python3
"""Parameter sweeps of a runtime integrand (ExprSweep) against the one-integral-per-call path
(ExprIntegrator), on one GPU, one process (profiles/r8/expr_sweep.md):

  shape   the launch-shape table: S samples per lane per workgroup in {16, 64, 256, 1024}
          (gx = ceil(n / (256 S)) given as an explicit grid) at n = 1e6, K = 4096 and
          n = 1e9, K = 8, and at n = 1e7, K = 8 (few rows, where gy cannot make up for a
          small gx); device ms per sweep
  large   n = 1e9, K = 8: the sweep's device time per row against ExprIntegrator.time per
          integration (the literal-substituted expression of each row)
  small   n = 1e6, K = 4096 and n = 1e4, K = 65536: the sweep per row against K back-to-back
          ExprIntegrator integrations (time()) and K synchronous integrate() calls. A
          baseline row's cost does not depend on the parameter's value, so the K baseline
          integrations cycle over 8 compiled literal expressions instead of compiling K
  compile host wall-clock of one expr_sweep_compile (three fresh expressions)

Every timing: device events (time()) or a host clock around synchronous calls, each shape
warmed first, windows of at least 0.2 s, the two sides alternating, three repeats; the
spread is (max - min) / median of the repeats.

  python tools/expr_sweep_probe.py [--only shape,large,small,compile] [--out FILE]
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


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def summary(v):
    return {"median": statistics.median(v), "spread": spread(v), "reps": v}


def iters_for(ms_one: float) -> int:
    return max(3, int(math.ceil(WINDOW_S * 1e3 / max(ms_one, 1e-3))))


def lin(lo, hi, k):
    import numpy as np

    return np.linspace(lo, hi, k).reshape(k, 1)


def sweep_ms(m, es, rows, a, b, n, iters=None):
    """Device ms per sweep; iters from a short calibration unless given."""
    if iters is None:
        iters = iters_for(es.time(rows, a, b, n, m.Rule.mid, 0, n, 3))
    return es.time(rows, a, b, n, m.Rule.mid, 0, n, iters), iters


def shape_table(m):
    out = []
    for n, k, expr, a, b in ((10**6, 4096, "exp(-p0*x*x)", 0.0, 2.0),
                            (10**9, 8, "4.0/(1.0+p0*x*x)", 0.0, 1.0),
                            # few rows of a middling size: where a large S starves the device
                            (10**7, 8, "exp(-p0*x*x)", 0.0, 2.0)):
        rows = lin(0.5, 4.0, k)
        sweeps = {}
        for s in (16, 64, 256, 1024):
            gx = min(max(-(-n // (256 * s)), 1), 2048)
            sweeps[s] = (m.ExprSweep(expr, 1, 0, gx), gx)
        its = {s: sweep_ms(m, es, rows, a, b, n)[1] for s, (es, _) in sweeps.items()}  # warm
        ms = {s: [] for s in sweeps}
        for _ in range(REPS):
            for s, (es, _) in sweeps.items():  # alternating
                ms[s].append(sweep_ms(m, es, rows, a, b, n, its[s])[0])
        for s, (es, gx) in sweeps.items():
            gy = m.expr_sweep_shape(n, k, gx)[1]
            rec = {"case": "shape", "n": n, "rows": k, "S": s, "gx": gx, "gy": gy,
                   "iters": its[s], "ms_per_sweep": summary(ms[s]),
                   "us_per_row": statistics.median(ms[s]) * 1e3 / k}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def literal(expr: str, p: float) -> str:
    return expr.replace("p0", repr(float(p)))


def large_rows(m):
    n, k, expr, a, b = 10**9, 8, "4.0/(1.0+p0*x*x)", 0.0, 1.0
    rows = lin(0.5, 4.0, k)
    es = m.ExprSweep(expr, 1, 0)
    base = [m.ExprIntegrator(literal(expr, r[0]), 0) for r in rows]
    one = base[0].time(a, b, n, m.Rule.mid, 0, n, 3)
    it_b = max(3, iters_for(one * k))
    _, it_s = sweep_ms(m, es, rows, a, b, n)
    for e in base:
        e.time(a, b, n, m.Rule.mid, 0, n, 3)  # warm every module
    b_ms, s_ms = [], []
    for _ in range(REPS):
        b_ms.append(sum(e.time(a, b, n, m.Rule.mid, 0, n, it_b) for e in base) / k)
        s_ms.append(sweep_ms(m, es, rows, a, b, n, it_s)[0] / k)
    vals = es.integrate(rows, a, b, n, m.Rule.mid, 0, n)
    want = [e.integrate(a, b, n, m.Rule.mid, 0, n) for e in base]
    rec = {"case": "large", "n": n, "rows": k, "shape": m.expr_sweep_shape(n, k),
           "baseline_ms_per_integration": summary(b_ms), "sweep_ms_per_row": summary(s_ms),
           "sweep_over_baseline": statistics.median(s_ms) / statistics.median(b_ms),
           "max_rel_diff": max(abs(v - w) / abs(w) for v, w in zip(vals, want)),
           "subintervals_per_s": n / (statistics.median(s_ms) * 1e-3)}
    print(json.dumps(rec), flush=True)
    return [rec]


def small_rows(m):
    out = []
    expr, a, b = "exp(-p0*x*x)", 0.0, 2.0
    base = [m.ExprIntegrator(literal(expr, 0.5 + 0.5 * j), 0) for j in range(8)]
    es = m.ExprSweep(expr, 1, 0)
    for n, k in ((10**6, 4096), (10**4, 65536)):
        rows = lin(0.5, 4.0, k)
        for e in base:
            e.time(a, b, n, m.Rule.mid, 0, n, 50)
            e.integrate(a, b, n, m.Rule.mid, 0, n)
        _, it_s = sweep_ms(m, es, rows, a, b, n)
        es.integrate(rows, a, b, n, m.Rule.mid, 0, n)
        bt, bs, st, ss = [], [], [], []
        for _ in range(REPS):
            # K back-to-back integrations, device events (K / 8 per compiled literal)
            bt.append(sum(e.time(a, b, n, m.Rule.mid, 0, n, k // 8) * (k // 8) for e in base)
                      * 1e3 / k)
            st.append(sweep_ms(m, es, rows, a, b, n, it_s)[0] * 1e3 / k)
            t0 = time.perf_counter()  # K synchronous calls, host clock
            for i in range(k):
                base[i & 7].integrate(a, b, n, m.Rule.mid, 0, n)
            bs.append((time.perf_counter() - t0) * 1e6 / k)
            reps = max(1, int(WINDOW_S / max(st[-1] * 1e-6 * k, 1e-4)))
            t0 = time.perf_counter()  # the sweep's synchronous call: upload .. values
            for _ in range(reps):
                es.integrate(rows, a, b, n, m.Rule.mid, 0, n)
            ss.append((time.perf_counter() - t0) * 1e6 / (k * reps))
        rec = {"case": "small", "n": n, "rows": k, "shape": m.expr_sweep_shape(n, k),
               "baseline_time_us_per_row": summary(bt), "baseline_integrate_us_per_row": summary(bs),
               "sweep_time_us_per_row": summary(st), "sweep_integrate_us_per_row": summary(ss),
               "ratio_time": statistics.median(bt) / statistics.median(st),
               "ratio_integrate": statistics.median(bs) / statistics.median(ss),
               "subintervals_per_s": n / (statistics.median(st) * 1e-6)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def compile_time(m):
    ts = []
    for j in range(REPS):
        t0 = time.perf_counter()
        m.expr_sweep_compile(f"exp(-p0*x*x) + {j + 1}.5*p1", 2)
        ts.append(time.perf_counter() - t0)
    rec = {"case": "compile", "seconds": summary(ts)}
    print(json.dumps(rec), flush=True)
    return [rec]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", default="compile,shape,large,small")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from cuda_v_mpi_amd._native import native

    m = native()
    only = a.only.split(",")
    if m.device_count() < 1 and only != ["compile"]:
        raise SystemExit("expr_sweep_probe: needs a HIP device (only `--only compile` does not)")
    recs = []
    for name, fn in (("compile", compile_time), ("shape", shape_table), ("large", large_rows),
                     ("small", small_rows)):
        if name in only:
            recs += fn(m)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
