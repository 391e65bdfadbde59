#!/usr/bin/env python3
"""Double integrals of a run-time expression: ExprIntegrator2D against the route there was
before it, ExprSweep with one parameter row per y sample (profiles/r16/expr2d.md).

Both integrate 4/(1 + x^2 + y^2) on [0, 1]^2 with the midpoint rule, N x N samples (default
32768: 2^30 samples; a sweep holds at most 2^20 rows, so N may not pass that). The
sweep route is f(x, p0) with the N y midpoints as rows, the rows' values summed on the host
and multiplied by hy. The two are timed in alternation, ROUNDS times each, after the clocks
have settled on the same work: device time (events around back-to-back launches) and end to
end (rows in to value out, host clock around the synchronous call). With --full also, for
scale: the 1-D expression at 2^30 samples, the two skinny rules at 2^30 samples, and what
hoisting an x-only factor is worth (exp(-x*x)*cos(x*y) against cos(x*y) alone and against
exp(-(x*x+y*y))).

    python tools/expr2d_probe.py --full [--n 32768] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def summary(v):
    return {"runs": [round(x, 4) for x in v], "median": statistics.median(v),
            "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def main() -> int:
    import numpy as np

    from cuda_v_mpi_amd._native import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    if m.device_count() < 1:
        raise SystemExit("expr2d_probe needs a HIP device")
    N, mid = a.n, m.Rule.mid
    hy = 1.0 / N
    params = np.ascontiguousarray(((np.arange(N) + 0.5) * hy).reshape(N, 1))
    es = m.ExprSweep("4.0/(1.0+x*x+p0*p0)", 1, 0, 0)
    ei = m.ExprIntegrator2D("4.0/(1.0+x*x+y*y)", 0, 0)
    out = {"n": N, "shape_2d": m.expr2d_shape(N, N, 0).as_tuple(),
           "shape_sweep": m.expr_sweep_shape(N, N, 0)}

    def sweep_value():
        return float(np.sum(es.integrate(params, 0.0, 1.0, N, mid, 0, N))) * hy

    def two_d_value():
        return ei.integrate(0.0, 1.0, N, 0.0, 1.0, N, mid, 0, N)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.5:   # settle the clocks on the timed work
        es.time(params, 0.0, 1.0, N, mid, 0, N, 5)
        ei.time(0.0, 1.0, N, 0.0, 1.0, N, mid, 0, N, 5)
    vs, v2 = sweep_value(), two_d_value()
    out.update(value_sweep=vs, value_2d=v2, rel_diff=abs(vs - v2) / abs(v2))
    dev_s, dev_2, e2e_s, e2e_2 = [], [], [], []
    for _ in range(a.rounds):
        dev_s.append(es.time(params, 0.0, 1.0, N, mid, 0, N, a.iters))
        dev_2.append(ei.time(0.0, 1.0, N, 0.0, 1.0, N, mid, 0, N, a.iters))
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(5):
            sweep_value()
        e2e_s.append((time.perf_counter() - t0) / 5 * 1e3)
        t0 = time.perf_counter()
        for _ in range(5):
            two_d_value()
        e2e_2.append((time.perf_counter() - t0) / 5 * 1e3)
    out.update(device_ms_sweep=summary(dev_s), device_ms_2d=summary(dev_2),
               e2e_ms_sweep=summary(e2e_s), e2e_ms_2d=summary(e2e_2),
               samples_per_s_sweep=N * N / (statistics.median(dev_s) * 1e-3),
               samples_per_s_2d=N * N / (statistics.median(dev_2) * 1e-3))
    if a.full:
        one = m.ExprIntegrator("4.0/(1.0+x*x)", 0)
        n1 = 1 << 30
        out["device_ms_1d_2^30"] = summary([one.time(0.0, 1.0, n1, mid, 0, n1, 10)
                                            for _ in range(5)])
        k = (1 << 30) // 3
        for name, (nx, ny) in (("skinny_x_3", (3, k)), ("skinny_y_3", (k, 3))):
            out["shape_" + name] = m.expr2d_shape(nx, ny, 0).as_tuple()
            out["device_ms_" + name] = summary(
                [ei.time(0.0, 1.0, nx, 0.0, 1.0, ny, mid, 0, ny, 10) for _ in range(5)])
        for name, e in (("gauss", "exp(-(x*x+y*y))"), ("exp_cos", "exp(-x*x)*cos(x*y)"),
                        ("cos_only", "cos(x*y)")):
            g = m.ExprIntegrator2D(e, 0, 0)
            out["device_ms_" + name] = summary(
                [g.time(0.0, 1.0, N, 0.0, 1.0, N, mid, 0, N, 5) for _ in range(5)])
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
