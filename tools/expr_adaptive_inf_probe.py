#!/usr/bin/env python3
"""Infinite and half-infinite ranges of the adaptive integrators (ExprAdaptive and
ExprAdaptiveSweep with `unbounded`) on one MI355X (profiles/r24/expr_adaptive_inf.md):

  * the cases of tests/expr_adaptive_inf_cases.py at rtol = 1e-10 from 65536 panels: device and
    end-to-end ms, rounds, evals, true error;
  * 4096-row sweeps of exp(-p0*x*x) and 1.0/((x-p0)*(x-p0)+p1) over the whole axis, the second
    also with lines of width 1e-3, which the rounding of the abscissa keeps from converging;
  * a round of the unbounded eval kernels beside the finite one on the same list length: calls
    that take one round from 65536 and 2^20 panels, where only the eval kernel differs;
  * the route before: the finite rule on [-L, L] with L picked by hand;
  * registers and scratch of the eval kernels, from the code objects.

Device time is events around back-to-back calls (the `time` methods: the rounds' syncs and the
host's reads are inside), end to end a host clock around synchronous calls. Whatever is compared
alternates, ROUNDS times each, after the clocks have settled on the same work; a figure is the
median of the rounds, the spread max - min.

    python tools/expr_adaptive_inf_probe.py [--md profiles/r24/expr_adaptive_inf.md] [--out FILE.json]
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
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

RTOL = 1e-10
INF = float("inf")
REGISTER_EXPRS = ("exp(-x*x)", "1.0/((x-p0)*(x-p0)+p1)", "x*x*x/expm1(x)")


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def settle(work, seconds=0.5):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        work()


def timed(calls: dict, rounds: int, iters: int) -> dict:
    """calls: name -> (device_ms(iters), run()). Alternates the names, `rounds` times each."""
    settle(lambda: [c[0](2) for c in calls.values()])
    dev = {k: [] for k in calls}
    e2e = {k: [] for k in calls}
    for _ in range(rounds):
        for k, (device_ms, run) in calls.items():
            dev[k].append(device_ms(iters))
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            e2e[k].append((time.perf_counter() - t0) / iters * 1e3)
    return {k: {"device_ms": med(dev[k]), "device_spread": spread(dev[k]),
                "e2e_ms": med(e2e[k]), "e2e_spread": spread(e2e[k])} for k in calls}


def main() -> int:
    import numpy as np

    import expr_adaptive_inf_cases as ic
    from cuda_v_mpi_amd._native import native
    from expr_adaptive_sweep_probe import code_object_registers

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--md", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = native()
    if m.device_count() < 1:
        raise SystemExit("expr_adaptive_inf_probe needs a HIP device")
    out = {"rtol": RTOL, "rounds_of_timing": a.rounds, "iters": a.iters}

    # 1. the table from the default 65536 panels
    opt = m.AdaptOptions(rtol=RTOL, unbounded=True)
    table = []
    for case in ic.TABLE:
        ea = m.ExprAdaptive(case.expr, 0)
        r = ea.integrate(case.a, case.b, opt)
        t = timed({"call": (lambda n, ea=ea, c=case: ea.time(c.a, c.b, opt, n),
                            lambda ea=ea, c=case: ea.integrate(c.a, c.b, opt))},
                  a.rounds, a.iters)["call"]
        table.append(dict(t, case=case.name, expr=case.expr, a=case.a, b=case.b, range=r.range,
                          rounds=r.rounds, evals=r.evals, converged=r.converged, floor=r.floor,
                          forced=r.forced, abs_err=abs(r.value - case.truth),
                          bound=ic.value_bound(r, case), tol=r.tol))
        del ea
    out["table"] = table

    # 2. 4096-row sweeps over the whole axis
    k = 4096
    sweeps = []
    lorentz = "1.0/((x-p0)*(x-p0)+p1)"
    centres = np.linspace(-5.0, 5.0, k)
    families = [
        ("exp(-p0*x*x)", "p0 = 1e-2 .. 1e2", np.logspace(-2, 2, k).reshape(k, 1),
         lambda p: np.sqrt(np.pi / p[:, 0])),
        (lorentz, "p0 = -5 .. 5, p1 = 1e-2, 1e-4, 1",
         np.stack([centres, np.resize([1e-2, 1e-4, 1.0], k)], axis=1),
         lambda p: np.pi / np.sqrt(p[:, 1])),
        # lines of width 1e-3 up to 5 away from the origin: past what the abscissa's rounding
        # lets the rule resolve (the note says why)
        (lorentz, "p0 = -5 .. 5, p1 = 1e-2, 1e-4, 1, 1e-6",
         np.stack([centres, np.resize([1e-2, 1e-4, 1.0, 1e-6], k)], axis=1),
         lambda p: np.pi / np.sqrt(p[:, 1]))]
    sopt = m.AdaptSweepOptions(rtol=RTOL, unbounded=True)
    for expr, rows, params, truth in families:
        es = m.ExprAdaptiveSweep(expr, params.shape[1], 0)
        r = es.integrate(params, -INF, INF, sopt)
        t = timed({"call": (lambda n, es=es, p=params: es.time(p, -INF, INF, sopt, n),
                            lambda es=es, p=params: es.integrate(p, -INF, INF, sopt))},
                  a.rounds, max(2, a.iters // 2))["call"]
        rel = np.abs(r.value - truth(params)) / truth(params)
        sweeps.append(dict(t, expr=expr, parameters=rows, rows=k, call_rounds=r.call_rounds,
                           call_evals=r.call_evals, peak=r.peak,
                           converged=int(r.converged.sum()), capped=int(r.capped.sum()),
                           max_rel_err=float(rel.max())))
        del es
    out["sweeps"] = sweeps

    # 3. one round, finite beside unbounded, on the same list length (atol large: one round)
    one_round = []
    for expr, fin in (("exp(-x*x)", (0.0, 6.0)), ("1.0/(1.0+x*x)", (0.0, 6.0)),
                      ("x*x*x/expm1(x)", (0.5, 6.0))):
        ea = m.ExprAdaptive(expr, 0)
        for panels in (65536, 1 << 20):
            o = m.AdaptOptions(rtol=0.0, atol=1e300, panels=panels, unbounded=True)
            ranges = {"finite": fin, "upper": (fin[0], INF), "lower": (-INF, -fin[0]),
                      "both": (-INF, INF)}
            if "expm1" in expr:
                del ranges["lower"], ranges["both"]     # 0/0 at x = 0, overflow below
            calls = {kind: (lambda n, ab=ab: ea.time(ab[0], ab[1], o, n),
                            lambda ab=ab: ea.integrate(ab[0], ab[1], o))
                     for kind, ab in ranges.items()}
            for kind, ab in ranges.items():
                assert ea.integrate(ab[0], ab[1], o).rounds == 1
            t = timed(calls, a.rounds, a.iters)
            for kind, v in t.items():
                one_round.append(dict(v, expr=expr, panels=panels, kind=kind,
                                      extra_us=(v["device_ms"] - t["finite"]["device_ms"]) * 1e3,
                                      extra_ns_per_node=(v["device_ms"] - t["finite"]["device_ms"])
                                      * 1e6 / (15 * panels)))
        del ea
    out["one_round"] = one_round

    # 4. the route before: the finite rule on [-L, L], L by hand
    before = []
    fopt = m.AdaptOptions(rtol=RTOL)
    for expr, truth, ls in (("exp(-x*x)", math.sqrt(math.pi), (6.0,)),
                            ("1.0/(1.0+x*x)", math.pi, (1e2, 1e4, 1e6, 1e8, 1e10))):
        ea = m.ExprAdaptive(expr, 0)
        calls = {"inf": (lambda n: ea.time(-INF, INF, opt, n),
                         lambda: ea.integrate(-INF, INF, opt))}
        for big in ls:
            calls[f"L={big:g}"] = (lambda n, big=big: ea.time(-big, big, fopt, n),
                                   lambda big=big: ea.integrate(-big, big, fopt))
        t = timed(calls, a.rounds, a.iters)
        for name, v in t.items():
            ab = (-INF, INF) if name == "inf" else (-float(name[2:]), float(name[2:]))
            r = ea.integrate(ab[0], ab[1], opt if name == "inf" else fopt)
            before.append(dict(v, expr=expr, route=name, rounds=r.rounds, evals=r.evals,
                               converged=r.converged, abs_err=abs(r.value - truth),
                               tol=RTOL * truth))
        del ea
    out["before"] = before

    # 5. registers and scratch, each integrand alone and with 8 parameters
    regs = []
    for expr in REGISTER_EXPRS:
        alone = expr.replace("p0", "3.0").replace("p1", "1e-6")
        objs = {"ExprAdaptive": (m.expr_adapt_compile(alone), m.expr_adapt_unbounded_compile(alone)),
                "ExprAdaptiveSweep, 8 parameters": (m.expr_adapt_sweep_compile(expr, 8),
                                                    m.expr_adapt_sweep_unbounded_compile(expr, 8))}
        for where, codes in objs.items():
            for code in codes:
                for name, r in code_object_registers(code).items():
                    if "_eval" in name:
                        regs.append(dict(r, expr=expr, where=where, kernel=name))
    out["registers"] = regs

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
    def ms(r):
        return (f"{r['device_ms']:.4f} ({r['device_spread']:.4f}) | {r['e2e_ms']:.4f} "
                f"({r['e2e_spread']:.4f})")

    def ends(r):
        return f"({r['a']:g}, {r['b']:g})"

    ls = ["# Infinite and half-infinite ranges of the adaptive integrators (r24)", "",
          f"One MI355X, `tools/expr_adaptive_inf_probe.py`, one process, rtol = {out['rtol']:g}. "
          f"Device time is events around {out['iters']} back-to-back calls (the rounds' syncs and "
          "the host's reads are inside), end to end a host clock around the same number of "
          f"synchronous calls. What is compared alternates, {out['rounds_of_timing']} rounds "
          "each, after 0.5 s of the same work; a figure is the median of the rounds, the spread "
          "max - min.", "",
          "## The cases of tests/expr_adaptive_inf_cases.py from 65536 panels", "",
          "| integrand | range | kind | rounds | evals | floor / forced | true error | bound | "
          "converged | device ms (spread) | end to end ms (spread) |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["table"]:
        ls.append(f"| `{r['expr']}` | {ends(r)} | {r['range']} | {r['rounds']} | {r['evals']} | "
                  f"{r['floor']} / {r['forced']} | {r['abs_err']:.1e} | {r['bound']:.1e} | "
                  f"{'yes' if r['converged'] else 'no'} | {ms(r)} |")
    ls += ["", "## Sweeps of 4096 rows over (-inf, inf)", "",
           "| family | rows | rounds | evals | longest list | rows converged | rows capped | "
           "largest relative error | device ms (spread) | end to end ms (spread) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["sweeps"]:
        ls.append(f"| `{r['expr']}` | {r['parameters']} | {r['call_rounds']} | {r['call_evals']} | "
                  f"{r['peak']} | {r['converged']} of {r['rows']} | {r['capped']} | "
                  f"{r['max_rel_err']:.1e} | {ms(r)} |")
    ls += ["", "## One round: the unbounded eval kernels beside the finite one", "",
           "Calls that take exactly one round (atol = 1e300), so the six launches and the sync are "
           "the same and only the eval kernel differs; `extra` is the device time above the finite "
           "call on the same list length, also per node (15 per interval; `both` evaluates f twice "
           "per node).", "",
           "| integrand | panels | kind | device ms (spread) | end to end ms (spread) | extra us | "
           "extra ns / node |", "|---|---|---|---|---|---|---|"]
    for r in out["one_round"]:
        ls.append(f"| `{r['expr']}` | {r['panels']} | {r['kind']} | {ms(r)} | "
                  f"{r['extra_us']:.1f} | {r['extra_ns_per_node']:.4f} |")
    ls += ["", "## The route before: the finite rule on [-L, L], L by hand", "",
           "| integrand | route | rounds | evals | true error | tol | converged | device ms "
           "(spread) | end to end ms (spread) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in out["before"]:
        route = "(-inf, inf)" if r["route"] == "inf" else f"[-L, L], {r['route']}"
        ls.append(f"| `{r['expr']}` | {route} | {r['rounds']} | {r['evals']} | "
                  f"{r['abs_err']:.1e} | {r['tol']:.1e} | {'yes' if r['converged'] else 'no'} | "
                  f"{ms(r)} |")
    ls += ["", "## Registers and scratch of the eval kernels", "",
           "From the code objects' metadata; the expressions with p0, p1 are compiled alone with "
           "3.0 and 1e-6 in their place.", "",
           "| integrand | where | kernel | VGPRs | SGPRs | scratch bytes | spilled VGPRs |",
           "|---|---|---|---|---|---|---|"]
    for r in out["registers"]:
        ls.append(f"| `{r['expr']}` | {r['where']} | {r['kernel']} | {r.get('vgpr_count')} | "
                  f"{r.get('sgpr_count')} | {r.get('private_segment_fixed_size')} | "
                  f"{r.get('vgpr_spill_count')} |")
    return "\n".join(ls) + "\n"


if __name__ == "__main__":
    sys.exit(main())
