#!/usr/bin/env python3
"""Integrals over a box by a lattice rule: what ExprLattice costs and what it delivers
(profiles/r22/expr_lattice.md). No pass threshold.

  * device time and samples/s of exp(-(x0*x0 + ... )) on [0, 1]^d at d = 2, 6 and 16, m = 24 and
    64 shifts (2^30 samples), with the partials kernel's VGPRs and scratch from the code object;
  * the d = 2 row beside ExprIntegrator2D at the same sample count (a 32768 x 32768 midpoint rule
    of exp(-(x*x+y*y)): the route there was before, which forms x once per column), timed in
    alternation;
  * the d = 6 row beside the same points evaluated with torch on the GPU (the fractions, the tent,
    the coordinates and the sum as tensor operations, one shift at a time: the only way to that
    integral before);
  * the true error and err_est of the five truth cases of the tests at m = 12, 16, 20 and 24
    (16 shifts);
  * the rtol = 1e-8 walk of the six-dimensional Gaussian exp(-sum (x_j - 1/2)^2).

    python tools/expr_lattice_probe.py [--m 24] [--shifts 64] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def summary(v):
    return {"runs": [round(x, 4) for x in v], "median": statistics.median(v),
            "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def gauss(d: int) -> str:
    return "exp(-(" + "+".join(f"x{j}*x{j}" for j in range(d)) + "))"


def code_object_registers(code: bytes) -> dict:
    """vgpr_count, sgpr_count and the scratch bytes of miint_lattice_partials from the code
    object's metadata (llvm-readelf of the ROCm installation); empty when there is none."""
    tool = None
    for root in (os.environ.get("ROCM_PATH", "/opt/rocm"),):
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
        if not re.search(r"\.name:\s+miint_lattice_partials\b", block):
            continue
        for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                    "sgpr_spill_count"):
            hit = re.search(r"\." + key + r":\s+(\d+)", block)
            if hit:
                out[key] = int(hit.group(1))
    return out


TRUTHS = {
    "gauss6": ("exp(-(" + "+".join(f"(x{j}-0.5)*(x{j}-0.5)" for j in range(6)) + "))",
               [(0.0, 1.0)] * 6, 1, (math.sqrt(math.pi) * math.erf(0.5)) ** 6),
    "cos8": ("cos(" + "+".join(f"x{j}" for j in range(8)) + ")", [(0.0, 1.0)] * 8, 1,
             (complex(math.sin(1.0), 1.0 - math.cos(1.0)) ** 8).real),
    "exp16": ("exp((" + "+".join(f"x{j}" for j in range(16)) + ")/16.0)", [(0.0, 1.0)] * 16, 1,
              (16.0 * math.expm1(1.0 / 16.0)) ** 16),
    "ball3": ("(x0*x0+x1*x1+x2*x2<1.0)?1.0:0.0", [(-1.0, 1.0)] * 3, 1, 4.0 * math.pi / 3.0),
    "prod4": ("x0*x1*x2*x3", [(0.0, 2.0)] * 4, 0, 16.0),
}


def torch_route(m, box, z, words, periodic=False):
    """The rule's points and the Gaussian's sum as torch operations on the GPU, one shift at a
    time; returns the estimates."""
    import torch

    dev = torch.device("cuda", 0)
    n = 1 << m
    i = torch.arange(n, dtype=torch.int64, device=dev)[:, None]
    zz = torch.tensor(z, dtype=torch.int64, device=dev)[None, :]
    frac = ((i * zz) & (n - 1)) << (32 - m)
    lo = torch.tensor([p[0] for p in box], dtype=torch.float64, device=dev)
    width = torch.tensor([p[1] - p[0] for p in box], dtype=torch.float64, device=dev)
    est = []
    for row in words:
        u = (frac + torch.tensor([int(w) for w in row], dtype=torch.int64, device=dev)) & 0xFFFFFFFF
        if periodic:
            t = (2 * u + 1).to(torch.float64) * 2.0 ** -33
        else:
            w = torch.where(u >= 1 << 31, 0xFFFFFFFF - u, u)
            t = (2 * w + 1).to(torch.float64) * 2.0 ** -32
        x = t * width + lo
        est.append(torch.exp(-(x * x).sum(dim=1)).sum())
    vol = float(torch.prod(width))
    return [float(e) * vol / n for e in est]


def main() -> int:
    import numpy as np

    from cuda_v_mpi_amd._native import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=24)
    ap.add_argument("--shifts", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    mod = native()
    if mod.device_count() < 1:
        raise SystemExit("expr_lattice_probe needs a HIP device")
    import torch

    m, rows = a.m, a.shifts
    samples = rows << m
    opt = mod.LatticeOptions(shifts=rows)
    out = {"m": m, "shifts": rows, "samples": samples, "shape": mod.lattice_shape(1 << m, rows)}
    rules = {d: mod.ExprLattice(gauss(d), d) for d in (2, 6, 16)}
    boxes = {d: [(0.0, 1.0)] * d for d in rules}
    side = int(round(math.sqrt(samples)))
    two_d = mod.ExprIntegrator2D("exp(-(x*x+y*y))", 0, 0) if side * side == samples else None
    mid = mod.Rule.mid

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.5:   # settle the clocks on the timed work
        rules[6].time(boxes[6], m, opt, 0, None, 1)
    dev = {d: [] for d in rules}
    dev_2d = []
    for _ in range(a.rounds):               # in alternation
        for d, el in rules.items():
            dev[d].append(el.time(boxes[d], m, opt, 0, None, a.iters))
        if two_d:
            dev_2d.append(two_d.time(0.0, 1.0, side, 0.0, 1.0, side, mid, 0, side, a.iters))
    truth1 = math.sqrt(math.pi) / 2 * math.erf(1.0)
    for d, el in rules.items():
        r = el.integrate(boxes[d], m, opt)
        ms = statistics.median(dev[d])
        out[f"d{d}"] = {"expr": gauss(d), "device_ms": summary(dev[d]),
                        "samples_per_s": samples / (ms * 1e-3), "value": r.value,
                        "err_est": r.err_est, "abs_err": abs(r.value - truth1 ** d),
                        "registers": code_object_registers(mod.expr_lattice_compile(gauss(d), d))}
    if two_d:
        v = two_d.integrate(0.0, 1.0, side, 0.0, 1.0, side, mid, 0, side)
        ms2 = statistics.median(dev_2d)
        out["d2_tensor_rule"] = {"nx": side, "ny": side, "device_ms": summary(dev_2d),
                                 "samples_per_s": samples / (ms2 * 1e-3), "value": v,
                                 "abs_err": abs(v - truth1 ** 2),
                                 "lattice_over_tensor_time":
                                     statistics.median(dev[2]) / ms2}

    # d = 6 beside the torch evaluation of the same points
    z6 = [int(v) for v in mod.lattice_generator(m, 6)]
    words = np.asarray(mod.lattice_shifts(0, rows, 6))
    torch_route(m, boxes[6], z6, words[:1])           # warm
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        t0 = time.perf_counter()
        est = torch_route(m, boxes[6], z6, words)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    r6 = rules[6].integrate(boxes[6], m, opt)
    out["d6_torch_route"] = {"ms": summary(runs), "samples_per_s": samples / (min(runs) * 1e-3),
                             "value": sum(est) / rows,
                             "worst_rel_diff_of_an_estimate": float(np.max(
                                 np.abs(np.array(est) - r6.estimates) / np.abs(r6.estimates))),
                             "torch_over_lattice_time": min(runs) / statistics.median(dev[6])}

    # the truth cases
    out["truth_cases"] = {}
    for name, (expr, box, seed, truth) in TRUTHS.items():
        el = mod.ExprLattice(expr, len(box))
        rows_out = {}
        for lm in (12, 16, 20, 24):
            r = el.integrate(box, lm, mod.LatticeOptions(shifts=16, seed=seed))
            rows_out[str(lm)] = {"value": r.value, "err_est": r.err_est,
                                 "abs_err": abs(r.value - truth),
                                 "in_standard_errors": abs(r.value - truth) / r.err_est,
                                 "device_ms": r.device_ms}
        out["truth_cases"][name] = {"d": len(box), "truth": truth, "levels": rows_out}

    # the walk to rtol = 1e-8
    expr, box, seed, truth = TRUTHS["gauss6"]
    el = mod.ExprLattice(expr, 6)
    wopt = mod.LatticeOptions(shifts=16, seed=seed, rtol=1e-8)
    el.integrate_to(box, wopt)                         # warm
    walls, devs = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        r = el.integrate_to(box, wopt)
        walls.append((time.perf_counter() - t0) * 1e3)
        devs.append(r.device_ms)
    out["walk_gauss6_rtol_1e-8"] = {"value": r.value, "err_est": r.err_est, "m": r.m,
                                    "levels": r.levels, "evals": r.evals,
                                    "converged": r.converged, "abs_err": abs(r.value - truth),
                                    "wall_ms": summary(walls), "device_ms": summary(devs)}
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
