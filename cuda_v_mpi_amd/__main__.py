"""Python command line: ``python -m cuda_v_mpi_amd <command> [flags]``.

Mirrors the native tools in build/bin (same stdout contract as the reference programs,
SURVEY §2.6) on top of the Python API, and adds JSON output:

    riemann     sin on [0, pi], N = 1e9 (riemann.cpp)          [--integrand pi4 --n 1e9 ...]
    cintegrate  train distance from the profile (cintegrate.cu)  [--parity --sp 32 --sm 2]
    trainscan   two-phase prefix scan (4main.c)                   [--parity --algo lookback]
    integrate   any integrand, JSON result                        [--integrand --n --rule ...]
                or any f(x):  --expr "exp(-x*x)" --a 0 --b 3 (compiled at run time, hipRTC)
                or to a tolerance: --expr "1.0/sqrt(x)" --a 0 --b 1 --rtol 1e-10
                or over a box: --expr "exp(-(x0*x0+x1*x1+x2*x2))" --box 0:1,0:1,0:3 --m 20
    table2d     2-D velocity field v(x) v(y), bilinear, JSON      [--grid 4096 --iters 100]
    oracle      print every SURVEY §6.1 oracle value (CPU only)
    scale       GPU-count sweep 1,2,4,8: weak/strong efficiency, RCCL latency [--gpus 1,2,4,8]
    compare     the reference's CUDA-vs-MPI comparison, measured here: the same integral on
                the MI355X and on this host's cores (host engine; for sin also the reference's
                own scalar MPI program on threads)        [--integrand sin --n 1e9 --ranks 8]
    info        devices and build

Multi-GPU: launch under torchrun (one process per GPU); the process group is created from
the environment and partial sums are reduced with RCCL.
"""
from __future__ import annotations

import argparse
import json
import math
import sys

from .utils import output


def _elapsed() -> float:
    """Seconds since this process started (the reference starts its clock first thing in
    main(), before MPI_Init / context creation: riemann.cpp:51, cintegrate.cu:104)."""
    import time

    import psutil

    return time.time() - psutil.Process().create_time()


def _ctx(backend=None):
    """Process group for the ranks (torchrun env). GPU runs reduce through the native RCCL
    communicator, so their torch group is the gloo control plane (one RCCL communicator per
    rank); host/cpu backends reduce over gloo itself."""
    from .parallel import dist as mdist

    return mdist.init(backend=backend or mdist.control_backend("native"))


def cmd_riemann(a) -> int:
    from . import Integrator

    ctx = _ctx("gloo" if a.backend in ("cpu", "host") else None)
    spec_b = {"sin": math.pi, "pi4": 1.0}.get(a.integrand, None)
    it = Integrator(a.integrand, n=int(a.n), rule=a.rule, dtype=a.dtype, div=a.div, ctx=ctx,
                    backend=a.backend, block=a.block)
    r = it.run()
    if ctx.is_root:
        print(output.fmt_seconds(_elapsed()))
        print(output.fmt_riemann_result(spec_b if spec_b is not None else it.spec.b, a.n, r.value))
        if a.json:
            print(json.dumps(r.as_dict()))
    ctx.destroy()
    return 0


def cmd_cintegrate(a) -> int:
    from . import Integrator
    from .parallel.decomposition import coverage_seconds

    ctx = _ctx("gloo" if a.backend in ("cpu", "host") else None)
    seconds = coverage_seconds(a.sp * a.sm) if a.parity else 1800
    it = Integrator("table", n=seconds * 10000, rule="left", b=float(seconds), ctx=ctx,
                    backend=a.backend)
    r = it.run()
    if ctx.is_root:
        print(output.fmt_seconds(_elapsed()))
        print(output.fmt_cintegrate_distance(r.value))
        if a.json:
            print(json.dumps(r.as_dict()))
    ctx.destroy()
    return 0


def cmd_trainscan(a) -> int:
    from ._native import native
    from .parallel.dist import native_comm

    ctx = _ctx()
    m = native()
    cfg = m.TrainScanConfig()
    cfg.parity, cfg.algo = a.parity, a.algo
    comm = native_comm(ctx) if ctx.world > 1 else None
    if ctx.is_root:
        print(output.fmt_step_size(cfg.steps_per_sec))
    r = m.TrainScan(cfg, ctx.device, comm).run()
    if ctx.is_root:
        print(output.fmt_seconds(_elapsed()))
        print(output.fmt_total_distance(r["distance"]))
        if a.json:
            print(json.dumps(r))
    ctx.destroy()
    return 0


def cmd_compare(a) -> int:
    """The reference is a CUDA-vs-MPI comparison (its name; riemann.cpp vs cintegrate.cu):
    one JSON row per side, measured in this process, plus the ratio."""
    import time

    from . import Integrator
    from ._native import native

    m = native()
    n = int(a.n)
    rows = []

    def timed(fn, reps):
        fn()  # warm: threads, code, clocks
        best, v = float("inf"), None
        for _ in range(reps):
            t = time.perf_counter()
            v = fn()
            best = min(best, time.perf_counter() - t)
        return v, best

    if a.expr:  # any f(x): compiled for the host cores and, below, with hipRTC for gfx950
        lo = 0.0 if a.a is None else a.a
        hi = 1.0 if a.b is None else a.b
        pool = m.HostPool(a.threads)
        he = m.HostExpr(a.expr)
        rl = getattr(m.Rule, a.rule)
        v, s = timed(lambda: he.integrate(lo, hi, n, rl, 0, n, pool), a.reps)
        rows.append({"side": "host", "what": f"{a.expr} compiled for the host, "
                     f"{pool.threads} threads, scalar libm per sample", "value": v,
                     "seconds": s, "subintervals_per_s": n / s})
    else:
        host = Integrator(a.integrand, n=n, rule=a.rule, backend="host", threads=a.threads)
        v, s = timed(lambda: host.run().value, a.reps)
        rows.append({"side": "host", "what": f"host engine, {host._pool.threads} threads, "
                     f"{m.host_isa()}, per-sample fp64", "value": v,
                     "abs_err": abs(v - host.spec.analytic()), "seconds": s,
                     "subintervals_per_s": n / s})
    if a.integrand == "sin" and a.rule == "left" and not a.expr:
        pool = m.HostPool(a.threads)
        v, s = timed(lambda: m.host_riemann_mpi_parity(a.ranks, float(n), math.pi, pool), 1)
        rows.append({"side": "reference-program", "what": f"riemann.cpp as mpirun -np {a.ranks} "
                     f"runs it ({a.ranks - 1} workers on threads, scalar libm sin)", "value": v,
                     "abs_err": abs(v - 2.0), "seconds": s, "subintervals_per_s": n / s})
    if m.device_count() > 0 and a.expr:
        ei = m.ExprIntegrator(a.expr, 0)
        rl = getattr(m.Rule, a.rule)
        v = ei.integrate(lo, hi, n, rl, 0, n)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.06:  # clock settle
            ei.time(lo, hi, n, rl, 0, n, 4)
        s = ei.time(lo, hi, n, rl, 0, n, a.steps) * 1e-3
        rows.append({"side": "gpu", "what": f"{a.expr} compiled with hipRTC for gfx950",
                     "value": v, "seconds": s, "subintervals_per_s": n / s})
    elif m.device_count() > 0:
        gpu = Integrator(a.integrand, n=n, rule=a.rule)
        gpu.plan.prepare_steps(a.steps)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.06:  # clock settle, as bench.py (--settle-ms)
            gpu.run_steps(a.steps)
        t = gpu.run_steps(a.steps)
        v = gpu.plan.host_result(gpu.plan.host_index_of(a.steps - 1, True))
        s = t["device_ms"] * 1e-3 / a.steps
        rows.append({"side": "gpu", "what": f"MI355X HIP kernels, hipGraph batches of {a.steps}",
                     "value": v, "abs_err": abs(v - gpu.spec.analytic()), "seconds": s,
                     "subintervals_per_s": n / s})
    else:
        rows.append({"side": "gpu", "skipped": "no HIP device visible"})
    rate = {r["side"]: r.get("subintervals_per_s") for r in rows}
    for r in rows:
        print(json.dumps(r))
    if rate.get("gpu") and rate.get("host"):
        print(json.dumps({"speedup_gpu_vs_host": rate["gpu"] / rate["host"],
                          "speedup_gpu_vs_reference_program":
                          rate["gpu"] / rate["reference-program"]
                          if rate.get("reference-program") else None}))
    return 0


_INFINITIES = ("inf", "+inf", "-inf", "infinity", "+infinity", "-infinity")


def _join_infinities(argv: list) -> list:
    """``--a -inf`` as ``--a=-inf``: argparse takes a value that starts with a dash and is no
    plain number for an option of its own."""
    out, i = [], 0
    while i < len(argv):
        if (argv[i] in ("--a", "--b") and i + 1 < len(argv)
                and argv[i + 1].lower() in _INFINITIES):
            out.append(f"{argv[i]}={argv[i + 1]}")
            i += 2
        else:
            out.append(argv[i])
            i += 1
    return out


def _json_ends(rec: dict) -> dict:
    """An infinite a or b as the string "inf" / "-inf": json has no number for it."""
    import math

    for k in ("a", "b"):
        if isinstance(rec.get(k), float) and math.isinf(rec[k]):
            rec[k] = "inf" if rec[k] > 0 else "-inf"
    return rec


def cmd_integrate(a) -> int:
    from . import Integrator

    if (a.curve_rtol is not None or a.curve_atol is not None or a.points is not None
            or a.at):
        return _integrate_curve(a)
    if a.ranges and a.row_rtol is None and a.row_atol is None:
        raise SystemExit("integrate: --ranges gives the rows of a sweep to a tolerance their own "
                         "ranges: it needs --row-rtol R / --row-atol T")
    if a.osc is not None or a.omega is not None or a.max_cycles is not None:
        return _integrate_osc(a)
    for flag, v in (("--a", a.a), ("--b", a.b)):
        if (v is not None and v in (float("inf"), float("-inf"))
                and not (a.expr and not a.box and any(t is not None for t in (
                    a.rtol, a.atol, a.row_rtol, a.row_atol)))):
            raise SystemExit(f"integrate: {flag} {v}: an infinite range needs --expr with --rtol / "
                             "--atol or --row-rtol / --row-atol (the fixed rules and --box have no "
                             "such range)")
    if a.expr:  # any f(x): compiled at run time with hipRTC (ops.kernels.riemann_expr)
        from .ops import kernels

        lo = 0.0 if a.a is None else a.a
        hi = 1.0 if a.b is None else a.b
        if a.area_rtol is not None or a.area_atol is not None:
            return _integrate_adaptive2d(a, lo, hi)
        if a.y_lo is not None or a.y_hi is not None:
            raise SystemExit("integrate: --y-lo / --y-hi are the limits of a double integral to a "
                             "tolerance: they need --area-rtol R / --area-atol T (the fixed rule "
                             "has no such region)")
        if a.panels_y is not None:
            raise SystemExit("integrate: --panels-y belongs to --area-rtol / --area-atol")
        if a.row_rtol is not None or a.row_atol is not None:
            return _integrate_adaptive_sweep(a, lo, hi)
        if a.max_total is not None:
            raise SystemExit("integrate: --max-total belongs to --row-rtol / --row-atol")
        if a.box:
            return _integrate_lattice(a)
        _no_lattice_flags(a)
        if a.rtol is not None or a.atol is not None:
            return _integrate_adaptive(a, lo, hi)
        if a.panels is not None or a.max_depth is not None or a.max_intervals is not None:
            raise SystemExit("integrate: --panels / --max-depth / --max-intervals belong to "
                             "--rtol / --atol")
        a.n = 1e9 if a.n is None else a.n
        a.rule = a.rule or "left"
        if (a.ya is None) != (a.yb is None):
            raise SystemExit("integrate: --ya and --yb go together (the y interval of a double "
                             "integral)")
        if a.ny is not None and a.ya is None:
            raise SystemExit("integrate: --ny belongs to a double integral (--ya AY --yb BY)")
        if a.ya is not None:  # f(x, y) on [a, b] x [ya, yb]: n x ny samples
            from . import integrate_expr2d

            if a.params or a.linspace:
                raise SystemExit("integrate: a double integral takes no --params / --linspace")
            on_host = a.backend == "host" or a.device == "cpu"
            ny = int(a.n) if a.ny is None else int(a.ny)
            r = integrate_expr2d(a.expr, lo, hi, a.ya, a.yb, int(a.n), ny, rule=a.rule,
                                 backend="host" if on_host else "hip", analytic=a.analytic)
            rec = {"expr": a.expr, "a": lo, "b": hi, "ya": a.ya, "yb": a.yb, "n": int(a.n),
                   "ny": ny, "rule": a.rule, "value": r.value,
                   "ms_per_integration": r.seconds_device * 1e3,
                   "samples_per_s": r.subintervals_per_s}
            if a.analytic is not None:
                rec.update(analytic=a.analytic, abs_err=r.abs_err)
            print(json.dumps(rec))
            return 0
        if a.params or a.linspace:  # a parameter sweep: f(x, p0..p7), K rows per launch
            from . import integrate_expr_sweep
            from ._native import native

            if a.params and a.linspace:
                raise SystemExit("integrate: give --params FILE or --linspace, not both")
            m = native()
            on_host = a.backend == "host" or a.device == "cpu"
            rows = m.load_param_rows(a.params) if a.params else m.linspace_param_rows(a.linspace)
            r = integrate_expr_sweep(a.expr, rows, lo, hi, n=int(a.n), rule=a.rule,
                                     backend="host" if on_host else "hip")
            if a.json:
                rec = {"expr": a.expr, "a": lo, "b": hi, "n": int(a.n), "rule": a.rule,
                       "rows": r.rows, "nparams": r.nparams, "values": r.values,
                       "ms_per_sweep": r.seconds * 1e3,
                       "subintervals_per_s": r.subintervals_per_s}
                print(json.dumps(rec))
            else:
                for k, (row, v) in enumerate(zip(rows, r.values)):
                    print(k, " ".join(f"{p:.17g}" for p in row), f"{v:.13g}")
            return 0
        v = kernels.riemann_expr(a.expr, lo, hi, int(a.n), rule=a.rule)
        rec = {"expr": a.expr, "a": lo, "b": hi, "n": int(a.n), "rule": a.rule, "value": v}
        if a.analytic is not None:
            rec.update(analytic=a.analytic, abs_err=abs(v - a.analytic))
        print(json.dumps(rec))
        return 0

    if a.box:
        raise SystemExit("integrate: --box is the box of an --expr integrand over x0, x1, ...")
    _no_lattice_flags(a)
    if a.y_lo is not None or a.y_hi is not None:
        raise SystemExit("integrate: --y-lo / --y-hi are the limits in y of an --expr double "
                         "integral")
    if a.area_rtol is not None or a.area_atol is not None or a.panels_y is not None:
        raise SystemExit("integrate: --area-rtol / --area-atol are the tolerance of an --expr "
                         "double integral")
    if a.row_rtol is not None or a.row_atol is not None or a.max_total is not None:
        raise SystemExit("integrate: --row-rtol / --row-atol are the per-row tolerance of an "
                         "--expr parameter sweep")
    if (a.rtol is not None or a.atol is not None or a.panels is not None
            or a.max_depth is not None or a.max_intervals is not None):
        raise SystemExit("integrate: --rtol / --atol and their bounds are the tolerance of an "
                         "--expr integrand")
    a.n = 1e9 if a.n is None else a.n
    a.rule = a.rule or "left"
    ctx = _ctx()
    r = Integrator(a.integrand, n=int(a.n), rule=a.rule, dtype=a.dtype, div=a.div, ctx=ctx,
                   backend=a.backend).run()
    if ctx.is_root:
        print(json.dumps(r.as_dict()))
    ctx.destroy()
    return 0


def _no_lattice_flags(a) -> None:
    for flag, on in (("--m", a.m is not None), ("--shifts", a.shifts is not None),
                     ("--seed", a.seed is not None), ("--z", bool(a.z)),
                     ("--periodic", a.periodic), ("--m-max", a.m_max is not None)):
        if on:
            raise SystemExit(f"integrate: {flag} belongs to --box (the lattice rule of an "
                             "--expr integrand)")


def _integrate_lattice(a) -> int:
    """integrate --expr E --box A0:B0,A1:B1,... --m M | --rtol R [--atol T]: the integral over a
    box by a randomly shifted lattice rule (one GPU, or --backend cpu for the numpy model).
    Whatever belongs to another mode is refused before anything runs."""
    from . import integrate_expr_nd

    given = {"--a": a.a is not None, "--b": a.b is not None, "--n": a.n is not None,
             "--rule": a.rule is not None, "--ya": a.ya is not None, "--yb": a.yb is not None,
             "--ny": a.ny is not None, "--params": bool(a.params),
             "--linspace": bool(a.linspace), "--panels": a.panels is not None,
             "--max-depth": a.max_depth is not None,
             "--max-intervals": a.max_intervals is not None}
    for flag, on in given.items():
        if on:
            raise SystemExit(f"integrate: --box integrates over a box by a lattice rule: {flag} "
                             "does not go with it")
    if a.device == "cpu" or a.backend == "host":
        which = "--device cpu" if a.device == "cpu" else "--backend host"
        raise SystemExit(f"integrate: --box has no host engine: {which} does not go with it")
    walk = a.rtol is not None or a.atol is not None
    if walk == (a.m is not None):
        raise SystemExit("integrate: --box takes --m M (the rule of 2^M points) or --rtol R / "
                         "--atol T (the walk over M), one of the two")
    if a.m_max is not None and not walk:
        raise SystemExit("integrate: --m-max belongs to --box with --rtol / --atol")
    try:
        box = [tuple(float(v) for v in side.split(":")) for side in a.box.split(",")]
        if any(len(side) != 2 for side in box):
            raise ValueError
        z = [int(v) for v in a.z.split(",")] if a.z else None
    except ValueError:
        raise SystemExit(f"integrate: --box wants A0:B0,A1:B1,... and --z Z0,Z1,... (got "
                         f"{a.box!r}, {a.z!r})") from None
    try:
        r = integrate_expr_nd(a.expr, box, m=a.m, rtol=a.rtol if walk else None,
                              atol=(a.atol or 0.0) if walk else 0.0,
                              shifts=16 if a.shifts is None else a.shifts, seed=a.seed or 0,
                              periodic=a.periodic, z=z, backend=a.backend, m_max=a.m_max)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"integrate: {e}") from None
    if walk and not r.converged:
        print(f"integrate: not converged: err_est {r.err_est:.3g} after {r.levels} levels "
              f"(m = {r.m})", file=sys.stderr)
    rec = r.as_dict()
    pack = __import__("struct").pack
    rec["value_bits"] = "%016x" % int.from_bytes(pack("<d", r.value), "little")
    rec["err_est_bits"] = "%016x" % int.from_bytes(pack("<d", r.err_est), "little")
    if a.analytic is not None:
        rec.update(analytic=a.analytic, abs_err=abs(r.value - a.analytic))
    print(json.dumps(rec))
    return 0


def _integrate_adaptive(a, lo: float, hi: float) -> int:
    """integrate --expr E --rtol R / --atol T: the integral to a tolerance (one GPU, one
    rank). Whatever belongs to another mode is refused before anything runs."""
    import os

    from . import integrate_expr_adaptive

    given = {"--n": a.n is not None, "--rule": a.rule is not None, "--ya": a.ya is not None,
             "--yb": a.yb is not None, "--ny": a.ny is not None, "--params": bool(a.params),
             "--linspace": bool(a.linspace)}
    for flag, on in given.items():
        if on:
            raise SystemExit(f"integrate: --rtol / --atol choose the samples themselves: {flag} "
                             "does not go with them")
    if a.device == "cpu" or a.backend != "hip":
        which = "--device cpu" if a.device == "cpu" else f"--backend {a.backend}"
        raise SystemExit(f"integrate: --rtol / --atol have no host engine: {which} does not go "
                         "with them")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("integrate: --rtol / --atol run as one rank: a rank environment "
                         f"(WORLD_SIZE = {os.environ['WORLD_SIZE']}) does not go with them")
    opts = {k: v for k, v in (("rtol", a.rtol), ("atol", a.atol), ("panels", a.panels),
                              ("max_depth", a.max_depth), ("max_intervals", a.max_intervals))
            if v is not None}
    try:
        r = integrate_expr_adaptive(a.expr, lo, hi, **opts)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"integrate: {e}") from None
    if not r.converged:
        print(f"integrate: not converged: err_est {r.err_est:.3g} against tol {r.tol:.3g} "
              f"(capped {int(r.capped)}, nonfinite {r.nonfinite}, forced {r.forced})",
              file=sys.stderr)
    rec = _json_ends(r.as_dict())
    rec["value_bits"] = "%016x" % int.from_bytes(__import__("struct").pack("<d", r.value),
                                                 "little")
    if a.analytic is not None:
        rec.update(analytic=a.analytic, abs_err=abs(r.value - a.analytic))
    print(json.dumps(rec))
    return 0


def _integrate_osc(a) -> int:
    """integrate --expr E --osc cos|sin --omega W --rtol R / --atol T: the integral of f(x)
    cos(W x) or f(x) sin(W x) to a tolerance (one GPU, one rank; --backend cpu: the numpy
    model); --b inf is the Fourier tail. Whatever belongs to another mode is refused before
    anything runs, naming the conflict."""
    import math
    import os

    from . import integrate_expr_oscillatory

    who = "--osc / --omega"
    if a.osc is None:
        which = "--omega" if a.omega is not None else "--max-cycles"
        raise SystemExit(f"integrate: {which} belongs to --osc cos|sin (the weight of an "
                         "oscillatory integral): --osc is missing")
    if a.omega is None:
        raise SystemExit("integrate: --osc needs --omega W (the weight is cos(W x) or sin(W x)): "
                         "--omega is missing")
    if not a.expr:
        raise SystemExit(f"integrate: {who} are the weight of an --expr integrand: --expr is "
                         "missing")
    if a.rtol is None and a.atol is None:
        raise SystemExit(f"integrate: {who} integrate to a tolerance: they need --rtol R / "
                         "--atol T")
    given = {"--n": a.n is not None, "--rule": a.rule is not None, "--ya": a.ya is not None,
             "--yb": a.yb is not None, "--ny": a.ny is not None, "--y-lo": a.y_lo is not None,
             "--y-hi": a.y_hi is not None, "--box": bool(a.box), "--params": bool(a.params),
             "--linspace": bool(a.linspace), "--row-rtol": a.row_rtol is not None,
             "--row-atol": a.row_atol is not None, "--area-rtol": a.area_rtol is not None,
             "--area-atol": a.area_atol is not None, "--panels-y": a.panels_y is not None,
             "--max-total": a.max_total is not None, "--m": a.m is not None,
             "--shifts": a.shifts is not None, "--seed": a.seed is not None, "--z": bool(a.z),
             "--periodic": a.periodic, "--m-max": a.m_max is not None}
    for flag, on in given.items():
        if on:
            raise SystemExit(f"integrate: {who} integrate one f(x) against one weight to a "
                             f"tolerance: {flag} does not go with them")
    if a.device == "cpu" or a.backend == "host":
        which = "--device cpu" if a.device == "cpu" else "--backend host"
        raise SystemExit(f"integrate: {who} have no host engine: {which} does not go with them")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"integrate: {who} run as one rank: a rank environment "
                         f"(WORLD_SIZE = {os.environ['WORLD_SIZE']}) does not go with them")
    lo = 0.0 if a.a is None else a.a
    hi = 1.0 if a.b is None else a.b
    if lo == -math.inf or hi == -math.inf or lo == math.inf:
        raise SystemExit(f"integrate: {who} take a finite range or (A, inf): --a {lo:g} --b "
                         f"{hi:g} does not go with them ((-inf, b) and two-sided Fourier "
                         "integrals are not supported)")
    if a.max_cycles is not None and hi != math.inf:
        raise SystemExit("integrate: --max-cycles bounds the Fourier tail: it needs --b inf")
    opts = {k: v for k, v in (("rtol", a.rtol), ("atol", a.atol), ("panels", a.panels),
                              ("max_depth", a.max_depth), ("max_intervals", a.max_intervals),
                              ("max_cycles", a.max_cycles)) if v is not None}
    if hi == math.inf and a.panels is not None:
        opts["tail_panels"] = opts.pop("panels")
    if hi == math.inf and a.rtol is not None and a.atol is None:
        raise SystemExit("integrate: the Fourier tail (--b inf) needs --atol T: its cycles are "
                         "held to shares of an absolute tolerance, --rtol alone is refused")
    if hi == math.inf:
        opts.setdefault("rtol", 0.0)
    try:
        r = integrate_expr_oscillatory(a.expr, lo, hi, a.omega, a.osc, backend=a.backend, **opts)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"integrate: {e}") from None
    if not r.converged:
        print(f"integrate: not converged: err_est {r.err_est:.3g} against tol {r.tol:.3g}: "
              f"{r.reason}", file=sys.stderr)
    rec = _json_ends(r.as_dict())
    rec["value_bits"] = "%016x" % int.from_bytes(__import__("struct").pack("<d", r.value),
                                                 "little")
    if a.analytic is not None:
        rec.update(analytic=a.analytic, abs_err=abs(r.value - a.analytic))
    print(json.dumps(rec) if a.json else f"{r.value:.17g}")
    return 0


def _integrate_adaptive2d(a, lo: float, hi: float) -> int:
    """integrate --expr E --ya AY --yb BY --area-rtol R / --area-atol T: the double integral to a
    tolerance (one GPU, one rank); with --y-lo EXPR --y-hi EXPR in place of --ya / --yb, y between
    two curves. Whatever belongs to another mode is refused before anything runs."""
    import math
    import os

    from . import integrate_expr2d_adaptive

    who = "--area-rtol / --area-atol"
    region = a.y_lo is not None or a.y_hi is not None
    if region and (a.y_lo is None or a.y_hi is None):
        missing = "--y-hi" if a.y_hi is None else "--y-lo"
        raise SystemExit("integrate: --y-lo and --y-hi go together (the two limits in y of a "
                         f"double integral): {missing} is missing")
    if region and (a.ya is not None or a.yb is not None):
        raise SystemExit("integrate: --y-lo / --y-hi are the limits in y as expressions over x: "
                         "--ya / --yb (the limits as numbers) do not go with them")
    if not region and (a.ya is None or a.yb is None):
        raise SystemExit(f"integrate: {who} are the tolerance of a double integral: they need "
                         "--ya AY --yb BY (or --y-lo EXPR --y-hi EXPR)")
    if a.rtol is not None or a.atol is not None:
        raise SystemExit(f"integrate: {who} are the tolerance of a double integral: --rtol / "
                         "--atol do not go with them")
    if a.row_rtol is not None or a.row_atol is not None or a.max_total is not None:
        raise SystemExit(f"integrate: {who} are the tolerance of a double integral: --row-rtol / "
                         "--row-atol do not go with them")
    given = {"--n": a.n is not None, "--ny": a.ny is not None, "--rule": a.rule is not None,
             "--params": bool(a.params), "--linspace": bool(a.linspace), "--box": bool(a.box)}
    for flag, on in given.items():
        if on:
            raise SystemExit(f"integrate: {who} choose the samples themselves: {flag} does not "
                             "go with them")
    _no_lattice_flags(a)
    if a.device == "cpu" or a.backend != "hip":
        which = "--device cpu" if a.device == "cpu" else f"--backend {a.backend}"
        raise SystemExit(f"integrate: {who} have no host engine: {which} does not go with them")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"integrate: {who} run as one rank: a rank environment "
                         f"(WORLD_SIZE = {os.environ['WORLD_SIZE']}) does not go with them")
    for flag, v in (("--a", lo), ("--b", hi), ("--ya", a.ya), ("--yb", a.yb)):
        if v is not None and math.isinf(v):
            raise SystemExit(f"integrate: {flag} {v}: {who} integrate over a finite rectangle "
                             "(no infinite side)")
    opts = {k: v for k, v in (("rtol", a.area_rtol), ("atol", a.area_atol),
                              ("panels_x", a.panels),
                              ("panels_y", a.panels if a.panels_y is None else a.panels_y),
                              ("max_depth", a.max_depth), ("max_intervals", a.max_intervals))
            if v is not None}
    try:
        if region:
            from . import integrate_expr2d_region

            r = integrate_expr2d_region(a.expr, lo, hi, a.y_lo, a.y_hi, **opts)
        else:
            r = integrate_expr2d_adaptive(a.expr, lo, hi, a.ya, a.yb, **opts)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"integrate: {e}") from None
    if not r.converged:
        print(f"integrate: not converged: err_est {r.err_est:.3g} against tol {r.tol:.3g} "
              f"(capped {int(r.capped)}, nonfinite {r.nonfinite}, forced {r.forced})",
              file=sys.stderr)
    if not a.json:
        print(f"{r.value:.17g}")
        return 0
    rec = r.as_dict()
    rec["value_bits"] = "%016x" % int.from_bytes(__import__("struct").pack("<d", r.value),
                                                 "little")
    if a.analytic is not None:
        rec.update(analytic=a.analytic, abs_err=abs(r.value - a.analytic))
    print(json.dumps(rec))
    return 0


def _integrate_adaptive_sweep(a, lo: float, hi: float) -> int:
    """integrate --expr E --params FILE | --linspace SPEC --row-rtol R / --row-atol T: every row
    to its own tolerance in shared rounds (one GPU, one rank). Whatever belongs to another mode is
    refused before anything runs."""
    import os

    from . import integrate_expr_adaptive_sweep
    from ._native import native

    who = "--row-rtol / --row-atol"
    if a.rtol is not None or a.atol is not None:
        raise SystemExit(f"integrate: {who} are the per-row tolerance of a parameter sweep: "
                         "--rtol / --atol do not go with them")
    given = {"--n": a.n is not None, "--rule": a.rule is not None, "--ya": a.ya is not None,
             "--yb": a.yb is not None, "--ny": a.ny is not None, "--box": bool(a.box)}
    for flag, on in given.items():
        if on:
            raise SystemExit(f"integrate: {who} choose the samples themselves: {flag} does not "
                             "go with them")
    _no_lattice_flags(a)
    if not (a.params or a.linspace):
        raise SystemExit(f"integrate: {who} need the rows of --params FILE or --linspace "
                         "p0=LO:HI:COUNT")
    if a.params and a.linspace:
        raise SystemExit("integrate: give --params FILE or --linspace, not both")
    if a.device == "cpu" or a.backend != "hip":
        which = "--device cpu" if a.device == "cpu" else f"--backend {a.backend}"
        raise SystemExit(f"integrate: {who} have no host engine: {which} does not go with them")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"integrate: {who} run as one rank: a rank environment "
                         f"(WORLD_SIZE = {os.environ['WORLD_SIZE']}) does not go with them")
    opts = {k: v for k, v in (("rtol", a.row_rtol), ("atol", a.row_atol), ("panels", a.panels),
                              ("max_depth", a.max_depth), ("max_intervals", a.max_intervals),
                              ("max_total", a.max_total)) if v is not None}
    if a.ranges and (a.a is not None or a.b is not None):
        raise SystemExit("integrate: --ranges gives every row its own a and b: --a / --b do not "
                         "go with it")
    m = native()
    try:
        rows = m.load_param_rows(a.params) if a.params else m.linspace_param_rows(a.linspace)
        if a.ranges:
            ends = _load_columns(a.ranges, 2, "--ranges", "a b")
            if len(ends) != len(rows):
                raise ValueError(f"--ranges {a.ranges}: {len(ends)} ranges for {len(rows)} rows")
            lo, hi = [e[0] for e in ends], [e[1] for e in ends]
        r = integrate_expr_adaptive_sweep(a.expr, rows, lo, hi, **opts)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"integrate: {e}") from None
    missed = int((~r.converged).sum())
    if missed:
        print(f"integrate: not converged: {missed} of {len(r.value)} rows (see converged, capped, "
              "nonfinite and forced per row with --json)", file=sys.stderr)
    if not a.json:
        for k, (row, v) in enumerate(zip(rows, r.value)):
            print(k, " ".join(f"{p:.17g}" for p in row), f"{v:.17g}")
        return 0
    pack = __import__("struct").pack
    rec = _json_ends({k: (v.tolist() if hasattr(v, "tolist") else v)
                      for k, v in r.as_dict().items()})
    rec["rows"] = len(r.value)
    rec["not_converged"] = missed
    rec["value_bits"] = ["%016x" % int.from_bytes(pack("<d", float(v)), "little")
                         for v in r.value]
    print(json.dumps(rec))
    return 0


def _load_columns(path: str, columns: int, flag: str, what: str) -> list:
    """The lines of a text file as tuples of ``columns`` numbers (blank lines and lines that
    begin with # are skipped); anything else is refused, naming the line."""
    out = []
    try:
        with open(path) as fh:
            lines = fh.read().splitlines()
    except OSError as e:
        raise ValueError(f"{flag} {path}: {e.strerror}") from None
    for n, line in enumerate(lines, 1):
        words = line.split()
        if not words or words[0].startswith("#"):
            continue
        try:
            row = tuple(float(w) for w in words)
        except ValueError:
            row = ()
        if len(row) != columns:
            raise ValueError(f"{flag} {path}: line {n}: expected `{what}`, got '{line.strip()}'")
        out.append(row)
    return out


def _integrate_curve(a) -> int:
    """integrate --expr E --curve-rtol R / --curve-atol T with --a A --b B --points M or --at
    FILE: the running integral on the grid, every cell to a tolerance (one GPU, one rank).
    Whatever belongs to another mode is refused before anything runs."""
    import math
    import os

    import numpy as np

    from . import integrate_expr_curve

    who = "--curve-rtol / --curve-atol"
    if a.curve_rtol is None and a.curve_atol is None:
        raise SystemExit(f"integrate: --points / --at are the grid of a running integral to a "
                         f"tolerance: they need {who}")
    if not a.expr:
        raise SystemExit(f"integrate: {who} are the tolerance of an --expr running integral")
    given = {"--n": a.n is not None, "--rule": a.rule is not None, "--rtol": a.rtol is not None,
             "--atol": a.atol is not None, "--row-rtol": a.row_rtol is not None,
             "--row-atol": a.row_atol is not None, "--ranges": bool(a.ranges),
             "--area-rtol": a.area_rtol is not None, "--area-atol": a.area_atol is not None,
             "--panels-y": a.panels_y is not None, "--y-lo": a.y_lo is not None,
             "--y-hi": a.y_hi is not None, "--ya": a.ya is not None, "--yb": a.yb is not None,
             "--ny": a.ny is not None, "--box": bool(a.box), "--osc": a.osc is not None,
             "--omega": a.omega is not None, "--max-cycles": a.max_cycles is not None,
             "--params": bool(a.params), "--linspace": bool(a.linspace)}
    for flag, on in given.items():
        if on:
            raise SystemExit(f"integrate: {who} are the tolerance of a running integral on a "
                             f"grid: {flag} does not go with them")
    _no_lattice_flags(a)
    if a.device == "cpu" or a.backend != "hip":
        which = "--device cpu" if a.device == "cpu" else f"--backend {a.backend}"
        raise SystemExit(f"integrate: {who} have no host engine: {which} does not go with them")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"integrate: {who} run as one rank: a rank environment "
                         f"(WORLD_SIZE = {os.environ['WORLD_SIZE']}) does not go with them")
    if a.at:
        if a.a is not None or a.b is not None or a.points is not None:
            raise SystemExit("integrate: --at FILE is the whole grid: --a / --b / --points do not "
                             "go with it")
    else:
        if a.a is None or a.b is None or a.points is None:
            raise SystemExit(f"integrate: {who} need a grid: --a A --b B --points M, or --at FILE")
        if math.isinf(a.a) or math.isinf(a.b):
            raise SystemExit(f"integrate: {who} take a finite grid: --a {a.a} --b {a.b} has an "
                             "infinite end")
        if a.points < 1:
            raise SystemExit(f"integrate: --points {a.points} must be at least 1")
    opts = {k: v for k, v in (("rtol", a.curve_rtol), ("atol", a.curve_atol),
                              ("panels", a.panels), ("max_depth", a.max_depth),
                              ("max_intervals", a.max_intervals), ("max_total", a.max_total))
            if v is not None}
    try:
        if a.at:
            x = np.array([p[0] for p in _load_columns(a.at, 1, "--at", "x")], dtype=np.float64)
        else:  # x_j = a + ((b - a) j) / M, the last one b: the adaptive rules' edges
            j = np.arange(a.points + 1, dtype=np.float64)
            x = a.a + ((a.b - a.a) * j) / float(a.points)
            x[-1] = a.b
        r = integrate_expr_curve(a.expr, x, **opts)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"integrate: {e}") from None
    missed = int((~r.cells["converged"]).sum())
    if missed:
        print(f"integrate: not converged: {missed} of {len(r.cells['value'])} cells, the first "
              f"one cell {int(np.flatnonzero(~r.cells['converged'])[0])} (see converged per point "
              "and capped, nonfinite and forced per cell with --json)", file=sys.stderr)
    if not a.json:
        for xj, v, e in zip(r.x, r.value, r.err_est):
            print(f"{xj:.17g} {v:.17g} {e:.3g}")
        return 0
    pack = __import__("struct").pack
    rec = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.as_dict().items()}
    rec["cells"] = {k: v.tolist() for k, v in r.cells.items()}
    rec["points"] = len(r.value)
    rec["not_converged"] = missed
    rec["value_bits"] = ["%016x" % int.from_bytes(pack("<d", float(v)), "little")
                         for v in r.value]
    print(json.dumps(rec))
    return 0


def cmd_table2d(a) -> int:
    """BASELINE #5: the separable field v(x) v(y) over [0, 1800]^2 on a grid x grid midpoint
    grid, bilinear interpolation of the 1801^2 outer-product table; ranks split the rows."""
    from ._native import native

    ctx = _ctx("gloo" if a.backend == "cpu" else None)  # cpu: host tensors, host collective
    m = native()
    want = m.table2d_oracle(a.grid)
    rec = {"program": "table2d", "grid": a.grid, "gpus": ctx.world, "backend": a.backend}
    if a.backend == "cpu":
        import torch

        from .ops.kernels import table2d_reference
        from .utils import fixtures

        from .parallel.decomposition import rank_slice

        v = torch.as_tensor(fixtures.profile_table(), dtype=torch.float64)
        b, c = rank_slice(a.grid, ctx.rank, ctx.world)  # this rank's sample rows
        part = table2d_reference(torch.outer(v, v), 1800.0, 1800.0, a.grid, a.grid, b, b + c)
        rec["result"] = float(ctx.all_reduce_sum(torch.tensor([part], dtype=torch.float64))[0])
    else:
        from .parallel.dist import native_comm

        comm = native_comm(ctx) if ctx.world > 1 else None
        plan = m.Table2DPlan(a.grid, 1800.0, ctx.device, comm)
        rec["result"] = plan.run()
        rec["ms_per_integration"] = plan.time(a.iters, True)
        rec["samples_per_s"] = a.grid * a.grid / (rec["ms_per_integration"] * 1e-3)
    rec["midpoint_oracle"] = want
    rec["rel_err_vs_oracle"] = abs(rec["result"] - want) / want
    if ctx.is_root:
        print(json.dumps(rec))
    ctx.destroy()
    return 0


def cmd_oracle(a) -> int:
    from ._native import native

    m = native()
    o = m.oracle
    rows = {
        "profile_exact_integral": o.profile_exact_integral(),
        "cintegrate_sp32_sm2": o.cintegrate_parity(32, 2),
        "cintegrate_sp30_sm2": o.cintegrate_parity(30, 2),
        "cintegrate_sp32_sm3": o.cintegrate_parity(32, 3),
        "trainscan_p1": o.trainscan_parity(1)[0],
        "trainscan_p7": o.trainscan_parity(7)[0],
        "trainscan_p16": o.trainscan_parity(16)[0],
        "riemann_np8_n1e6": o.riemann_mpi_parity(8, 1e6),
        "train_analytic_1800": o.train_distance(1800.0),
        "pi4_left_n1e6_err": o.riemann_serial(m.Integrand.pi4, 0, 1, 10**6, m.Rule.left) - math.pi,
    }
    print(json.dumps(rows, indent=1))
    return 0


def cmd_info(a) -> int:
    from . import __version__
    from ._native import extension_path, native

    m = native()
    n = m.device_count()
    print(f"cuda_v_mpi_amd {__version__}  extension {extension_path()}")
    for d in range(n):
        print(" ", m.device_info(d))
    if n == 0:
        print("  no HIP device visible")
    return 0


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="python -m cuda_v_mpi_amd", description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="cmd", required=True)

    def common(sp, integrand="sin"):
        sp.add_argument("--integrand", default=integrand)
        sp.add_argument("--n", type=float, default=1e9)
        sp.add_argument("--rule", default="left", choices=["left", "mid", "right"])
        sp.add_argument("--dtype", default="fp64", choices=["fp64", "fp32", "fp32acc"])
        sp.add_argument("--div", default="series_exact", choices=["series", "ieee", "series_direct", "series_exact"])
        sp.add_argument("--block", type=int, default=256, choices=[64, 128, 256, 512, 1024],
                        help="threads per workgroup (the reference's SP)")
        sp.add_argument("--backend", default="hip", choices=["hip", "host", "cpu"])
        sp.add_argument("--json", action="store_true")

    common(sub.add_parser("riemann"))
    c = sub.add_parser("cintegrate")
    c.add_argument("--parity", action="store_true")
    c.add_argument("--sp", type=int, default=32)
    c.add_argument("--sm", type=int, default=2)
    c.add_argument("--backend", default="hip", choices=["hip", "host", "cpu"])
    c.add_argument("--json", action="store_true")
    t = sub.add_parser("trainscan")
    t.add_argument("--parity", action="store_true")
    t.add_argument("--algo", default="fused", choices=["fused", "onepass", "lookback"])
    t.add_argument("--json", action="store_true")
    ig = sub.add_parser("integrate")
    common(ig, integrand="pi4")
    ig.add_argument("--expr", default="", help="any f(x) as one C++ expression over x (hipRTC)")
    ig.add_argument("--a", type=float, default=None, help="the lower end; with --rtol / --atol "
                    "or --row-rtol / --row-atol also inf, +inf, -inf or infinity (any case): "
                    "(A, inf), (-inf, B) and (-inf, inf) are mapped onto t in (0, 1] and the "
                    "rounds bisect t (the record's range: finite, upper, lower or both; resabs is "
                    "then that of the mapped integrand, for (-inf, inf) the integral of "
                    "|f(x) + f(-x)| over (0, inf)). A singularity at the finite end ends as "
                    "nonfinite: split the range there. An oscillatory tail does not converge, "
                    "and the run says so. Refused without a tolerance flag")
    ig.add_argument("--b", type=float, default=None, help="the upper end, as --a")
    ig.add_argument("--analytic", type=float, default=None)
    ig.add_argument("--params", default="", help="--expr over x and p0..p7: a file of "
                    "parameter rows (one per line), all rows in one launch")
    ig.add_argument("--linspace", default="", help="p0=LO:HI:COUNT, a one-parameter sweep")
    ig.add_argument("--device", default="gpu", choices=["gpu", "cpu"],
                    help="sweeps and double integrals: cpu = the host cores (as --backend host)")
    ig.add_argument("--ya", type=float, default=None, help="with --yb: the double integral of "
                    "--expr over x and y on [a, b] x [ya, yb], n x ny samples")
    ig.add_argument("--yb", type=float, default=None)
    ig.add_argument("--ny", type=float, default=None, help="samples along y (default: --n)")
    ig.add_argument("--rtol", type=float, default=None, help="with --expr: integrate to the "
                    "tolerance max(atol, rtol |value|), adaptively (one GPU, one rank)")
    ig.add_argument("--atol", type=float, default=None)
    ig.add_argument("--panels", type=int, default=None, help="--rtol / --atol: the equal "
                    "intervals to start from (65536)")
    ig.add_argument("--max-depth", type=int, default=None, help="bisections of one interval (60)")
    ig.add_argument("--max-intervals", type=int, default=None, help="intervals in all (2^22)")
    ig.add_argument("--osc", default=None, choices=["cos", "sin"], help="with --expr, --omega W "
                    "and --rtol / --atol: the integral of f(x) cos(W x) or f(x) sin(W x) to the "
                    "tolerance, at a cost that does not grow with W (Filon-Clenshaw-Curtis (13, "
                    "25): one GPU, one rank; --backend cpu runs the numpy model). f must be "
                    "finite on the closed range. --b inf is the Fourier tail on (A, inf): it "
                    "needs W != 0 and --atol, --panels is then per cycle (16) and --max-cycles "
                    "bounds it. --json also carries omega, kind, cycles, extrapolated, reason")
    ig.add_argument("--omega", type=float, default=None, help="--osc: the weight's frequency W")
    ig.add_argument("--max-cycles", type=int, default=None, help="--osc with --b inf: the "
                    "cycles of the Fourier tail (50)")
    ig.add_argument("--area-rtol", type=float, default=None, help="with --expr and --ya / --yb: "
                    "the double integral over the finite rectangle to the tolerance "
                    "max(area-atol, area-rtol |value|): the (7, 15) x (7, 15) product on rectangles "
                    "bisected along the axis with the larger error (one GPU, one rank); prints the "
                    "value, --json the record. --panels P and --panels-y Q (64, Q defaults to P) "
                    "are then the first grid, --max-depth is per axis. An indicator's curve runs "
                    "to the cap and reports capped")
    ig.add_argument("--area-atol", type=float, default=None)
    ig.add_argument("--panels-y", type=int, default=None, help="--area-rtol / --area-atol: the "
                    "equal parts along y to start from (default: --panels)")
    ig.add_argument("--y-lo", default=None, metavar="EXPR", help="with --y-hi and --area-rtol / "
                    "--area-atol, in place of --ya / --yb: the double integral over a <= x <= b, "
                    "y_lo(x) <= y <= y_hi(x), both limits expressions over x alone (write "
                    "--y-lo=-sqrt(1.0-x*x) where one begins with a minus). The region is mapped onto "
                    "[a, b] x [0, 1] and the rounds run on f (y_hi - y_lo); where y_hi < y_lo the "
                    "strip counts negatively. --json also carries y_lo, y_hi")
    ig.add_argument("--y-hi", default=None, metavar="EXPR")
    ig.add_argument("--row-rtol", type=float, default=None, help="with --expr and --params / "
                    "--linspace: every row to its own tolerance max(row-atol, row-rtol |value of "
                    "the row|), the rows sharing the rounds (one GPU, one rank); --panels and "
                    "--max-intervals are then per row")
    ig.add_argument("--row-atol", type=float, default=None)
    ig.add_argument("--max-total", type=int, default=None, help="--row-rtol / --row-atol: "
                    "intervals of all rows together (2^22)")
    ig.add_argument("--ranges", default="", metavar="FILE", help="--row-rtol / --row-atol: a "
                    "file of K lines `a b`, row r integrated over its own finite [a_r, b_r] "
                    "(instead of --a / --b); a_r > b_r negates the row, a_r == b_r gives 0")
    ig.add_argument("--curve-rtol", type=float, default=None, help="with --expr: the running "
                    "integral F(x_j) from x_0 on a grid, either --a A --b B --points M (M equal "
                    "cells) or --at FILE (one grid point per line, strictly increasing or "
                    "decreasing); every cell to max(its share of curve-atol by length, "
                    "curve-rtol |its integral|). Prints `x F err_est` lines, or --json with the "
                    "arrays (one GPU, one rank); --panels and --max-intervals are then per cell")
    ig.add_argument("--curve-atol", type=float, default=None)
    ig.add_argument("--points", type=int, default=None, metavar="M",
                    help="--curve-rtol / --curve-atol: M equal cells on [a, b]")
    ig.add_argument("--at", default="", metavar="FILE",
                    help="--curve-rtol / --curve-atol: the grid, one point per line")
    ig.add_argument("--box", default="", help="with --expr over x0, x1, ...: A0:B0,A1:B1,..., the "
                    "integral over the box by a randomly shifted lattice rule (--m M, or --rtol / "
                    "--atol for the walk over M)")
    ig.add_argument("--m", type=int, default=None, help="--box: n = 2^M points per shift")
    ig.add_argument("--shifts", type=int, default=None, help="--box: random shifts (16)")
    ig.add_argument("--seed", type=int, default=None, help="--box: the shifts' seed (0)")
    ig.add_argument("--z", default="", help="--box --m: the generating vector Z0,Z1,...")
    ig.add_argument("--periodic", action="store_true", help="--box: no tent transform")
    ig.add_argument("--m-max", type=int, default=None, help="--box --rtol: the last level")
    ig.set_defaults(n=None, rule=None)  # given or not: --rtol / --atol refuse them
    t2 = sub.add_parser("table2d")
    t2.add_argument("--grid", type=int, default=4096)
    t2.add_argument("--iters", type=int, default=100)
    t2.add_argument("--backend", default="hip", choices=["hip", "cpu"])
    sub.add_parser("oracle")
    sub.add_parser("info")
    cp = sub.add_parser("compare")
    cp.add_argument("--integrand", default="sin")
    cp.add_argument("--n", type=float, default=1e9)
    cp.add_argument("--rule", default="left", choices=["left", "mid", "right"])
    cp.add_argument("--threads", type=int, default=0)
    cp.add_argument("--ranks", type=int, default=8, help="reference program: mpirun -np P")
    cp.add_argument("--reps", type=int, default=3)
    cp.add_argument("--steps", type=int, default=48)
    cp.add_argument("--expr", default="", help="any f(x) as one C++ expression over x")
    cp.add_argument("--a", type=float, default=None)
    cp.add_argument("--b", type=float, default=None)
    sc = sub.add_parser("scale")
    sc.add_argument("--gpus", default="1,2,4,8")
    sc.add_argument("--steps", type=int, default=200)
    sc.add_argument("--warmup", type=int, default=10)
    sc.add_argument("--no-comm", action="store_true")
    sc.add_argument("--jsonl", default="")
    sc.add_argument("--md", default="")
    a = p.parse_args(_join_infinities(sys.argv[1:] if argv is None else list(argv)))
    if a.cmd == "scale":
        from .parallel import scaling

        return scaling.main(["--gpus", a.gpus, "--steps", str(a.steps), "--warmup",
                             str(a.warmup)] + (["--no-comm"] if a.no_comm else []) +
                            (["--jsonl", a.jsonl] if a.jsonl else []) +
                            (["--md", a.md] if a.md else []))
    return {"riemann": cmd_riemann, "cintegrate": cmd_cintegrate, "trainscan": cmd_trainscan,
            "integrate": cmd_integrate, "table2d": cmd_table2d, "oracle": cmd_oracle,
            "info": cmd_info, "compare": cmd_compare}[a.cmd](a)


if __name__ == "__main__":
    sys.exit(main())
