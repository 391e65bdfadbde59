"""High-level integration API.

    >>> from cuda_v_mpi_amd import Integrator
    >>> r = Integrator("pi4", n=10**9).run()          # one MI355X, fp64, left rule
    >>> r.value, r.abs_err, r.subintervals_per_s

Backends
  ``hip``  the native runtime: gfx950 kernels, hipGraph replay, RCCL for world > 1
           (``comm="native"``: C++ RCCL communicator captured in the graph, default;
           ``comm="torch"``: kernels on the torch stream + torch.distributed all_reduce;
           ``comm_obj=``: any native communicator, e.g. a loopback rank, see
           parallel/loopback.py)
  ``host`` the native host engine (miint/host.hpp): the rank's slice evaluated per sample
           in fp64 on ``threads`` vector threads (AVX-512 / AVX2 / baseline, picked at run
           time), world > 1 reduced with torch.distributed (gloo). The reference's own (MPI,
           CPU) side of its CUDA-vs-MPI comparison; needs no GPU.
  ``cpu``  plain PyTorch fp64 evaluation of the rank's slice + torch.distributed (gloo)
           all_reduce. Exists so the decomposition / collective logic can be exercised
           without a GPU; it is never used implicitly.
"""
from __future__ import annotations

import dataclasses
import math
import time

import numpy as np
import torch

from .models import integrands
from .parallel import decomposition
from .parallel.dist import DistContext, native_comm


@dataclasses.dataclass
class IntegrationResult:
    value: float
    analytic: float
    n: int
    integrand: str
    rule: str
    dtype: str
    gpus: int
    seconds_wall: float
    seconds_device: float

    @property
    def abs_err(self) -> float:
        return abs(self.value - self.analytic)

    @property
    def rel_err(self) -> float:
        return self.abs_err / abs(self.analytic) if self.analytic else float("nan")

    @property
    def subintervals_per_s(self) -> float:
        t = self.seconds_device if self.seconds_device > 0 else self.seconds_wall
        return self.n / t if t > 0 else float("nan")

    def as_dict(self) -> dict:
        d = dataclasses.asdict(self)
        d.update(abs_err=self.abs_err, rel_err=self.rel_err,
                 subintervals_per_s=self.subintervals_per_s)
        return d


class Integrator:
    def __init__(self, integrand: str | integrands.IntegrandSpec = "pi4", n: int = 10**9,
                 rule: str = "left", dtype: str = "fp64", div: str = "series_exact",
                 backend: str = "hip", ctx: DistContext | None = None, comm: str = "native",
                 fused: bool = True, grid: int = 0, slots: int = 16, a: float | None = None,
                 b: float | None = None, force_collective: bool = False, bucket: bool = True,
                 chain: bool = True, comm_obj=None, threads: int = 0,
                 slice_of: tuple[int, int] | None = None, step_streams: int = 0,
                 block: int = 256, multistep: bool = True, close: str = "auto",
                 allreduce_to_host: bool = True, timeout_s: float = 300.0,
                 work: str = "auto", queue_wg_per_cu: int = 0, tile: str = "auto", **spec_kw):
        spec = integrands.get(integrand, **spec_kw) if isinstance(integrand, str) else integrand
        if a is not None or b is not None:
            spec = dataclasses.replace(spec, a=spec.a if a is None else a,
                                       b=spec.b if b is None else b)
        if n < 1:
            raise ValueError("n must be >= 1")
        if rule not in ("left", "mid", "right"):
            raise ValueError("rule must be left|mid|right")
        if dtype not in ("fp64", "fp32", "fp32acc"):
            raise ValueError("dtype must be fp64|fp32|fp32acc")
        self.spec, self.n, self.rule, self.dtype, self.div = spec, int(n), rule, dtype, div
        self.backend, self.comm_kind = backend, comm
        if comm_obj is not None:  # an existing native communicator (e.g. a loopback rank)
            ctx = DistContext(rank=comm_obj.rank, world=comm_obj.world, device=comm_obj.device,
                              backend=comm_obj.kind)
        self.ctx = ctx or DistContext()
        self.begin, self.count = decomposition.rank_slice(self.n, self.ctx.rank, self.ctx.world)
        self._plan = None
        self._comm = None
        self._pool = None
        if backend in ("hip", "host"):
            from ._native import native

            m = native()
            if backend == "hip" and m.device_count() < 1:
                raise RuntimeError("backend='hip' needs a HIP device; use backend='host' or "
                                   "'cpu' explicitly")
            cfg = m.RiemannConfig()
            cfg.integrand = getattr(m.Integrand, spec.name)
            cfg.a, cfg.b, cfg.n = spec.a, spec.b, self.n
            cfg.rule = getattr(m.Rule, rule)
            cfg.dtype = getattr(m.DType, dtype)
            cfg.div = getattr(m.DivMode, div)
            cfg.coef = list(spec.coef)
            cfg.p0, cfg.p1 = spec.p0, spec.p1
            cfg.table = spec.native_table()
            cfg.grid, cfg.fused, cfg.slots = grid, fused, slots
            cfg.block = block  # threads per workgroup (the reference's SP): 64 .. 1024
            cfg.force_collective = force_collective
            cfg.bucket = bucket
            cfg.chain = chain
            cfg.step_streams = step_streams
            cfg.multistep = multistep  # graph batches as one persistent launch
            cfg.close = close  # multi-step batches closed by a kernel or inside the launch
            if work not in ("auto", "static", "queue"):
                raise ValueError("work must be auto|static|queue")
            cfg.work = work  # multi-step batches dealt statically or from a work queue
            cfg.queue_wg_per_cu = queue_wg_per_cu  # its pullers per CU (0: the residency)
            if tile not in ("auto", "short", "long"):
                raise ValueError("tile must be auto|short|long")
            cfg.tile = tile  # fp64 series_exact pi4: 384- or 1536-sample tiles (plan.tile)
            cfg.allreduce_to_host = allreduce_to_host  # bucketed all-reduce into pinned memory
            cfg.timeout_s = timeout_s  # collective watchdog of the plan's sync (<= 0: none)
            if slice_of is not None:  # (rank, world): that rank's share, on this device
                cfg.slice_rank, cfg.slice_world = int(slice_of[0]), int(slice_of[1])
            self._m = m
            if backend == "host":
                self._cfg = cfg
                self._pool = m.HostPool(threads)
                return
            if comm_obj is not None:
                self._comm = comm_obj
                self._plan = m.RiemannPlan(cfg, comm_obj.device, comm_obj)
            elif (self.ctx.world > 1 or force_collective) and comm == "native":
                self._comm = native_comm(self.ctx)
                self._plan = m.RiemannPlan(cfg, self.ctx.device, self._comm)
            else:
                cfg.rank, cfg.world = self.ctx.rank, self.ctx.world
                self._plan = m.RiemannPlan(cfg, self.ctx.device)
        elif backend != "cpu":
            raise ValueError("backend must be 'hip', 'host' or 'cpu'")

    # ------------------------------------------------------------------ info
    @property
    def plan(self):
        return self._plan

    @property
    def h(self) -> float:
        return (self.spec.b - self.spec.a) / self.n

    def describe(self) -> dict:
        d = dict(integrand=self.spec.name, n=self.n, rule=self.rule, dtype=self.dtype,
                 backend=self.backend, rank=self.ctx.rank, world=self.ctx.world,
                 begin=self.begin, count=self.count)
        if self._plan is not None:
            d.update(grid=self._plan.grid, block=self._plan.block,
                     div=str(self._plan.effective_div).split(".")[-1])
        return d

    # ------------------------------------------------------------------ execution
    def _torch_reduce(self, value: float) -> float:
        dev = "cuda" if self.ctx.backend == "nccl" else "cpu"
        t = torch.tensor([value], dtype=torch.float64, device=dev)
        self.ctx.all_reduce_sum(t)
        return float(t.item())

    def _cpu_local(self) -> float:
        spec, h = self.spec, self.h
        off = {"left": 0.0, "mid": 0.5, "right": 1.0}[self.rule]
        dt = torch.float64 if self.dtype == "fp64" else torch.float32
        chunk = 1 << 22
        parts = []
        for s in range(self.begin, self.begin + self.count, chunk):
            i = torch.arange(s, min(self.begin + self.count, s + chunk), dtype=torch.float64)
            x = (spec.a + (i + off) * h).to(dt)
            parts.append(float(spec.f_torch(x).to(torch.float64).sum()))
        return math.fsum(parts) * h

    def run(self) -> IntegrationResult:
        t0 = time.perf_counter()
        dev_s = 0.0
        if self.backend == "cpu":
            value = self._torch_reduce(self._cpu_local()) if self.ctx.world > 1 else self._cpu_local()
        elif self.backend == "host":
            t = time.perf_counter()
            value = self._m.host_riemann(self._cfg, self.begin, self.count, self._pool)
            dev_s = time.perf_counter() - t  # the rank's compute time ("device" = host cores)
            if self.ctx.world > 1:
                value = self._torch_reduce(value)
        else:
            if self._comm is not None or self.ctx.world == 1:
                t = self._plan.run_steps(1, pipeline=False, graphs=False)
                value = self._plan.host_result(0)
                dev_s = t["device_ms"] * 1e-3
            else:  # torch.distributed reduction of the native plan's local value
                t = self._plan.run_steps(1, pipeline=False, graphs=False)
                value = self._torch_reduce(self._plan.host_result(0))
                dev_s = t["device_ms"] * 1e-3
        wall = time.perf_counter() - t0
        return IntegrationResult(value=value, analytic=self.spec.analytic(), n=self.n,
                                 integrand=self.spec.name, rule=self.rule, dtype=self.dtype,
                                 gpus=self.ctx.world, seconds_wall=wall, seconds_device=dev_s)

    def run_steps(self, steps: int, pipeline: bool = True, graphs: bool = True) -> dict:
        """Back-to-back integrations on the native runtime (benchmark inner loop)."""
        if self._plan is None:
            raise RuntimeError("run_steps needs backend='hip'")
        return self._plan.run_steps(steps, pipeline, graphs)

    def launch_steps(self, steps: int, pipeline: bool = True, graphs: bool = True) -> None:
        if self._plan is None:
            raise RuntimeError("launch_steps needs backend='hip'")
        self._plan.launch_steps(steps, pipeline, graphs)

    def sync(self) -> None:
        if self._plan is not None:
            self._plan.sync()

    def timeline(self, steps: int, form: str = "auto") -> dict:
        """One multi-step batch from the timeline build of its persistent launch
        (``RiemannPlan::timeline_batch``): per workgroup, device-clock stamps at kernel entry,
        after every step's block sum and at exit (``stamps`` uint64 [grid, steps + 2], ticks of
        ``clock_khz``), the shader clock at entry and exit, and the raw XCC_ID / HW_ID words
        (``hw``); ``xcc`` is the XCC id decoded from them. A diagnostic, never timed: read its
        shares (``tools/timeline_report.py``), not its length.

        A plan built with ``work="queue"`` (or ``form="queue"`` on any plan that runs the
        queue) records the queue launch instead (``t["work"] == "queue"``): per physical
        workgroup ``wg_stamps`` [workgroups, 2], per item ``item_stamp`` and ``item_owner``
        [steps, grid]; ``shader_clock``, ``hw`` and ``xcc`` are per physical workgroup."""
        if self._plan is None:
            raise RuntimeError("timeline needs backend='hip'")
        t = self._plan.timeline_batch(steps, form)
        t["xcc"] = t["hw"][:, 0] & 0xF
        return t


def integrate(integrand: str = "pi4", n: int = 10**9, **kw) -> IntegrationResult:
    return Integrator(integrand, n=n, **kw).run()


def integrate_expr(expr: str, a: float, b: float, n: int = 10**9, rule: str = "left",
                   backend: str = "hip", ctx: DistContext | None = None, threads: int = 0,
                   analytic: float | None = None) -> IntegrationResult:
    """Integrate any f(x) given as one C++ expression over ``x`` (``"exp(-x*x)"``): compiled
    for gfx950 with hipRTC (``backend="hip"``) or for the host cores (``backend="host"``),
    this rank's slice of the n-sample rule evaluated per sample in fp64, world > 1 reduced
    with torch.distributed. ``analytic`` (if known) sets the result's error reference.
    """
    from ._native import native

    if rule not in ("left", "mid", "right"):
        raise ValueError("rule must be left|mid|right")
    m = native()
    ctx = ctx or DistContext()
    begin, count = decomposition.rank_slice(int(n), ctx.rank, ctx.world)
    rl = getattr(m.Rule, rule)
    t0 = time.perf_counter()
    if backend == "hip":
        value = m.ExprIntegrator(expr, ctx.device).integrate(float(a), float(b), int(n), rl,
                                                              begin, count)
    elif backend == "host":
        value = m.HostExpr(expr).integrate(float(a), float(b), int(n), rl, begin, count,
                                           m.HostPool(threads))
    else:
        raise ValueError("integrate_expr backend must be 'hip' or 'host'")
    dev_s = time.perf_counter() - t0
    if ctx.world > 1:
        dev = "cuda" if ctx.backend == "nccl" else "cpu"
        t = torch.tensor([value], dtype=torch.float64, device=dev)
        ctx.all_reduce_sum(t)
        value = float(t.item())
    return IntegrationResult(value=value, analytic=float("nan") if analytic is None else analytic,
                             n=int(n), integrand=f"expr:{expr}", rule=rule, dtype="fp64",
                             gpus=ctx.world, seconds_wall=time.perf_counter() - t0,
                             seconds_device=dev_s)


def _fma_coords(first: int, count: int, off: float, h: float, a: float) -> torch.Tensor:
    """fma(i + off, h, a) for i in [first, first + count) as an fp64 tensor: the coordinates the
    expression kernels form, rounded once. torch has no fused multiply-add on the CPU, so the
    native module forms them on the host (std::fma; no GPU needed)."""
    from ._native import native

    return torch.from_numpy(native().fma_coords(int(first), int(count), float(off), float(h),
                                                float(a)))


def _tree_sum(t: torch.Tensor, dim: int) -> torch.Tensor:
    """Sum along `dim` in a fixed order: the upper half is added onto the lower half (the
    middle element of an odd length waits a level) until one element is left, so a value
    passes through ceil(log2(length)) additions. torch.sum's own order is not documented."""
    t = t.movedim(dim, -1)
    while t.shape[-1] > 1:
        n = t.shape[-1]
        half = n // 2
        low = t[..., :half] + t[..., n - half:]
        t = torch.cat([low, t[..., half:n - half]], dim=-1) if n % 2 else low
    return t[..., 0]


def integrate_expr2d(expr: str, ax: float, bx: float, ay: float, by: float, nx: int,
                     ny: int | None = None, rule: str = "mid", backend: str = "hip",
                     ctx: DistContext | None = None, threads: int = 0,
                     analytic: float | None = None) -> IntegrationResult:
    """The double integral of any f(x, y) given as one C++ expression over ``x`` and ``y`` on
    the rectangle [ax, bx] x [ay, by]: nx x ny samples (ny defaults to nx), the same rule on
    both axes, value = hx * hy * sum. ``backend="hip"``: the hipRTC-compiled gfx950 kernels
    (``ops.kernels.riemann_expr2d``); ``"host"``: compiled for the host cores (HostExpr2D);
    ``"cpu"``: the torch fp64 form (``expr_torch``'s subset of expressions) summed in row
    chunks in a fixed order (``_tree_sum``), needs no GPU. This rank integrates its rows, rank_slice(ny, rank, world); world > 1
    is reduced with torch.distributed."""
    if rule not in ("left", "mid", "right"):
        raise ValueError("rule must be left|mid|right")
    nx = int(nx)
    ny = nx if ny is None else int(ny)
    if nx < 1 or ny < 1:
        raise ValueError("integrate_expr2d needs nx >= 1 and ny >= 1")
    ax, bx, ay, by = float(ax), float(bx), float(ay), float(by)
    ctx = ctx or DistContext()
    begin, count = decomposition.rank_slice(ny, ctx.rank, ctx.world)
    t0 = time.perf_counter()
    if backend == "hip":
        from ._native import native

        m = native()
        value = m.ExprIntegrator2D(expr, ctx.device).integrate(
            ax, bx, nx, ay, by, ny, getattr(m.Rule, rule), begin, count)
    elif backend == "host":
        from ._native import native

        m = native()
        value = m.HostExpr2D(expr).integrate(ax, bx, nx, ay, by, ny, getattr(m.Rule, rule),
                                             begin, count, m.HostPool(threads))
    elif backend == "cpu":
        off = {"left": 0.0, "mid": 0.5, "right": 1.0}[rule]
        hx, hy = (bx - ax) / nx, (by - ay) / ny
        x = _fma_coords(0, nx, off, hx, ax)
        # fixed order: a row's columns in a tree, a chunk's rows in a tree, chunks one by one
        chunk = max(1, (1 << 22) // nx)      # rows per chunk: about 4 M samples at a time
        total = 0.0
        for r in range(begin, begin + count, chunk):
            y = _fma_coords(r, min(chunk, begin + count - r), off, hy, ay).unsqueeze(1)
            total += float(_tree_sum(_tree_sum(expr_torch(expr, x, y), 1), 0))
        value = total * (hx * hy)
    else:
        raise ValueError("integrate_expr2d backend must be 'hip', 'host' or 'cpu'")
    dev_s = time.perf_counter() - t0
    if ctx.world > 1:
        dev = "cuda" if ctx.backend == "nccl" else "cpu"
        t = torch.tensor([value], dtype=torch.float64, device=dev)
        ctx.all_reduce_sum(t)
        value = float(t.item())
    return IntegrationResult(value=value, analytic=float("nan") if analytic is None else analytic,
                             n=nx * ny, integrand=f"expr2d:{expr}", rule=rule, dtype="fp64",
                             gpus=ctx.world, seconds_wall=time.perf_counter() - t0,
                             seconds_device=dev_s)


@dataclasses.dataclass
class SweepResult:
    values: list            # K values, one per parameter row
    abs_err: list | None    # per row, when analytic values were given
    rows: int
    nparams: int
    n: int
    expr: str
    rule: str
    seconds: float          # the sweep call, rows in to values out (the compile is not in it)

    @property
    def subintervals_per_s(self) -> float:
        return self.rows * self.n / self.seconds if self.seconds > 0 else float("nan")

    def as_dict(self) -> dict:
        d = dataclasses.asdict(self)
        d.update(subintervals_per_s=self.subintervals_per_s)
        return d


def integrate_expr_sweep(expr: str, params, a: float, b: float, n: int = 10**6,
                         rule: str = "left", backend: str = "hip", threads: int = 0,
                         analytic=None) -> SweepResult:
    """A parameter sweep: the integral of f(x, p0, ..., p{nparams-1}) on [a, b] for every row
    of ``params`` (K x nparams; a list of rows or a 2-D array), the expression over ``x`` and
    ``p0`` .. ``p7`` compiled once, all K rows in one launch (``backend="hip"``,
    ``ops.kernels.riemann_expr_sweep``) or on the host cores (``backend="host"``).
    ``analytic`` (a sequence of K values) adds the per-row error."""
    from ._native import native
    from .ops.kernels import _param_rows

    if rule not in ("left", "mid", "right"):
        raise ValueError("rule must be left|mid|right")
    m = native()
    p = _param_rows(params)
    # the one compile stays outside the clock: it is per expression, not per sweep
    if backend == "hip":
        from .ops import kernels

        m.expr_sweep_compile(expr, int(p.shape[1]))
        t0 = time.perf_counter()
        values = kernels.riemann_expr_sweep(expr, p, float(a), float(b), int(n), rule=rule)
        values = [float(v) for v in values.cpu()]
    elif backend == "host":
        hs, pool = m.HostExprSweep(expr, p.shape[1]), m.HostPool(threads)
        t0 = time.perf_counter()
        values = [float(v) for v in hs.integrate(p, float(a), float(b), int(n),
                                                 getattr(m.Rule, rule), 0, int(n), pool)]
    else:
        raise ValueError("integrate_expr_sweep backend must be 'hip' or 'host'")
    secs = time.perf_counter() - t0
    err = None
    if analytic is not None:
        want = [float(w) for w in analytic]
        if len(want) != len(values):
            raise ValueError(f"analytic has {len(want)} values for {len(values)} rows")
        err = [abs(v - w) for v, w in zip(values, want)]
    return SweepResult(values=values, abs_err=err, rows=len(values), nparams=int(p.shape[1]),
                       n=int(n), expr=expr, rule=rule, seconds=secs)


@dataclasses.dataclass
class RunningResult:
    x: torch.Tensor         # upper limits: x[j] = a + (j + 1) * every * h
    values: torch.Tensor    # values[j] ~ the integral of f from a to x[j] (fp64)
    total: float            # h * sum over all n samples
    device_ms: float        # the scan's kernels (hip) or the evaluation (cpu), in ms


# What the torch form of an expression may call: the C names of the device math library that
# torch has under one name or another.
_TORCH_MATH = {
    "sin": torch.sin, "cos": torch.cos, "tan": torch.tan, "asin": torch.asin,
    "acos": torch.acos, "atan": torch.atan, "atan2": torch.atan2, "sinh": torch.sinh,
    "cosh": torch.cosh, "tanh": torch.tanh, "exp": torch.exp, "exp2": torch.exp2,
    "expm1": torch.expm1, "log": torch.log, "log2": torch.log2, "log10": torch.log10,
    "log1p": torch.log1p, "sqrt": torch.sqrt, "rsqrt": torch.rsqrt, "fabs": torch.abs,
    "abs": torch.abs, "erf": torch.erf, "erfc": torch.erfc, "floor": torch.floor,
    "ceil": torch.ceil, "pow": torch.pow, "fmin": torch.fmin, "fmax": torch.fmax,
    "hypot": torch.hypot, "fma": lambda p, q, r: p * q + r,
}


def expr_torch(expr: str, x: torch.Tensor, y: torch.Tensor | None = None,
               names: dict | None = None) -> torch.Tensor:
    """The torch form of a run-time expression: f(x) element-wise in x's dtype, for an
    expression made of numbers, ``x``, + - * /, parentheses and the math functions torch has
    (sin, exp, pow, fabs, ...). The syntax tree is walked, nothing is ``eval``-ed; anything
    else (``?:``, comparisons, other names) raises ValueError: the cpu backend covers the
    arithmetic subset of what the hipRTC backends compile. With ``y`` given the name ``y``
    resolves to it and the result has the broadcast shape of x and y (f(x, y)); without it
    ``y`` is an unknown name, as before. ``names`` maps further names to tensors (``x0`` ...
    ``x15`` of ``integrate_expr_nd``); they are looked up before ``x`` and ``y``."""
    import ast

    try:
        tree = ast.parse(expr.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError(f"the cpu backend cannot read the expression {expr!r}: {e.msg}") from None
    binops = {ast.Add: torch.add, ast.Sub: torch.sub, ast.Mult: torch.mul, ast.Div: torch.div}

    def const(v):
        return torch.tensor(float(v), dtype=x.dtype)

    def walk(node):
        if isinstance(node, ast.Expression):
            return walk(node.body)
        if isinstance(node, ast.Constant) and type(node.value) in (int, float):
            return const(node.value)
        if isinstance(node, ast.Name) and names is not None and node.id in names:
            return names[node.id]
        if isinstance(node, ast.Name) and node.id == "x":
            return x
        if isinstance(node, ast.Name) and node.id == "y" and y is not None:
            return y
        if isinstance(node, ast.BinOp) and type(node.op) in binops:
            return binops[type(node.op)](walk(node.left), walk(node.right))
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = walk(node.operand)
            return -v if isinstance(node.op, ast.USub) else v
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Name)
                and node.func.id in _TORCH_MATH and not node.keywords):
            return _TORCH_MATH[node.func.id](*[walk(arg) for arg in node.args])
        raise ValueError(f"the cpu backend does not evaluate {ast.dump(node)[:60]} "
                         f"(expression {expr!r})")

    if y is not None:
        return walk(tree) + torch.zeros_like(x + y)
    return walk(tree) + torch.zeros_like(x)  # a constant expression still has x's shape


def integrate_expr_running(expr: str, a: float, b: float, n: int, rule: str = "left",
                           every: int = 1, backend: str = "hip") -> RunningResult:
    """The running integral of any f(x) given as one C++ expression over ``x``, as a curve:
    ``values[j] = h * sum of f(x_i) over samples i < (j + 1) * every`` of the n-sample rule on
    [a, b], which approximates the integral of f from a to ``x[j] = a + (j + 1) * every * h``
    (floor(n / every) values; every = 1: one per sample). A distance curve from a velocity, a
    CDF from a density, an error function, an accumulated dose.

    ``backend="hip"``: three hipRTC-compiled gfx950 kernels, only the values are written to
    HBM (``ops.kernels.riemann_expr_scan``). ``backend="cpu"``: the torch fp64 form, ``cumsum``
    of the per-sample values at x_i = a + (i + off) * h (``expr_torch``'s subset of
    expressions); needs no GPU."""
    if rule not in ("left", "mid", "right"):
        raise ValueError("rule must be left|mid|right")
    n, every = int(n), int(every)
    if n < 1 or every < 1:
        raise ValueError("integrate_expr_running needs n >= 1 and every >= 1")
    a, b = float(a), float(b)
    h = (b - a) / n
    if backend == "hip":
        from .ops import kernels

        values, rec = kernels._expr_scan(expr, a, b, n, rule, every, 0, None, None)
        total, ms = rec["total"], rec["device_ms"]
    elif backend == "cpu":
        off = {"left": 0.0, "mid": 0.5, "right": 1.0}[rule]
        t0 = time.perf_counter()
        run = torch.cumsum(expr_torch(expr, a + (torch.arange(n, dtype=torch.float64) + off) * h),
                           dim=0)
        values = run[every - 1::every] * h
        total = float(run[-1]) * h
        ms = (time.perf_counter() - t0) * 1e3
    else:
        raise ValueError("integrate_expr_running backend must be 'hip' or 'cpu'")
    x = a + torch.arange(1, values.numel() + 1, dtype=torch.float64) * (every * h)
    return RunningResult(x=x.to(values.device), values=values, total=total, device_ms=ms)


@dataclasses.dataclass
class AdaptiveResult:
    value: float
    err_est: float          # the sum of the accepted intervals' |K15 - G7|
    resabs: float           # the rule's integral of |f|
    tol: float              # the last round's tolerance, max(atol, rtol * |value so far|)
    converged: bool         # err_est <= tol, not capped, no non-finite interval
    evals: int              # 15 x intervals evaluated
    rounds: int
    intervals: int          # the final partition
    splits: int
    floor: int              # accepted because |K15 - G7| is rounding noise
    forced: int             # accepted at max_depth, or too narrow to bisect
    nonfinite: int
    capped: bool            # the partition would have passed max_intervals
    device_ms: float        # the rounds (hip) or the model's run (cpu), in ms
    expr: str
    a: float
    b: float
    backend: str
    range: str = "finite"   # "upper" (a, inf), "lower" (-inf, b), "both" (-inf, inf)

    def as_dict(self) -> dict:
        return dataclasses.asdict(self)


_ADAPT_FIELDS = ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds",
                 "intervals", "splits", "floor", "forced", "nonfinite", "capped", "range")


def integrate_expr_adaptive(expr: str, a: float, b: float, rtol: float = 1e-10,
                            atol: float = 0.0, panels: int = 65536, max_depth: int = 60,
                            max_intervals: int = 1 << 22,
                            backend: str = "hip") -> AdaptiveResult:
    """The integral of any f(x) given as one C++ expression over ``x`` on [a, b] to the
    tolerance max(atol, rtol * |value|), with an error estimate and a ``converged`` flag:
    adaptive Gauss-Kronrod (7, 15), the intervals bisected where the estimate misses.
    ``backend="hip"``: the hipRTC-compiled gfx950 kernels (``ops.kernels.quad_expr``), one GPU.
    ``backend="cpu"``: the numpy model of the same rule (``utils.adaptive_quad``) on
    ``expr_torch``'s evaluation of the expression (its subset of expressions); needs no GPU.
    One rank, one f(x). a and b may be infinite (``float("inf")``): (a, inf), (-inf, b) and
    (-inf, inf) are mapped onto t in (0, 1] and the rounds bisect t; ``range`` names the kind, and
    err_est, resabs and tol are those of the mapped integrand (for (-inf, inf) resabs is the
    integral of |f(x) + f(-x)| over (0, inf)). A singularity at the finite end ends as
    ``nonfinite`` (split the range there), an oscillatory tail does not converge."""
    a, b = float(a), float(b)
    if backend == "hip":
        from .ops import kernels

        r = kernels.quad_expr(expr, a, b, rtol=rtol, atol=atol, panels=panels,
                              max_depth=max_depth, max_intervals=max_intervals, unbounded=True)
        fields = {k: getattr(r, k) for k in _ADAPT_FIELDS}
        ms = r.device_ms
    elif backend == "cpu":
        from .utils.adaptive_quad import adaptive_model

        def f(x):
            return expr_torch(expr, torch.from_numpy(x)).numpy()

        t0 = time.perf_counter()
        r = adaptive_model(f, a, b, rtol=rtol, atol=atol, panels=int(panels),
                           max_depth=int(max_depth), max_intervals=int(max_intervals),
                           unbounded=True)
        ms = (time.perf_counter() - t0) * 1e3
        fields = {k: r[k] for k in _ADAPT_FIELDS}
    else:
        raise ValueError("integrate_expr_adaptive backend must be 'hip' or 'cpu'")
    return AdaptiveResult(**fields, device_ms=ms, expr=expr, a=a, b=b, backend=backend)


@dataclasses.dataclass
class OscillatoryResult(AdaptiveResult):
    """``AdaptiveResult`` (evals counts 25 per interval; err_est sums |K25 - K13|) and the
    weight: cos(omega x) or sin(omega x). ``cycles`` and ``extrapolated`` describe a Fourier
    tail (b = inf); ``reason`` says why a run did not converge."""
    omega: float = 0.0
    kind: str = "cos"
    cycles: int = 0
    extrapolated: bool = False
    reason: str = ""


_OSC_FIELDS = _ADAPT_FIELDS + ("omega", "kind", "cycles", "extrapolated", "reason")


def integrate_expr_oscillatory(expr: str, a: float, b: float, omega: float, kind: str = "cos",
                               rtol: float = 1e-10, atol: float = 0.0, panels: int = 65536,
                               max_depth: int = 60, max_intervals: int = 1 << 22,
                               tail_panels: int = 16, max_cycles: int = 50,
                               backend: str = "hip") -> OscillatoryResult:
    """The integral of f(x) cos(omega x) or f(x) sin(omega x) on [a, b] to the tolerance
    max(atol, rtol * |value|): f is one C++ expression over ``x``, omega a number, and the cost
    does not grow with omega (adaptive Filon-Clenshaw-Curtis: the weight is integrated exactly,
    only f is interpolated). ``backend="hip"``: the hipRTC-compiled gfx950 kernels
    (``ops.kernels.quad_expr_osc``), one GPU. ``backend="cpu"``: the numpy model of the same
    rule (``utils.adaptive_osc``) on ``expr_torch``'s evaluation of the expression; needs no
    GPU. f must be finite on the closed range: both ends of every interval are evaluated.
    ``b = inf`` is the Fourier tail on (a, inf): it needs omega != 0 and atol > 0 (rtol alone is
    refused), runs cycles of ``tail_panels`` panels and extrapolates their partial sums; a = -inf
    is not supported. One rank, one f(x), one omega."""
    import math

    a, b, omega = float(a), float(b), float(omega)
    tail = math.isinf(b) and b > 0 and math.isfinite(a)
    if backend == "hip":
        from .ops import kernels

        r = kernels.quad_expr_osc(expr, a, b, omega, kind, rtol=rtol, atol=atol, panels=panels,
                                  max_depth=max_depth, max_intervals=max_intervals,
                                  tail_panels=tail_panels, max_cycles=max_cycles)
        fields = {k: getattr(r, k) for k in _OSC_FIELDS}
        ms = r.device_ms
    elif backend == "cpu":
        from .utils.adaptive_osc import osc_model, osc_tail_model

        def f(x):
            return expr_torch(expr, torch.from_numpy(np.ascontiguousarray(x))).numpy()

        t0 = time.perf_counter()
        if tail:
            r = osc_tail_model(f, a, omega, kind, atol=atol, rtol=rtol, max_depth=int(max_depth),
                               max_intervals=int(max_intervals), panels=int(tail_panels),
                               max_cycles=int(max_cycles))
        else:
            r = osc_model(f, a, b, omega, kind, rtol=rtol, atol=atol, panels=int(panels),
                          max_depth=int(max_depth), max_intervals=int(max_intervals))
        ms = (time.perf_counter() - t0) * 1e3
        fields = {k: r[k] for k in _OSC_FIELDS}
    else:
        raise ValueError("integrate_expr_oscillatory backend must be 'hip' or 'cpu'")
    return OscillatoryResult(**fields, device_ms=ms, expr=expr, a=a, b=b, backend=backend)


@dataclasses.dataclass
class Adaptive2DResult:
    value: float
    err_est: float          # the sum of the accepted rectangles' |K15xK15 - G7xG7|
    resabs: float           # the rule's integral of |f|
    tol: float              # the last round's tolerance, max(atol, rtol * |value so far|)
    converged: bool         # err_est <= tol, not capped, no non-finite rectangle
    evals: int              # 225 x rectangles evaluated
    rounds: int
    intervals: int          # the rectangles of the final partition
    splits: int
    splits_x: int           # bisections along x; splits = splits_x + splits_y
    splits_y: int
    floor: int              # accepted because the difference is rounding noise
    forced: int             # accepted at the axis's max_depth, or too narrow to bisect
    nonfinite: int
    capped: bool            # the partition would have passed max_intervals
    device_ms: float        # the rounds (hip) or the model's run (cpu), in ms
    expr: str
    ax: float
    bx: float
    ay: float
    by: float
    backend: str

    def as_dict(self) -> dict:
        return dataclasses.asdict(self)


_ADAPT2D_FIELDS = ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds",
                   "intervals", "splits", "splits_x", "splits_y", "floor", "forced", "nonfinite",
                   "capped")


def integrate_expr2d_adaptive(expr: str, ax: float, bx: float, ay: float, by: float,
                              rtol: float = 1e-10, atol: float = 0.0, panels_x: int = 64,
                              panels_y: int = 64, max_depth: int = 60,
                              max_intervals: int = 1 << 22,
                              backend: str = "hip") -> Adaptive2DResult:
    """The double integral of any f(x, y) given as one C++ expression over ``x`` and ``y`` on the
    finite rectangle [ax, bx] x [ay, by] to the tolerance max(atol, rtol * |value|), with an
    error estimate and a ``converged`` flag: the (7, 15) x (7, 15) Gauss-Kronrod product on
    rectangles, each bisected along the axis that carries more of its error.
    ``backend="hip"``: the hipRTC-compiled gfx950 kernels (``ops.kernels.quad_expr2d``), one GPU.
    ``backend="cpu"``: the numpy model of the same rule (``utils.adaptive_quad2d``) on
    ``expr_torch``'s evaluation of the expression (its subset of expressions); needs no GPU.
    One rank, one f(x, y), finite sides. A discontinuity along a curve (an indicator) is never
    within its share of the tolerance: such a run ends ``capped``."""
    ax, bx, ay, by = float(ax), float(bx), float(ay), float(by)
    if backend == "hip":
        from .ops import kernels

        r = kernels.quad_expr2d(expr, ax, bx, ay, by, rtol=rtol, atol=atol,
                                panels=(int(panels_x), int(panels_y)), max_depth=max_depth,
                                max_intervals=max_intervals)
        fields = {k: getattr(r, k) for k in _ADAPT2D_FIELDS}
        ms = r.device_ms
    elif backend == "cpu":
        from .utils.adaptive_quad2d import adaptive2d_model

        def f(x, y):
            return expr_torch(expr, torch.from_numpy(np.ascontiguousarray(x)),
                              torch.from_numpy(np.ascontiguousarray(y))).numpy()

        t0 = time.perf_counter()
        r = adaptive2d_model(f, ax, bx, ay, by, rtol=rtol, atol=atol, panels_x=int(panels_x),
                             panels_y=int(panels_y), max_depth=int(max_depth),
                             max_intervals=int(max_intervals))
        ms = (time.perf_counter() - t0) * 1e3
        fields = {k: r[k] for k in _ADAPT2D_FIELDS}
    else:
        raise ValueError("integrate_expr2d_adaptive backend must be 'hip' or 'cpu'")
    return Adaptive2DResult(**fields, device_ms=ms, expr=expr, ax=ax, bx=bx, ay=ay, by=by,
                            backend=backend)


@dataclasses.dataclass
class AdaptiveRegionResult(Adaptive2DResult):
    """An ``Adaptive2DResult`` of the mapped integrand f (y_hi - y_lo) on [ax, bx] x [0, 1]:
    ``ay`` and ``by`` are 0.0 and 1.0, the ends of the mapped variable."""
    y_lo: str               # the limits in y, expressions over x
    y_hi: str


def integrate_expr2d_region(expr: str, ax: float, bx: float, y_lo: str, y_hi: str,
                            rtol: float = 1e-10, atol: float = 0.0, panels_x: int = 64,
                            panels_y: int = 64, max_depth: int = 60,
                            max_intervals: int = 1 << 22,
                            backend: str = "hip") -> AdaptiveRegionResult:
    """The double integral of f(x, y) over the region { ax <= x <= bx, y_lo(x) <= y <= y_hi(x) }
    to the tolerance max(atol, rtol * |value|): ``expr`` over ``x`` and ``y``, the two limits
    C++ expressions over ``x`` alone. The region is mapped onto [ax, bx] x [0, 1] by
    y = y_lo + (y_hi - y_lo) v, and the rounds of ``integrate_expr2d_adaptive`` run on the mapped
    integrand f (y_hi - y_lo): ``err_est``, ``resabs`` and ``tol`` are its, and ``panels_y``
    divides v. ``ax > bx`` negates, and where y_hi(x) < y_lo(x) that strip counts negatively
    (neither refused nor clamped). A limit that is not finite at a node makes its rectangle
    ``nonfinite``.
    ``backend="hip"``: the hipRTC-compiled gfx950 kernels (``ops.kernels.quad_expr2d_region``),
    one GPU. ``backend="cpu"``: the numpy model (``utils.adaptive_quad2d.region_model``) on
    ``expr_torch``'s evaluation of the three expressions; needs no GPU.
    Left out: limits in x that depend on y (swap the names), infinite sides, parameter rows,
    more than one rank, the host engine."""
    ax, bx = float(ax), float(bx)
    if backend == "hip":
        from .ops import kernels

        r = kernels.quad_expr2d_region(expr, ax, bx, y_lo, y_hi, rtol=rtol, atol=atol,
                                       panels=(int(panels_x), int(panels_y)),
                                       max_depth=max_depth, max_intervals=max_intervals)
        fields = {k: getattr(r, k) for k in _ADAPT2D_FIELDS}
        ms = r.device_ms
    elif backend == "cpu":
        from ._native import native
        from .utils.adaptive_quad2d import region_model

        native().expr_region_source(expr, y_lo, y_hi)   # the refusals of the hip backend

        def f(x, y):
            return expr_torch(expr, torch.from_numpy(np.ascontiguousarray(x)),
                              torch.from_numpy(np.ascontiguousarray(y))).numpy()

        def limit(which):
            return lambda x: expr_torch(which, torch.from_numpy(np.ascontiguousarray(x))).numpy()

        t0 = time.perf_counter()
        r = region_model(f, limit(y_lo), limit(y_hi), ax, bx, rtol=rtol, atol=atol,
                         panels_x=int(panels_x), panels_y=int(panels_y),
                         max_depth=int(max_depth), max_intervals=int(max_intervals))
        ms = (time.perf_counter() - t0) * 1e3
        fields = {k: r[k] for k in _ADAPT2D_FIELDS}
    else:
        raise ValueError("integrate_expr2d_region backend must be 'hip' or 'cpu'")
    return AdaptiveRegionResult(**fields, device_ms=ms, expr=expr, ax=ax, bx=bx, ay=0.0, by=1.0,
                                backend=backend, y_lo=y_lo, y_hi=y_hi)


@dataclasses.dataclass
class AdaptiveSweepResult:
    """Per row (numpy arrays of K entries, fields as in ``AdaptiveResult``), then the call."""
    value: "np.ndarray"
    err_est: "np.ndarray"
    resabs: "np.ndarray"
    tol: "np.ndarray"          # the row's last tolerance, max(atol, rtol * |its value so far|)
    converged: "np.ndarray"    # bool
    evals: "np.ndarray"
    rounds: "np.ndarray"       # the last round in which the row had an active interval
    intervals: "np.ndarray"
    splits: "np.ndarray"
    floor: "np.ndarray"
    forced: "np.ndarray"
    nonfinite: "np.ndarray"
    capped: "np.ndarray"       # bool: the row's partition would have passed max_intervals
    call_rounds: int           # the maximum over rows
    call_evals: int            # the sum over rows
    peak: int                  # the longest whole list
    device_ms: float           # the rounds (hip) or the model's run (cpu), in ms
    expr: str
    a: float
    b: float
    backend: str
    range: str = "finite"      # of the shared range, as in ``AdaptiveResult``

    def as_dict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}


_ADAPT_SWEEP_CALL_FIELDS = ("call_rounds", "call_evals", "peak", "range")


def integrate_expr_adaptive_sweep(expr: str, params, a: float, b: float, rtol: float = 1e-10,
                                  atol: float = 0.0, panels: int = 0, max_depth: int = 60,
                                  max_intervals: int = 0, max_total: int = 1 << 22,
                                  backend: str = "hip") -> AdaptiveSweepResult:
    """The integrals of f(x, p0, ..., p{nparams-1}) on a shared [a, b] for the K rows of
    ``params`` (K x nparams), each row to its own tolerance max(atol, rtol * |its value|), with
    its own error estimate, ``converged`` flag and counters; the rows share the rounds, and a
    row's result does not depend on the rows that ride along. ``panels`` and ``max_intervals``
    are per row (0: derived), ``max_total`` bounds all rows' intervals together.
    ``backend="hip"``: the hipRTC-compiled gfx950 kernels (``ops.kernels.quad_expr_sweep``),
    one GPU. ``backend="cpu"``: the numpy model (``utils.adaptive_quad.adaptive_sweep_model``)
    on ``expr_torch``'s subset of expressions; needs no GPU. One rank. A shared range (numbers
    for ``a`` and ``b``) may have infinite ends as for ``integrate_expr_adaptive``. With a
    sequence of K numbers for ``a`` or ``b`` (a number beside one is repeated) row r runs on
    its own finite [a[r], b[r]], bitwise as the one-row call on that range would; the result's
    ``a`` and ``b`` are then arrays."""
    from .utils.adaptive_quad import (SWEEP_ROW_FIELDS, adaptive_sweep_model,
                                      adaptive_sweep_ranges_model)

    ranged = np.ndim(a) != 0 or np.ndim(b) != 0
    if ranged:
        rows = len(params)
        a, b = (np.asarray(v, dtype=np.float64) if np.ndim(v) != 0 else np.full(rows, float(v))
                for v in (a, b))
    else:
        a, b = float(a), float(b)
    opts = dict(rtol=rtol, atol=atol, panels=int(panels), max_depth=int(max_depth),
                max_intervals=int(max_intervals), max_total=int(max_total))
    if not ranged:
        opts["unbounded"] = True
    if backend == "hip":
        from .ops import kernels

        r = kernels.quad_expr_sweep(expr, params, a, b, **opts)[0]
        fields = {k: getattr(r, k) for k in SWEEP_ROW_FIELDS + _ADAPT_SWEEP_CALL_FIELDS}
        ms = r.device_ms
    elif backend == "cpu":
        def f(x, *row):
            names = {f"p{j}": torch.tensor(float(v), dtype=torch.float64)
                     for j, v in enumerate(row)}
            return expr_torch(expr, torch.from_numpy(x), names=names).numpy()

        t0 = time.perf_counter()
        r = (adaptive_sweep_ranges_model if ranged else adaptive_sweep_model)(f, params, a, b,
                                                                              **opts)
        ms = (time.perf_counter() - t0) * 1e3
        r.setdefault("range", "finite")
        fields = {k: r[k] for k in SWEEP_ROW_FIELDS + _ADAPT_SWEEP_CALL_FIELDS}
    else:
        raise ValueError("integrate_expr_adaptive_sweep backend must be 'hip' or 'cpu'")
    return AdaptiveSweepResult(**fields, device_ms=ms, expr=expr, a=a, b=b, backend=backend)


@dataclasses.dataclass
class CurveResult:
    """Per point (numpy arrays of M + 1 entries; entry 0 is the start: 0, converged), the cells
    (``AdaptiveSweepResult``-like per-cell arrays in ``cells``), then the call."""
    x: "np.ndarray"
    value: "np.ndarray"        # F_j, the integral from x[0] to x[j]
    err_est: "np.ndarray"      # the sum of the cells' err_est before j
    tol: "np.ndarray"          # the sum of the cells' tolerances before j: err_est is held to it
    resabs: "np.ndarray"
    converged: "np.ndarray"    # bool: every cell before j converged
    cells: dict                # per cell: the fields of ``AdaptiveSweepResult``'s rows
    atol_cell: "np.ndarray"    # (atol * |x[c + 1] - x[c]|) / |x[M] - x[0]|
    total: float               # F_M
    call_rounds: int
    call_evals: int
    peak: int
    device_ms: float           # the rounds and the prefix (hip) or the model's run (cpu), in ms
    expr: str
    backend: str

    def as_dict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}


_CURVE_POINT_FIELDS = ("x", "value", "err_est", "tol", "resabs", "converged", "atol_cell",
                       "total", "call_rounds", "call_evals", "peak")


def integrate_expr_curve(expr: str, x, rtol: float = 1e-10, atol: float = 0.0, panels: int = 0,
                         max_depth: int = 60, max_intervals: int = 0, max_total: int = 1 << 22,
                         backend: str = "hip") -> CurveResult:
    """The running integral of f to a tolerance: F_j, the integral from x[0] to x[j], at every
    point of the caller's grid ``x`` (M + 1 strictly increasing or strictly decreasing numbers;
    F_0 = 0). Each cell [x[c], x[c + 1]] is integrated adaptively to max(atol_c, rtol * |its
    integral|) with atol_c its share of ``atol`` by length, so ``err_est[j]`` (the estimate of
    |F_j - truth|) is held to ``tol[j]`` <= atol + rtol * (the integral of |f| up to x[j]): a
    CDF is relatively accurate at every point, its far tail included. ``converged[j]`` says
    that every cell before x[j] converged; a capped or non-finite cell marks the points from it
    onwards and changes no point before it. ``panels`` and ``max_intervals`` are per cell (0:
    derived); ``max_total`` is dealt to the cells in equal parts, so a singular point inside a
    very fine grid caps its own cell: give such grids a larger ``max_total`` or fewer points.
    ``backend="hip"``: ``ops.kernels.quad_expr_curve``, one GPU. ``backend="cpu"``: the numpy
    model (``utils.adaptive_quad.adaptive_curve_model``) on ``expr_torch``'s subset of
    expressions; needs no GPU."""
    from .utils.adaptive_quad import SWEEP_ROW_FIELDS, adaptive_curve_model

    opts = dict(rtol=rtol, atol=atol, panels=int(panels), max_depth=int(max_depth),
                max_intervals=int(max_intervals), max_total=int(max_total))
    if backend == "hip":
        from .ops import kernels

        r = kernels.quad_expr_curve(expr, x, **opts)[0]
        fields = {k: getattr(r, k) for k in _CURVE_POINT_FIELDS}
        cells = {k: getattr(r.cells, k) for k in SWEEP_ROW_FIELDS}
        ms = r.device_ms
    elif backend == "cpu":
        def f(t):
            return expr_torch(expr, torch.from_numpy(np.ascontiguousarray(t))).numpy()

        t0 = time.perf_counter()
        r = adaptive_curve_model(f, x, **opts)
        ms = (time.perf_counter() - t0) * 1e3
        fields = {k: r[k] for k in _CURVE_POINT_FIELDS}
        cells = {k: r["cells"][k] for k in SWEEP_ROW_FIELDS}
    else:
        raise ValueError("integrate_expr_curve backend must be 'hip' or 'cpu'")
    return CurveResult(**fields, cells=cells, device_ms=ms, expr=expr, backend=backend)


@dataclasses.dataclass
class LatticeResult:
    value: float
    err_est: float          # one standard error over the shifts, not a bound; inf for one shift
    estimates: list         # est_r, one per shift
    m: int                  # the (last) level: n = 2^m points per shift
    n: int
    shifts: int
    evals: int              # shifts x points, every level counted
    levels: int
    converged: bool         # a tolerance was asked and met
    device_ms: float        # the kernels (hip) or the model's run (cpu), in ms
    expr: str
    box: list
    periodic: bool
    backend: str

    def as_dict(self) -> dict:
        return dataclasses.asdict(self)


def integrate_expr_nd(expr: str, box, m: int | None = None, rtol: float | None = None,
                      atol: float = 0.0, shifts: int = 16, seed: int = 0, periodic: bool = False,
                      z=None, backend: str = "hip", m_min: int = 12,
                      m_max: int | None = None) -> LatticeResult:
    """The integral of any f(x0, ..., x{d-1}) given as one C++ expression over a box
    ``[(a0, b0), ...]`` of 1 <= d <= 16 sides, by a randomly shifted rank-1 lattice rule with
    n = 2^m points and ``shifts`` random shifts: the value, ``err_est`` (one standard error over
    the shifts) and the shifts' estimates. With ``m`` the rule of that level (``z``: its
    generating vector; default: the built-in Korobov vector of m = 10..26). With ``rtol`` and /
    or ``atol`` instead, m walks from ``m_min`` to ``m_max`` and stops at the first level whose
    err_est <= max(atol, rtol * |value|); ``converged`` says whether one did. The tent transform
    is applied unless ``periodic``. ``backend="hip"``: the hipRTC-compiled gfx950 kernels
    (``ops.kernels.lattice_expr``), one GPU. ``backend="cpu"``: the numpy model of the same rule
    (``utils.lattice_rule``) on ``expr_torch``'s evaluation of the expression (its arithmetic
    subset); needs no GPU."""
    box = [(float(lo), float(hi)) for lo, hi in box]
    walk = rtol is not None or (atol is not None and atol > 0.0)
    if (m is None) != walk:
        raise ValueError("integrate_expr_nd takes a level m, or a tolerance (rtol and / or atol) "
                         "to walk m to, not both and not neither")
    if backend == "hip":
        from .ops import kernels

        r, _ = kernels.lattice_expr(expr, box, m=m, rtol=rtol, atol=atol, shifts=shifts,
                                    seed=seed, periodic=periodic, z=z, m_min=m_min, m_max=m_max)
        fields = dict(value=r.value, err_est=r.err_est, estimates=r.estimates.tolist(), m=r.m,
                      n=r.n, shifts=r.shifts, evals=r.evals, levels=r.levels,
                      converged=r.converged)
        ms = r.device_ms
    elif backend == "cpu":
        from .utils import lattice_rule

        def f(x):
            cols = {f"x{j}": torch.from_numpy(np.ascontiguousarray(x[:, j]))
                    for j in range(x.shape[1])}
            return expr_torch(expr, cols["x0"], names=cols).numpy()

        t0 = time.perf_counter()
        if walk:
            if z is not None:
                raise ValueError("lattice: a walk over m takes the built-in vectors (z belongs "
                                 "to one m)")
            r = lattice_rule.lattice_to_tolerance(f, box, rtol=rtol or 0.0, atol=atol or 0.0,
                                                  m_min=m_min, m_max=m_max, shifts=shifts,
                                                  seed=seed, periodic=periodic)
        else:
            r = lattice_rule.lattice_model(f, box, int(m), shifts=shifts, seed=seed,
                                           periodic=periodic, z=z)
        ms = (time.perf_counter() - t0) * 1e3
        fields = dict(value=r["value"], err_est=r["err_est"],
                      estimates=r["estimates"].tolist(), m=r["m"], n=r["n"],
                      shifts=int(r["shifts"].shape[0]), evals=int(r["evals"]),
                      levels=r["levels"], converged=r["converged"])
    else:
        raise ValueError("integrate_expr_nd backend must be 'hip' or 'cpu'")
    return LatticeResult(**fields, device_ms=ms, expr=expr, box=box, periodic=bool(periodic),
                         backend=backend)
