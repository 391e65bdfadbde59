"""Tensor-level entry points to the gfx950 HIP kernels.

Every function takes/returns ``torch`` tensors on a HIP device and launches the native
kernel on the current torch stream (so it composes with torch.distributed collectives and
torch.cuda graphs). There is no fallback: a CPU tensor or a missing extension is an error.

Kernel sources: csrc/kernels/{riemann,table,scan,selftest}.hip.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .._native import native
from ..models.integrands import IntegrandSpec

_RULE_OFF = {"left": 0.0, "mid": 0.5, "right": 1.0}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check(t: torch.Tensor, dtype=torch.float64, name: str = "tensor") -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a HIP device (got {t.device})")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("HIP device required (torch.cuda.is_available() is False)")
    return torch.device("cuda", torch.cuda.current_device())


def _enums(dtype: str, div: str):
    m = native()
    return getattr(m.DType, dtype), getattr(m.DivMode, div)


def default_grid() -> int:
    m = native()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return m.default_riemann_grid(cus, 32)


def riemann_partials(spec: IntegrandSpec, n: int, rule: str = "left", dtype: str = "fp64",
                     div: str = "series_exact", grid: int | None = None, i_begin: int = 0,
                     n_local: int | None = None, tile: str = "auto") -> torch.Tensor:
    """Per-workgroup unscaled partial sums of f over samples [i_begin, i_begin+n_local).
    ``tile``: the tile form of the fp64 series_exact pi4 kernels, auto | short | long."""
    m = native()
    dev = _device()
    grid = grid or default_grid()
    n_local = n if n_local is None else n_local
    h = (spec.b - spec.a) / n
    partials = torch.empty(grid, dtype=torch.float64, device=dev)
    table = _table_tensor(spec, dev)
    dt, dv = _enums(dtype, div)
    m.launch_riemann_partials(spec.native_id, spec.a, h, _RULE_OFF[rule], i_begin, n_local,
                              list(spec.coef), spec.p0, spec.p1, dt, dv, grid,
                              table.data_ptr() if table is not None else 0,
                              table.numel() if table is not None else 0,
                              partials.data_ptr(), _stream(), tile)
    return partials


_TABLE_CACHE: dict = {}


def _table_tensor(spec: IntegrandSpec, dev: torch.device):
    if spec.name != "table":
        return None
    key = (dev.index, spec.table)  # per table: a second table must not get the first's tensor
    t = _TABLE_CACHE.get(key)
    if t is None:
        t = torch.tensor(spec.native_table(), dtype=torch.float64, device=dev)
        _TABLE_CACHE[key] = t
    return t


def finalize(partials: torch.Tensor, scale: float, out: torch.Tensor | None = None) -> torch.Tensor:
    _check(partials, name="partials")
    out = torch.empty(1, dtype=torch.float64, device=partials.device) if out is None else out
    native().launch_finalize(partials.data_ptr(), partials.numel(), scale, out.data_ptr(), _stream())
    return out


def unset_slots(n: int, device) -> torch.Tensor:
    """n fp64 write-once slots in their unset state (csrc/include/miint/handoff.hpp): what the
    one-launch reductions hand partials over in; the consuming workgroup re-arms them."""
    word = native().UNSET_SLOT_WORD
    bits = (word << 32) | word
    return torch.full((n,), bits - (1 << 64), dtype=torch.int64, device=device).view(torch.float64)


class FusedWorkspace:
    """Partials (write-once slots) + ticket for the one-launch reduction; reuse across
    calls (graph-safe: the kernel re-arms both)."""

    def __init__(self, grid: int, device: torch.device | None = None):
        dev = device or _device()
        self.grid = grid
        self.partials = unset_slots(grid, dev)
        self.ticket = torch.zeros(native().TICKET_WORDS, dtype=torch.int32, device=dev)


def riemann(spec: IntegrandSpec, n: int, rule: str = "left", dtype: str = "fp64",
            div: str = "series_exact", grid: int | None = None, i_begin: int = 0,
            n_local: int | None = None, out: torch.Tensor | None = None,
            workspace: FusedWorkspace | None = None, fused: bool = True,
            tile: str = "auto") -> torch.Tensor:
    """h * scale * sum f over this launch's samples, as a 1-element fp64 device tensor."""
    m = native()
    dev = _device()
    grid = grid or (workspace.grid if workspace else default_grid())
    n_local = n if n_local is None else n_local
    h = (spec.b - spec.a) / n
    scale = h * spec.scale
    out = torch.empty(1, dtype=torch.float64, device=dev) if out is None else out
    if not fused:
        p = riemann_partials(spec, n, rule, dtype, div, grid, i_begin, n_local, tile)
        return finalize(p, scale, out)
    ws = workspace or FusedWorkspace(grid, dev)
    table = _table_tensor(spec, dev)
    dt, dv = _enums(dtype, div)
    m.launch_riemann_fused(spec.native_id, spec.a, h, _RULE_OFF[rule], i_begin, n_local,
                           list(spec.coef), spec.p0, spec.p1, dt, dv, ws.grid,
                           table.data_ptr() if table is not None else 0,
                           table.numel() if table is not None else 0,
                           ws.partials.data_ptr(), ws.ticket.data_ptr(), scale, out.data_ptr(),
                           _stream(), tile)
    return out


def point_values(spec: IntegrandSpec, n: int, rule: str = "left", div: str = "series",
                 i_begin: int = 0, n_local: int | None = None,
                 tile: str = "auto") -> torch.Tensor:
    """Every sample's f value exactly as the hot tile path computes it (validation)."""
    m = native()
    dev = _device()
    n_local = n if n_local is None else n_local
    out = torch.empty(n_local, dtype=torch.float64, device=dev)
    table = _table_tensor(spec, dev)
    m.launch_riemann_point_values(spec.native_id, spec.a, (spec.b - spec.a) / n, _RULE_OFF[rule],
                                  i_begin, n_local, list(spec.coef), spec.p0, spec.p1,
                                  getattr(m.DivMode, div),
                                  table.data_ptr() if table is not None else 0,
                                  table.numel() if table is not None else 0,
                                  out.data_ptr(), _stream(), tile)
    return out


def riemann_tile_len(spec: IntegrandSpec, n: int, rule: str = "left", dtype: str = "fp64",
                     div: str = "series_exact", i_begin: int = 0, n_local: int | None = None,
                     tile: str = "auto") -> int:
    """Samples per lane tile of the kernel a launch of these parameters runs (host only: a
    read-only view of the dispatcher, no device needed)."""
    m = native()
    n_local = n if n_local is None else n_local
    dt, dv = _enums(dtype, div)
    return m.riemann_tile_len(spec.native_id, spec.a, (spec.b - spec.a) / n, _RULE_OFF[rule],
                              i_begin, n_local, list(spec.coef), spec.p0, spec.p1, dt, dv, tile)


def pi4_recip_narrow(d: torch.Tensor) -> torch.Tensor:
    """The IEEE-division kIeee Pi4 tiles' reciprocal of every element of ``d`` (validation:
    bitwise 1 / d for 1 <= d <= 2**500 in fp64, 2**100 in fp32 — the fp32 tiles' form)."""
    f32 = d.dtype == torch.float32
    _check(d, dtype=torch.float32 if f32 else torch.float64, name="d")
    out = torch.empty_like(d)
    launch = native().launch_pi4_recip_narrow_f32 if f32 else native().launch_pi4_recip_narrow
    launch(d.data_ptr(), d.numel(), out.data_ptr(), _stream())
    return out


def pk_modifier_check(ac: torch.Tensor, ka: float, kb: float) -> torch.Tensor:
    """The packed-fp32 source modifiers of the long pi4 tile (validation): ``ac`` is n x 4 fp32
    (slope pair, centre pair); returns n x 16 fp32: columns 0..7 the residual pairs formed from
    one scalar pair (ka, kb) through op_sel and neg_hi, columns 8..15 the same from (k, -k)
    scalar pairs, in the order (ka, low), (kb, low), (ka, high), (kb, high)."""
    _check(ac, dtype=torch.float32, name="ac")
    if ac.dim() != 2 or ac.shape[1] != 4:
        raise ValueError("ac must be n x 4")
    out = torch.empty((ac.shape[0], 16), dtype=torch.float32, device=ac.device)
    native().launch_pk_modifier_check(ac.data_ptr(), ac.shape[0], float(ka), float(kb),
                                      out.data_ptr(), _stream())
    return out


def sum_array(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    _check(x, name="x")
    m = native()
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    grid = m.default_reduce_grid(cus)
    partials = torch.empty(grid, dtype=torch.float64, device=x.device)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    m.launch_sum_array(x.data_ptr(), x.numel(), scale, partials.data_ptr(), grid, out.data_ptr(),
                       _stream())
    return out


def profile_tensor(device=None) -> torch.Tensor:
    from ..models import integrands
    dev = device or _device()
    return _table_tensor(integrands.table(), torch.device(dev))


def _scan_table(table: torch.Tensor | None, dev) -> torch.Tensor:
    """The table a scan samples: the built-in profile, or a caller's contiguous fp64 device
    tensor of 2..2048 entries at unit spacing."""
    if table is None:
        return profile_tensor(dev)
    _check(table, name="table")
    if table.dim() != 1:
        raise ValueError("table must be one-dimensional")
    return table


def interp_fill(n: int, i0: int = 0, dt: float = 1e-4, out: torch.Tensor | None = None,
                table: torch.Tensor | None = None) -> torch.Tensor:
    dev = _device()
    tab = _scan_table(table, dev)
    out = torch.empty(n, dtype=torch.float64, device=dev) if out is None else out
    _check(out, name="out")
    native().launch_interp_fill(tab.data_ptr(), tab.numel(), dt, i0, n, out.data_ptr(), _stream())
    return out


def _scan_state(n: int, dev) -> torch.Tensor:
    nbytes = native().scan_state_bytes(n)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def inclusive_scan(x: torch.Tensor, carry: torch.Tensor | None = None,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """Single-pass decoupled look-back inclusive scan (fp64)."""
    _check(x, name="x")
    out = torch.empty_like(x) if out is None else out
    st = _scan_state(x.numel(), x.device)
    native().launch_inclusive_scan(x.data_ptr(), out.data_ptr(), x.numel(), st.data_ptr(),
                                   carry.data_ptr() if carry is not None else 0, _stream())
    _check_timeout(st)
    return out


def interp_scan(n: int, i0: int = 0, dt: float = 1e-4, window: tuple[int, int] | None = None,
                carry: torch.Tensor | None = None,
                table: torch.Tensor | None = None) -> torch.Tensor:
    """inclusive_scan(interp(profile, (i0+i)*dt)) fused in one pass."""
    dev = _device()
    tab = _scan_table(table, dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    st = _scan_state(n, dev)
    lo, hi = window if window is not None else (0, (1 << 64) - 1)
    native().launch_interp_scan(tab.data_ptr(), tab.numel(), dt, i0, n, lo, hi, out.data_ptr(),
                                st.data_ptr(), carry.data_ptr() if carry is not None else 0,
                                _stream())
    _check_timeout(st)
    return out


def trainscan(n: int, i0: int = 0, dt: float = 1e-4, window: tuple[int, int] | None = None,
              carries: torch.Tensor | None = None, algo: str = "fused",
              table: torch.Tensor | None = None):
    """Two-phase scan of the interpolated profile (csrc/kernels/trainscan.hip).

    Returns (vel, pos, totals): vel = running sum of the samples, pos = running sum of vel,
    totals = {T1, T2} (the slice's sample sum and vel sum without carries). `carries`
    (2-element device tensor {C1, C2}) shifts the slice as if it followed earlier ranks
    (algo="fused" only). algo="onepass": single pass with a decoupled look-back.
    algo="fold": the one-GPU form of "fused" that TrainScan runs without a communicator (the
    write kernel folds the per-block aggregates itself); it takes no carries, writes no totals
    (totals is None) and applies only to dt = 1/sps and at most 64 blocks of 256 tiles.
    `table`: the table to sample instead of the built-in profile."""
    if algo not in ("fused", "fold", "onepass"):
        raise ValueError("algo must be fused|fold|onepass")
    if algo == "onepass" and carries is not None:
        raise ValueError("the one-pass scan takes no carries (single-GPU form)")
    if algo == "fold" and carries is not None:
        raise RuntimeError("fold mode is single-GPU (no rank carries)")
    m = native()
    if algo == "fold" and not m.trainscan_fold_applies(dt, n):
        raise RuntimeError("fold mode needs dt = 1/sps and at most 64 blocks of 256 tiles")
    dev = _device()
    tab = _scan_table(table, dev)
    vel = torch.empty(n, dtype=torch.float64, device=dev)
    pos = torch.empty(n, dtype=torch.float64, device=dev)
    ws = torch.zeros(m.trainscan_workspace_bytes(n), dtype=torch.uint8, device=dev)  # zeroed once
    totals = torch.zeros(2, dtype=torch.float64, device=dev)
    lo, hi = window if window is not None else (0, (1 << 64) - 1)
    if algo == "onepass":
        m.launch_trainscan_onepass(tab.data_ptr(), tab.numel(), dt, i0, n, lo, hi, ws.data_ptr(),
                                   totals.data_ptr(), vel.data_ptr(), pos.data_ptr(), _stream())
        if m.trainscan_onepass_timeout(ws.data_ptr(), _stream()):
            raise RuntimeError("trainscan look-back spin limit hit")
        return vel, pos, totals
    m.launch_trainscan(tab.data_ptr(), tab.numel(), dt, i0, n, lo, hi, ws.data_ptr(),
                       totals.data_ptr(), carries.data_ptr() if carries is not None else 0,
                       vel.data_ptr(), pos.data_ptr(), _stream(), algo == "fold")
    return vel, pos, (None if algo == "fold" else totals)


def _check_timeout(state: torch.Tensor) -> None:
    flag = native().scan_timeout_flag(state.data_ptr(), _stream())
    if flag:
        raise RuntimeError("scan look-back spin limit hit (inter-workgroup hand-off failed)")


def add_carry(x: torch.Tensor, carry: torch.Tensor) -> torch.Tensor:
    _check(x, name="x")
    native().launch_add_carry(x.data_ptr(), x.numel(), carry.data_ptr(), _stream())
    return x


def outer_product(v: torch.Tensor) -> torch.Tensor:
    _check(v, name="v")
    n = v.numel()
    t = torch.empty((n, n), dtype=torch.float64, device=v.device)
    native().launch_outer_product(v.data_ptr(), n, t.data_ptr(), _stream())
    return t


def table2d(table: torch.Tensor, X: float, Y: float, gx: int, gy: int, row0: int = 0,
            row1: int | None = None, fused: bool = True) -> torch.Tensor:
    """Midpoint-rule integral of the bilinear interpolant of `table` (ny x nx) over
    [0,X]x[0,Y] on a gx x gy grid, sample rows [row0, row1) only. 1-element tensor.
    fused: one launch with the last-workgroup reduction; else partials + finalize."""
    _check(table, name="table")
    ny, nx = table.shape
    row1 = gy if row1 is None else row1
    m = native()
    grid = m.table2d_grid(nx, ny, X, Y, gx, gy, row0, row1)
    partials = (unset_slots(grid, table.device) if fused
                else torch.empty(grid, dtype=torch.float64, device=table.device))
    if not fused:
        m.launch_table2d_partials(table.data_ptr(), nx, ny, X, Y, gx, gy, row0, row1,
                                  partials.data_ptr(), _stream())
        return finalize(partials, 1.0)
    ticket = torch.zeros(m.TICKET_WORDS, dtype=torch.int32, device=table.device)
    out = torch.empty(1, dtype=torch.float64, device=table.device)
    m.launch_table2d_fused(table.data_ptr(), nx, ny, X, Y, gx, gy, row0, row1,
                           partials.data_ptr(), ticket.data_ptr(), out.data_ptr(), _stream())
    return out


def table2d_reference(table: torch.Tensor, X: float, Y: float, gx: int, gy: int,
                      row0: int = 0, row1: int | None = None, rows_per_chunk: int = 256) -> float:
    """Plain torch fp64 form of `table2d` (any device, CPU included): the same midpoint
    samples and bilinear blend, summed in row chunks of at most rows_per_chunk x gx."""
    ny, nx = table.shape
    row1 = gy if row1 is None else row1
    t = table.to(torch.float64)
    xs = (torch.arange(gx, dtype=torch.float64, device=t.device) + 0.5) * (X / gx) * ((nx - 1) / X)
    ix = xs.long().clamp(0, nx - 2)
    fx = (xs - ix).unsqueeze(0)
    total = 0.0
    for r in range(row0, row1, rows_per_chunk):
        rows = torch.arange(r, min(r + rows_per_chunk, row1), dtype=torch.float64, device=t.device)
        ys = (rows + 0.5) * (Y / gy) * ((ny - 1) / Y)
        iy = ys.long().clamp(0, ny - 2)
        fy = (ys - iy).unsqueeze(1)
        lo, hi = t[iy], t[iy + 1]
        top = lo[:, ix] + (lo[:, ix + 1] - lo[:, ix]) * fx
        bot = hi[:, ix] + (hi[:, ix + 1] - hi[:, ix]) * fx
        total += float((top + (bot - top) * fy).sum())
    return total * (X / gx) * (Y / gy)


def wave_ops(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(per-wave sums, per-wave inclusive scans) via the DPP primitives."""
    f32 = x.dtype == torch.float32
    _check(x, dtype=x.dtype, name="x")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError("wave_ops supports fp32/fp64")
    sums = torch.empty(math.ceil(x.numel() / 64), dtype=x.dtype, device=x.device)
    scan = torch.empty_like(x)
    native().selftest_wave_ops(x.data_ptr(), x.numel(), f32, sums.data_ptr(), scan.data_ptr(),
                               _stream())
    return sums, scan


def block_ops(x: torch.Tensor, block: int) -> tuple[torch.Tensor, torch.Tensor]:
    f32 = x.dtype == torch.float32
    _check(x, dtype=x.dtype, name="x")
    sums = torch.empty(math.ceil(x.numel() / block), dtype=x.dtype, device=x.device)
    scan = torch.empty_like(x)
    native().selftest_block_ops(x.data_ptr(), x.numel(), block, f32, sums.data_ptr(),
                                scan.data_ptr(), _stream())
    return sums, scan


_EXPR_CACHE: dict = {}


def riemann_expr(expr: str, a: float, b: float, n: int, rule: str = "left",
                 i_begin: int = 0, n_local: int | None = None) -> float:
    """Riemann sum of any f(x) given as one C++ expression over ``x`` (HIP device math:
    ``"exp(-x*x)"``, ``"sin(x)/x"``, ...), compiled for gfx950 at run time with hipRTC
    (csrc/runtime/expr.cpp) and cached per (expression, device). Every sample is evaluated
    in fp64; the value is h * sum over samples [i_begin, i_begin + n_local) of the n-sample
    rule on [a, b]. The reference hard-wires sin (riemann.cpp:37) and recompiles to change it.
    """
    m = native()
    dev = _device().index
    key = (expr, dev)
    ei = _EXPR_CACHE.get(key)
    if ei is None:
        ei = _EXPR_CACHE[key] = m.ExprIntegrator(expr, dev)
    n_local = n - i_begin if n_local is None else n_local
    return ei.integrate(float(a), float(b), int(n), getattr(m.Rule, rule), int(i_begin),
                        int(n_local))


_EXPR_SWEEP_CACHE: dict = {}


def _param_rows(params):
    """``params`` as a C-contiguous K x nparams float64 array (a list of K empty rows is
    K x 0, an empty sequence 0 x 0)."""
    import numpy as np

    p = np.asarray(params, dtype=np.float64)
    if p.ndim == 1 and p.size == 0:
        p = p.reshape(0, 0)
    if p.ndim != 2:
        raise ValueError("params must be K rows of nparams numbers (2-D)")
    return np.ascontiguousarray(p)


def riemann_expr_sweep(expr: str, params, a: float, b: float, n: int, rule: str = "left",
                       grid: int = 0, i_begin: int = 0,
                       n_local: int | None = None) -> torch.Tensor:
    """Riemann sums of f(x, p0, ..., p{nparams-1}) for K parameter rows in one launch:
    ``params`` is K x nparams (a list of rows or a 2-D float64 array), the expression may
    mention ``x`` and ``p0`` .. ``p7``. One hipRTC compile per (expression, nparams), cached
    with its module per device; the rows are kernel data, so a new row costs no compile
    (csrc/runtime/expr_sweep.cpp). Returns a 1-D fp64 tensor of the K values on the device;
    a row's value does not depend on the rows that ride along. No rows (K = 0): an empty
    tensor, nothing compiled or launched."""
    m = native()
    dev = _device()
    p = _param_rows(params)
    if p.shape[0] == 0:
        return torch.empty(0, dtype=torch.float64, device=dev)
    nparams = p.shape[1]
    key = (expr, int(nparams), dev.index, int(grid))
    es = _EXPR_SWEEP_CACHE.get(key)
    if es is None:
        es = _EXPR_SWEEP_CACHE[key] = m.ExprSweep(expr, int(nparams), dev.index, int(grid))
    n_local = n - i_begin if n_local is None else n_local
    vals = es.integrate(p, float(a), float(b), int(n), getattr(m.Rule, rule), int(i_begin),
                        int(n_local))
    return torch.as_tensor(vals, dtype=torch.float64).to(dev)


_EXPR2D_CACHE: dict = {}


def riemann_expr2d(expr: str, ax: float, bx: float, nx: int, ay: float, by: float, ny: int,
                   rule: str = "left", row_begin: int = 0, rows: int | None = None,
                   grid: int = 0) -> float:
    """Double Riemann sum of any f(x, y) given as one C++ expression over ``x`` and ``y``
    (``"exp(-(x*x+y*y))"``; it need not mention ``y``) on [ax, bx] x [ay, by]: nx x ny samples,
    the same rule on both axes, compiled for gfx950 with hipRTC (csrc/runtime/expr2d.cpp) and
    cached with its module per (expression, device, grid). The value is hx * hy * the sum over
    all nx columns of sample rows [row_begin, row_begin + rows) (default: the rows from
    row_begin on). ``grid``: the workgroup cap (0: 2048)."""
    m = native()
    dev = _device().index
    key = (expr, dev, int(grid))
    ei = _EXPR2D_CACHE.get(key)
    if ei is None:
        ei = _EXPR2D_CACHE[key] = m.ExprIntegrator2D(expr, dev, int(grid))
    rows = ny - row_begin if rows is None else rows
    return ei.integrate(float(ax), float(bx), int(nx), float(ay), float(by), int(ny),
                        getattr(m.Rule, rule), int(row_begin), int(rows))


_EXPR_ADAPT_CACHE: dict = {}


def quad_expr(expr: str, a: float, b: float, rtol: float = 1e-10, atol: float = 0.0,
              panels: int = 65536, max_depth: int = 60, max_intervals: int = 1 << 22,
              return_intervals: bool = False, unbounded: bool = False):
    """The integral of any f(x) given as one C++ expression over ``x`` on [a, b] to the
    tolerance max(atol, rtol * |value|): adaptive Gauss-Kronrod (7, 15) from ``panels`` equal
    intervals, bisected by rounds where the estimate misses its share (at most ``max_depth``
    times, ``max_intervals`` intervals in all), six hipRTC-compiled gfx950 kernels cached with
    their module per (expression, device) (csrc/runtime/expr_adaptive.cpp). Returns the native
    AdaptResult: value, err_est, resabs, tol, converged, evals, rounds, intervals, splits,
    floor, forced, nonfinite, capped, device_ms, range. With ``return_intervals`` also the final
    partition as two fp64 device tensors ``lo`` and ``hi``, running from a to b. With
    ``unbounded`` a and b may be infinite (refused otherwise): (a, inf), (-inf, b) and
    (-inf, inf) are mapped onto t in (0, 1] (miint/expr.hpp), the eval kernel's twin for the kind
    is compiled and loaded at the first such call, ``range`` names the kind, and the partition is
    that of [0, 1] in t, ascending (``utils.adaptive_quad.t_to_x`` gives the x)."""
    m = native()
    opt = m.AdaptOptions(float(rtol), float(atol), int(panels), int(max_depth),
                         int(max_intervals), bool(unbounded))
    m.adapt_check(float(a), float(b), opt)  # before any device call
    dev = _device()
    key = (expr, dev.index)
    ea = _EXPR_ADAPT_CACHE.get(key)
    if ea is None:
        ea = _EXPR_ADAPT_CACHE[key] = m.ExprAdaptive(expr, dev.index)
    if not return_intervals:
        return ea.integrate(float(a), float(b), opt)
    pairs = torch.empty((int(max_intervals), 2), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the rounds run on their own stream
    r = ea.integrate(float(a), float(b), opt, pairs.data_ptr(), int(max_intervals))
    pairs = pairs[:r.intervals]
    return r, pairs[:, 0].contiguous(), pairs[:, 1].contiguous()


_EXPR_OSC_CACHE: dict = {}


def quad_expr_osc(expr: str, a: float, b: float, omega: float, kind: str = "cos",
                  rtol: float = 1e-10, atol: float = 0.0, panels: int = 65536,
                  max_depth: int = 60, max_intervals: int = 1 << 22,
                  return_intervals: bool = False, tail_panels: int = 16, max_cycles: int = 50):
    """The integral of f(x) cos(omega x) (``kind="sin"``: f(x) sin(omega x)) on [a, b] to the
    tolerance max(atol, rtol * |value|), f one C++ expression over ``x`` and omega a number of
    the call: adaptive Filon-Clenshaw-Curtis (13, 25), the weight integrated exactly and only f
    interpolated, so the cost does not grow with omega. ``quad_expr``'s rounds and options around
    two hipRTC-compiled evaluation kernels, cached with their module per (expression, device)
    (csrc/runtime/expr_adaptive_osc.cpp). Both ends of every interval are evaluated: f must be
    finite on the closed range. Returns the native OscResult: AdaptResult's fields (evals counts
    25 per interval) and omega, kind, cycles, extrapolated, reason. With ``return_intervals``
    also the final partition as two fp64 device tensors ``lo`` and ``hi``, running from a to b.
    ``b = inf`` (a finite, omega != 0, atol > 0) is the Fourier tail: cycles of ``tail_panels``
    panels, at most ``max_cycles`` of them, extrapolated by Wynn's epsilon algorithm; it returns
    no partition."""
    import math

    m = native()
    a, b, omega = float(a), float(b), float(omega)
    tail = math.isinf(b) and b > 0 and math.isfinite(a)
    opt = m.AdaptOptions(float(rtol), float(atol), int(panels), int(max_depth),
                         int(max_intervals), False)
    topt = m.OscTailOptions(int(tail_panels), int(max_cycles))
    if kind not in ("cos", "sin"):
        raise ValueError(f"oscillatory: kind '{kind}' must be cos or sin")
    m.osc_check(a, b, omega, opt, tail, topt)  # before any device call
    if tail and return_intervals:
        raise ValueError("oscillatory: the Fourier tail returns no partition (return_intervals)")
    m.expr_osc_source(expr)                    # a refused expression too
    dev = _device()
    key = (expr, dev.index)
    eo = _EXPR_OSC_CACHE.get(key)
    if eo is None:
        eo = _EXPR_OSC_CACHE[key] = m.ExprAdaptiveOsc(expr, dev.index)
    if tail:
        return eo.integrate_tail(a, omega, kind, opt, topt)
    if not return_intervals:
        return eo.integrate(a, b, omega, kind, opt)
    pairs = torch.empty((int(max_intervals), 2), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the rounds run on their own stream
    r = eo.integrate(a, b, omega, kind, opt, pairs.data_ptr(), int(max_intervals))
    pairs = pairs[:r.intervals]
    return r, pairs[:, 0].contiguous(), pairs[:, 1].contiguous()


_EXPR_ADAPT2D_CACHE: dict = {}


def quad_expr2d(expr: str, ax: float, bx: float, ay: float, by: float, rtol: float = 1e-10,
                atol: float = 0.0, panels=64, max_depth: int = 60,
                max_intervals: int = 1 << 22, return_rects: bool = False):
    """The double integral of any f(x, y) given as one C++ expression over ``x`` and ``y`` on the
    finite rectangle [ax, bx] x [ay, by] to the tolerance max(atol, rtol * |value|): the tensor
    product of the Gauss-Kronrod (7, 15) pair (225 evaluations a rectangle) from ``panels`` equal
    rectangles (one number for both axes or a pair (panels_x, panels_y)), each bisected by rounds
    along the axis that carries more of its error where the estimate misses its share (at most
    ``max_depth`` times per axis, ``max_intervals`` rectangles in all), six hipRTC-compiled
    gfx950 kernels cached with their module per (expression, device)
    (csrc/runtime/expr_adaptive2d.cpp). Returns the native Adapt2DResult: value, err_est, resabs,
    tol, converged, evals, rounds, intervals, splits, splits_x, splits_y, floor, forced,
    nonfinite, capped, device_ms. With ``return_rects`` also the final partition as an fp64 device
    tensor [n, 4] of (x0, x1, y0, y1), ordered by (y0, x0)."""
    m = native()
    px, py = (panels, panels) if isinstance(panels, int) else panels
    opt = m.Adapt2DOptions(float(rtol), float(atol), int(px), int(py), int(max_depth),
                           int(max_intervals))
    m.adapt2d_check(float(ax), float(bx), float(ay), float(by), opt)  # before any device call
    dev = _device()
    key = (expr, dev.index)
    ea = _EXPR_ADAPT2D_CACHE.get(key)
    if ea is None:
        ea = _EXPR_ADAPT2D_CACHE[key] = m.ExprAdaptive2D(expr, dev.index)
    if not return_rects:
        return ea.integrate(float(ax), float(bx), float(ay), float(by), opt)
    rects = torch.empty((int(max_intervals), 4), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the rounds run on their own stream
    r = ea.integrate(float(ax), float(bx), float(ay), float(by), opt, rects.data_ptr(),
                     int(max_intervals))
    return r, rects[:r.intervals]


_EXPR_REGION_CACHE: dict = {}


def quad_expr2d_region(expr: str, ax: float, bx: float, y_lo: str, y_hi: str,
                       rtol: float = 1e-10, atol: float = 0.0, panels=64, max_depth: int = 60,
                       max_intervals: int = 1 << 22, return_rects: bool = False):
    """The double integral of f(x, y) over the region { ax <= x <= bx, y_lo(x) <= y <= y_hi(x) }
    to the tolerance max(atol, rtol * |value|): ``expr`` is one C++ expression over ``x`` and
    ``y``, ``y_lo`` and ``y_hi`` are C++ expressions over ``x`` alone. The region is mapped onto
    [ax, bx] x [0, 1] by y = y_lo + (y_hi - y_lo) v and ``quad_expr2d``'s rounds run on the
    mapped integrand f (y_hi - y_lo), the evaluation kernel replaced by its twin
    (csrc/runtime/expr_adaptive_region.cpp); the options are ``quad_expr2d``'s. Where
    y_hi(x) < y_lo(x) that strip counts negatively. One hipRTC compile and one module per
    (expr, y_lo, y_hi, device), cached. Returns the native Adapt2DResult; err_est, resabs and tol
    are those of the mapped integrand. With ``return_rects`` also the final partition as an fp64
    device tensor [n, 4] of (x0, x1, v0, v1) in the mapped variables, ordered by (v0, x0)
    (``utils.adaptive_quad2d.region_corners`` turns them into y)."""
    m = native()
    px, py = (panels, panels) if isinstance(panels, int) else panels
    opt = m.Adapt2DOptions(float(rtol), float(atol), int(px), int(py), int(max_depth),
                           int(max_intervals))
    m.adapt2d_check(float(ax), float(bx), 0.0, 1.0, opt)  # before any device call
    m.expr_region_source(expr, y_lo, y_hi)                # a refused expression too
    dev = _device()
    key = (expr, y_lo, y_hi, dev.index)
    ea = _EXPR_REGION_CACHE.get(key)
    if ea is None:
        ea = _EXPR_REGION_CACHE[key] = m.ExprAdaptiveRegion(expr, y_lo, y_hi, dev.index)
    if not return_rects:
        return ea.integrate(float(ax), float(bx), opt)
    rects = torch.empty((int(max_intervals), 4), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the rounds run on their own stream
    r = ea.integrate(float(ax), float(bx), opt, rects.data_ptr(), int(max_intervals))
    return r, rects[:r.intervals]


_EXPR_ADAPT_SWEEP_CACHE: dict = {}


def quad_expr_sweep(expr: str, params, a: float, b: float, rtol: float = 1e-10,
                    atol: float = 0.0, panels: int = 0, max_depth: int = 60,
                    max_intervals: int = 0, max_total: int = 1 << 22, unbounded: bool = False):
    """The integrals of f(x, p0, ..., p{nparams-1}) on [a, b] for K parameter rows, each row to
    its own tolerance max(atol, rtol * |value of that row|), in shared rounds: ``params`` is
    K x nparams as for ``riemann_expr_sweep``. Row by row the rule is ``quad_expr``'s, and a
    row's result is bitwise the same alone, in any batch and at any position
    (csrc/runtime/expr_adaptive_sweep.cpp). ``panels`` and ``max_intervals`` are per row
    (0: derived from the row count and ``max_total``, the capacity of the lists for all rows
    together). One hipRTC compile per (expression, nparams), cached with its module per device.
    Returns ``(result, values, err_est, converged)``: the native AdaptSweepResult (per-row
    arrays value, err_est, resabs, tol, converged, evals, rounds, intervals, splits, floor,
    forced, nonfinite, capped; for the call call_rounds, call_evals, peak, device_ms) and the
    first three of its per-row arrays as 1-D device tensors (fp64, fp64, bool). No rows: empty
    results, nothing compiled or launched. With ``unbounded`` the shared a and b may be infinite,
    as for ``quad_expr``; the result's ``range`` names the kind.

    Per-row ranges: with a sequence of K numbers for ``a`` or ``b`` (a scalar beside one is
    repeated) row r runs on its own [a[r], b[r]], bitwise as the one-row call on that range
    would; a[r] > b[r] negates that row, a[r] == b[r] gives it 0. Such ranges are finite."""
    import numpy as np

    m = native()
    p = _param_rows(params)
    rows, nparams = p.shape
    opt = m.AdaptSweepOptions(float(rtol), float(atol), int(panels), int(max_depth),
                              int(max_intervals), int(max_total), bool(unbounded))
    ranged = np.ndim(a) != 0 or np.ndim(b) != 0
    if ranged:
        lo, hi = (v if np.ndim(v) != 0 else np.full(rows, float(v)) for v in (a, b))
        lo, hi = (np.asarray(v, dtype=np.float64) for v in (lo, hi))
        if lo.ndim != 1 or hi.ndim != 1:
            raise ValueError("a and b must be numbers or 1-D sequences of one number per row")
        m.adapt_sweep_ranges_check(int(rows), int(nparams), int(p.size), lo, hi, opt)
    else:
        m.adapt_sweep_check(int(rows), int(nparams), int(p.size), float(a), float(b), opt)
    dev = _device()
    if rows == 0:
        r = m.AdaptSweepResult()
    else:
        key = (expr, int(nparams), dev.index)
        es = _EXPR_ADAPT_SWEEP_CACHE.get(key)
        if es is None:
            es = _EXPR_ADAPT_SWEEP_CACHE[key] = m.ExprAdaptiveSweep(expr, int(nparams), dev.index)
        r = (es.integrate_ranges(p, lo, hi, opt) if ranged
             else es.integrate(p, float(a), float(b), opt))
    return (r, torch.as_tensor(r.value, dtype=torch.float64).to(dev),
            torch.as_tensor(r.err_est, dtype=torch.float64).to(dev),
            torch.as_tensor(r.converged, dtype=torch.bool).to(dev))


_EXPR_ADAPT_CURVE_CACHE: dict = {}


def quad_expr_curve(expr: str, x, rtol: float = 1e-10, atol: float = 0.0, panels: int = 0,
                    max_depth: int = 60, max_intervals: int = 0, max_total: int = 1 << 22):
    """The running integral F_j of f from x[0] to x[j] on the caller's grid ``x`` (M + 1
    strictly increasing or strictly decreasing points), every cell [x[c], x[c + 1]] to its own
    tolerance max(atol_c, rtol * |its integral|), atol_c = (atol * |x[c + 1] - x[c]|) /
    |x[M] - x[0]|: the cells are the rows of a ranged sweep (``quad_expr_sweep``), each bitwise
    the one-row call on its range, and F is their prefix in a fixed order, formed on the device
    (miint/expr.hpp, ExprAdaptiveCurve). ``panels`` and ``max_intervals`` are per cell (0: the
    largest power of two with M * panels <= 65536, at least 1; ``max_total`` / M). Returns
    ``(result, values, err_est, tol, converged)``: the native AdaptCurveResult (per-point x,
    value, err_est, tol, resabs, converged; ``cells``, the per-cell AdaptSweepResult;
    ``atol_cell``; total, total_err_est, total_tol, total_resabs, unconverged; call_rounds,
    call_evals, peak, device_ms) and four of its per-point arrays as 1-D device tensors (fp64,
    fp64, fp64, bool) of M + 1 entries."""
    import numpy as np

    m = native()
    grid = np.asarray(x, dtype=np.float64)
    if grid.ndim != 1:
        raise ValueError("x must be a 1-D sequence of grid points")
    opt = m.AdaptSweepOptions(float(rtol), float(atol), int(panels), int(max_depth),
                              int(max_intervals), int(max_total), False)
    m.adapt_curve_check(grid, opt)
    dev = _device()
    key = (expr, dev.index)
    ec = _EXPR_ADAPT_CURVE_CACHE.get(key)
    if ec is None:
        ec = _EXPR_ADAPT_CURVE_CACHE[key] = m.ExprAdaptiveCurve(expr, dev.index)
    r = ec.integrate(grid, opt)
    return (r, torch.as_tensor(r.value, dtype=torch.float64).to(dev),
            torch.as_tensor(r.err_est, dtype=torch.float64).to(dev),
            torch.as_tensor(r.tol, dtype=torch.float64).to(dev),
            torch.as_tensor(r.converged, dtype=torch.bool).to(dev))


_EXPR_LATTICE_CACHE: dict = {}


def lattice_expr(expr: str, box, m: int | None = None, rtol: float | None = None,
                 atol: float = 0.0, shifts: int = 16, seed: int = 0, periodic: bool = False,
                 z=None, shift_words=None, begin: int = 0, count: int | None = None,
                 scale: float = 1.0, grid: int = 0, m_min: int = 12, m_max: int | None = None,
                 comm=None):
    """The integral of any f(x0, ..., x{d-1}) given as one C++ expression over the box
    ``[(a0, b0), ...]`` (d <= 16 sides) by a randomly shifted rank-1 lattice rule: n = 2^m
    points, ``shifts`` random shifts (or the explicit ``shift_words``, R x d uint32), the tent
    transform unless ``periodic``; three hipRTC-compiled gfx950 kernels cached with their module
    per (expression, d, periodic, device, grid) (csrc/runtime/expr_lattice.cpp). With ``m`` the
    rule of that level on points [begin, begin + count) (default: all), the ranks of ``comm``
    all-reducing their sums; with ``rtol`` / ``atol`` instead the walk of m from ``m_min`` to
    ``m_max``. Returns the native LatticeResult (value, err_est, estimates, m, n, shifts, evals,
    levels, converged, device_ms) and the estimates as an fp64 tensor on the host (the finish
    kernel stores them to pinned memory)."""
    mod = native()
    box = [(float(lo), float(hi)) for lo, hi in box]
    d = len(box)
    words = [] if shift_words is None else [int(w) for w in np.asarray(shift_words).ravel()]
    opt = mod.LatticeOptions(shifts=int(shifts), seed=int(seed), shift_words=words,
                             z=[] if z is None else [int(v) for v in z],
                             rtol=float(rtol or 0.0), atol=float(atol or 0.0), m_min=int(m_min),
                             m_max=int(m_max or 0))
    walk = m is None
    if walk:
        mod.lattice_check_walk(box, opt, float(scale))  # before any device call
    else:
        n = 1 << int(m) if 0 <= int(m) < 63 else 0
        mod.lattice_check(box, int(m), opt, int(begin),
                          max(n - int(begin), 0) if count is None else int(count), float(scale))
    dev = _device()
    key = (expr, d, bool(periodic), dev.index, int(grid))
    el = _EXPR_LATTICE_CACHE.get(key)
    if el is None:
        el = _EXPR_LATTICE_CACHE[key] = mod.ExprLattice(expr, d, bool(periodic), dev.index,
                                                        int(grid))
    if walk:
        r = el.integrate_to(box, opt, float(scale), comm)
    else:
        r = el.integrate(box, int(m), opt, int(begin), count, float(scale), comm)
    return r, torch.from_numpy(np.array(r.estimates, dtype=np.float64))


_EXPR_SCAN_CACHE: dict = {}


def riemann_expr_scan(expr: str, a: float, b: float, n: int, rule: str = "left", every: int = 1,
                      i_begin: int = 0, n_local: int | None = None,
                      out: torch.Tensor | None = None) -> tuple[torch.Tensor, float]:
    """Running integral of any f(x) given as one C++ expression over ``x``: F_i = h * sum of
    f(x_j) over samples i_begin <= j <= i of the n-sample rule on [a, b], for every sample i
    of [i_begin, i_begin + n_local) with (i + 1) % every == 0 (i the global index; every = 1:
    all of them). Three hipRTC-compiled kernels per expression, cached with their module per
    (expression, device): tile sums, tile prefix, one write pass (csrc/runtime/expr_scan.cpp);
    nothing but the written values touches HBM. Returns (a 1-D fp64 device tensor of the
    written values, the total h * sum over the slice). ``out``: a contiguous fp64 device
    tensor to write into (at least as many elements as values are written)."""
    values, r = _expr_scan(expr, a, b, n, rule, every, i_begin, n_local, out)
    return values, r["total"]


def _expr_scan(expr, a, b, n, rule, every, i_begin, n_local, out):
    """riemann_expr_scan's work: (values, ExprScan.run's record: total, outputs, device_ms)."""
    m = native()
    dev = _device()
    key = (expr, dev.index)
    es = _EXPR_SCAN_CACHE.get(key)
    if es is None:
        es = _EXPR_SCAN_CACHE[key] = m.ExprScan(expr, dev.index)
    n_local = n - i_begin if n_local is None else n_local
    count = m.expr_scan_outputs(int(i_begin), int(n_local), int(every))
    if out is None:
        out = torch.empty(count, dtype=torch.float64, device=dev)
    else:
        _check(out, dtype=torch.float64, name="out")
    torch.cuda.current_stream(dev).synchronize()  # the scan runs on its own stream
    r = es.run(float(a), float(b), int(n), getattr(m.Rule, rule), int(i_begin), int(n_local),
               int(every), out.data_ptr(), out.numel())
    return out[:count], r
