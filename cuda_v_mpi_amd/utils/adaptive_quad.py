"""The rule of the adaptive kernels (csrc/runtime/expr_adaptive.cpp, ExprAdaptive) in numpy:
the CPU model the device is held to.

Gauss-Kronrod (7, 15) on a list of intervals, bisection by rounds, the decisions of
miint/expr.hpp in the same order, on the doubles of the rule's own table (``gk15_nodes`` and
its weights) and at the nodes the kernels form (``gk15_abscissae``: fma(hw, t_j, c)). What the
model does not share with the device is the order of its sums (numpy's pairwise ``sum`` here,
butterflies and fma chains there) and the math library behind f, so a value agrees to rounding,
not bit for bit, and a decision on the border of a bound may fall the other way. The reference
that fixes bits, with the device's own order of every sum, is ``adaptive_exact.py`` beside it.

    r = adaptive_model(lambda x: 1.0 / (x * x + 1e-8), -1.0, 1.0, rtol=1e-10)
    r["value"], r["err_est"], r["converged"], r["lo"], r["hi"]

Infinite ranges (``unbounded=True``; miint/expr.hpp has the rule): the rounds run on t in
[0, 1] over g(t) = f(x(t)) / (t * t), with x and the divisor taken from the native
``adapt_range_map``, so f is evaluated at the device's bits. ``lo`` and ``hi`` are then the
partition in t, ascending; ``t_to_x`` gives the x.

    r = adaptive_model(lambda x: np.exp(-x * x), -np.inf, np.inf, unbounded=True)
    r["range"], t_to_x(-np.inf, np.inf, r["lo"])
"""
from __future__ import annotations

import numpy as np

FLOOR = 50.0 * 2.0 ** -52   # err <= FLOOR * R: the difference is rounding noise
DEFAULTS = dict(rtol=1e-10, atol=0.0, panels=65536, max_depth=60, max_intervals=1 << 22)


def check_options(a: float, b: float, rtol: float, atol: float, panels: int, max_depth: int,
                  max_intervals: int, unbounded: bool = False) -> None:
    """The refusals of ``adapt_check``, with the numbers named."""
    with np.errstate(invalid="ignore", over="ignore"):
        width_ok = bool(np.isfinite(np.float64(b) - np.float64(a)))
    if unbounded:
        if np.isnan(a) or np.isnan(b) or not (np.isinf(a) or np.isinf(b) or width_ok):
            raise ValueError(f"adaptive: a = {a:.17g} and b = {b:.17g} must not be NaN, and "
                             "b - a must be finite when both are")
    elif not (np.isfinite(a) and np.isfinite(b) and width_ok):
        raise ValueError(f"adaptive: a = {a:.17g} and b = {b:.17g} must be finite, and b - a too")
    if not (rtol >= 0 and atol >= 0 and np.isfinite(rtol) and np.isfinite(atol)
            and (rtol > 0 or atol > 0)):
        raise ValueError(f"adaptive: rtol = {rtol:.17g} and atol = {atol:.17g} must be finite "
                         "and >= 0, and not both 0")
    if not 1 <= max_intervals <= 1 << 26:
        raise ValueError(f"adaptive: max_intervals = {max_intervals} must be 1..2^26")
    if not 1 <= panels <= max_intervals:
        raise ValueError(f"adaptive: panels = {panels} must be 1..max_intervals = "
                         f"{max_intervals}")
    if not 0 <= max_depth <= 200:
        raise ValueError(f"adaptive: max_depth = {max_depth} must be 0..200")


def gk15(f, lo: np.ndarray, hi: np.ndarray):
    """K, err = |K - G| and R of every interval [lo_i, hi_i]: the centre first, then the pairs
    of nodes from the centre outwards, as the kernels add them."""
    from .._native import native

    m = native()
    t, wk, wg = m.gk15_nodes(), m.gk15_weights(), m.gk7_weights()
    x = m.gk15_abscissae(lo, hi)
    hw = 0.5 * (hi - lo)
    fx = np.asarray(f(x), dtype=np.float64) + np.zeros_like(x)
    assert t[7] == 0.0 and fx.shape == x.shape
    sk = wk[7] * fx[:, 7]
    sg = wg[3] * fx[:, 7]
    sa = wk[7] * np.abs(fx[:, 7])
    for j in range(1, 8):
        f1, f2 = fx[:, 7 - j], fx[:, 7 + j]
        sk = sk + wk[7 + j] * (f1 + f2)
        sa = sa + wk[7 + j] * (np.abs(f1) + np.abs(f2))
        if j % 2 == 0:
            sg = sg + wg[3 + j // 2] * (f1 + f2)
    k, g = hw * sk, hw * sg
    return k, np.abs(k - g), hw * sa


def range_kind(a: float, b: float) -> str:
    """'finite', 'upper', 'lower' or 'both': ``adapt_range`` (a == b and NaN ends: 'finite')."""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b) or a == b:
        return "finite"
    lo, hi = min(a, b), max(a, b)
    if np.isinf(lo) and np.isinf(hi):
        return "both"
    return "upper" if np.isinf(hi) else "lower" if np.isinf(lo) else "finite"


def t_to_x(a: float, b: float, t):
    """The x of every t of an unbounded run's partition, in the kernels' bits: a + (1 - t) / t
    for (a, inf), b - (1 - t) / t for (-inf, b), and for (-inf, inf) the positive one q =
    (1 - t) / t of the two abscissae q and -q. t = 0 is the infinite end. A finite range
    returns t."""
    from .._native import native

    t = np.asarray(t, dtype=np.float64)
    with np.errstate(divide="ignore"):
        x = native().adapt_range_map(float(a), float(b), t.ravel())[0]
    return x.reshape(t.shape)


def mapped_integrand(f, a: float, b: float):
    """g of miint/expr.hpp for the infinite range between a and b: g(t) = f(x) / (t * t), or
    (f(q) + f(-q)) / (t * t), with x, q and t * t from the native ``adapt_range_map``."""
    from .._native import native

    m = native()
    kind = range_kind(a, b)
    assert kind != "finite"

    def g(t):
        x, jac, x2 = (v.reshape(t.shape) for v in m.adapt_range_map(a, b, t.ravel()))
        if kind == "both":
            return (np.asarray(f(x), dtype=np.float64) + np.asarray(f(x2), dtype=np.float64)) / jac
        return np.asarray(f(x), dtype=np.float64) / jac

    return g


def adaptive_model(f, a: float, b: float, rtol: float = 1e-10, atol: float = 0.0,
                   panels: int = 65536, max_depth: int = 60,
                   max_intervals: int = 1 << 22, unbounded: bool = False) -> dict:
    """The integral of f on [a, b] by the rounds of ExprAdaptive. ``f`` maps an fp64 array to
    an fp64 array. Returns the fields of AdaptResult (``device_ms`` aside), ``peak`` (the
    longest active list) and the final partition ``lo``, ``hi`` running from a to b (for an
    infinite range, with ``unbounded``: the partition of [0, 1] in t, ascending)."""
    a, b = float(a), float(b)
    check_options(a, b, rtol, atol, panels, max_depth, max_intervals, unbounded)
    out = dict(value=0.0, err_est=0.0, resabs=0.0, tol=float(atol), converged=True, evals=0,
               rounds=0, intervals=0, splits=0, floor=0, forced=0, nonfinite=0, capped=False,
               peak=0, lo=np.empty(0), hi=np.empty(0), range="finite")
    if a == b:
        return out
    kind = range_kind(a, b)
    if kind != "finite":  # the same rounds on g over [0, 1], W = 1
        out = adaptive_model(mapped_integrand(f, a, b), 0.0, 1.0, rtol=rtol, atol=atol,
                             panels=panels, max_depth=max_depth, max_intervals=max_intervals)
        out["range"] = kind
        if a > b:
            out["value"] = -out["value"]
        return out
    swapped = a > b
    x0, x1 = (b, a) if swapped else (a, b)
    width = x1 - x0
    edges = x0 + (width * np.arange(panels + 1, dtype=np.float64)) / float(panels)
    edges[-1] = x1
    lo, hi = edges[:-1].copy(), edges[1:].copy()
    depth = np.zeros(panels, dtype=np.int64)
    s_acc = e_acc = r_acc = 0.0
    tol = float(atol)
    done_lo, done_hi = [], []
    with np.errstate(all="ignore"):
        while lo.size:
            n = lo.size
            out["rounds"] += 1
            out["evals"] += 15 * n
            out["peak"] = max(out["peak"], n)
            k, err, r = gk15(f, lo, hi)
            t = rtol * abs(s_acc + float(k.sum()))
            tol = float(atol) if atol > t else t          # a NaN sum: a NaN tolerance
            w = hi - lo
            c = lo + 0.5 * w
            nonfinite = ~(np.isfinite(k) & np.isfinite(err))
            within = ~nonfinite & ~(err > (tol * w) / width)
            floor = ~nonfinite & ~within & (err <= FLOOR * r)
            forced = (~nonfinite & ~within & ~floor
                      & ((depth >= max_depth) | (c == lo) | (c == hi)))
            split = ~(nonfinite | within | floor | forced)
            n_split = int(split.sum())
            out["nonfinite"] += int(nonfinite.sum())
            out["floor"] += int(floor.sum())
            out["forced"] += int(forced.sum())
            if out["intervals"] + (n - n_split) + 2 * n_split > max_intervals:
                out["capped"] = True   # nothing is split: the pending K and err join the totals
                s_acc += float(k[~split].sum()) + float(k[split].sum())
                e_acc += float(err[~split].sum()) + float(err[split].sum())
                r_acc += float(r[~split].sum())
                split = np.zeros(n, dtype=bool)
                n_split = 0
            else:
                s_acc += float(k[~split].sum())
                e_acc += float(err[~split].sum())
                r_acc += float(r[~split].sum())
            out["intervals"] += n - n_split
            out["splits"] += n_split
            done_lo.append(lo[~split])
            done_hi.append(hi[~split])
            cs = c[split]
            lo = np.stack([lo[split], cs], axis=1).ravel()
            hi = np.stack([cs, hi[split]], axis=1).ravel()
            depth = np.repeat(depth[split] + 1, 2)
    plo, phi = np.concatenate(done_lo), np.concatenate(done_hi)
    order = np.lexsort((phi, plo))
    plo, phi = plo[order], phi[order]
    if swapped:
        plo, phi = phi[::-1].copy(), plo[::-1].copy()
    out.update(value=-s_acc if swapped else s_acc, err_est=e_acc, resabs=r_acc, tol=tol,
               lo=plo, hi=phi)
    out["converged"] = bool(e_acc <= tol and not out["capped"] and out["nonfinite"] == 0)
    return out


# ------------------------------------------------------------------ sweeps: K rows of f(x, p)
SWEEP_DEFAULTS = dict(rtol=1e-10, atol=0.0, panels=0, max_depth=60, max_intervals=0,
                      max_total=1 << 22)
SWEEP_MAX_ROWS = 1 << 20
SWEEP_MAX_PARAMS = 8
SWEEP_INITIAL_TOTAL = 65536
SWEEP_MIN_PANELS = 16


def sweep_default_panels(rows: int) -> int:
    """``panels = 0``: the largest power of two p <= 65536 with rows * p <= 65536, at least 16."""
    p = DEFAULTS["panels"]
    while p > SWEEP_MIN_PANELS and rows * p > SWEEP_INITIAL_TOTAL:
        p >>= 1
    return p


def check_sweep_options(rows: int, nparams: int, param_count: int, a: float, b: float,
                        rtol: float = 1e-10, atol: float = 0.0, panels: int = 0,
                        max_depth: int = 60, max_intervals: int = 0,
                        max_total: int = 1 << 22, unbounded: bool = False) -> dict:
    """The refusals of ``adapt_sweep_check``, with its wording; returns ``panels`` and
    ``max_intervals`` with their zeros resolved."""
    what = "adaptive sweep: "
    if not 0 <= rows <= SWEEP_MAX_ROWS:
        raise ValueError(f"{what}rows = {rows} must be 0..2^20")
    if not 0 <= nparams <= SWEEP_MAX_PARAMS:
        raise ValueError(f"{what}nparams = {nparams} must be 0..{SWEEP_MAX_PARAMS}")
    if param_count != rows * nparams:
        raise ValueError(f"{what}{param_count} parameter values for {rows} rows of {nparams}")
    if not 1 <= max_total <= 1 << 26:
        raise ValueError(f"{what}max_total = {max_total} must be 1..2^26")
    k = max(rows, 1)
    if max_intervals == 0:
        max_intervals = max_total // k
    if panels == 0:
        panels = sweep_default_panels(k)
    if not 1 <= panels <= max_intervals:
        raise ValueError(f"{what}panels = {panels} must be 1..max_intervals = {max_intervals} "
                         "(per row)")
    if max_intervals > max_total // k:
        raise ValueError(f"{what}rows * max_intervals = {rows} * {max_intervals} passes "
                         f"max_total = {max_total}")
    check_options(a, b, rtol, atol, panels, max_depth, max_intervals, unbounded)
    return dict(panels=panels, max_intervals=max_intervals)


SWEEP_ROW_FIELDS = ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds",
                    "intervals", "splits", "floor", "forced", "nonfinite", "capped")


def adaptive_sweep_model(f, params, a: float, b: float, rtol: float = 1e-10, atol: float = 0.0,
                         panels: int = 0, max_depth: int = 60, max_intervals: int = 0,
                         max_total: int = 1 << 22, unbounded: bool = False) -> dict:
    """The integrals of f(x, *row) on [a, b] for every row of ``params`` (K x nparams) by the
    rounds of ExprAdaptiveSweep. A row's result does not depend on the rows that ride along, so
    this is ``adaptive_model`` row by row on the resolved options. Returns the per-row fields of
    AdaptSweepResult as arrays, ``peak_row`` (each row's longest list), and for the call
    ``call_rounds`` (the maximum), ``call_evals`` (the sum) and ``peak`` (the longest whole
    list: rows share rounds, so round t holds every row's t-th list), and ``range``."""
    p = np.asarray(params, dtype=np.float64)
    if p.ndim == 1 and p.size == 0:
        p = p.reshape(0, 0)
    if p.ndim != 2:
        raise ValueError("params must be K rows of nparams numbers (2-D)")
    rows, nparams = p.shape
    a, b = float(a), float(b)
    res = check_sweep_options(rows, nparams, p.size, a, b, rtol, atol, panels, max_depth,
                              max_intervals, max_total, unbounded)
    kind = range_kind(a, b)
    runs = []
    sizes: dict = {}
    for row in p:
        def frow(x, row=row):
            return f(x, *row)

        # an infinite range: the rounds see g on [0, 1], as adaptive_model would run them
        h = frow if kind == "finite" else mapped_integrand(frow, a, b)

        def counted(x, key=len(runs), h=h):
            sizes.setdefault(key, []).append(x.shape[0])
            return h(x)

        lo, hi = (a, b) if kind == "finite" else (0.0, 1.0)
        run = adaptive_model(counted, lo, hi, rtol=rtol, atol=atol, panels=res["panels"],
                             max_depth=max_depth, max_intervals=res["max_intervals"],
                             unbounded=unbounded)
        if kind != "finite" and a > b:
            run["value"] = -run["value"]
        runs.append(run)
    out = {}
    kinds = dict(converged=bool, capped=bool, value=np.float64, err_est=np.float64,
                 resabs=np.float64, tol=np.float64)
    for key in SWEEP_ROW_FIELDS:
        out[key] = np.array([r[key] for r in runs], dtype=kinds.get(key, np.int64))
    out["peak_row"] = np.array([r["peak"] for r in runs], dtype=np.int64)
    depth = max((len(v) for v in sizes.values()), default=0)
    whole = [sum(v[t] for v in sizes.values() if t < len(v)) for t in range(depth)]
    out["call_rounds"] = int(out["rounds"].max()) if rows else 0
    out["call_evals"] = int(out["evals"].sum())
    out["peak"] = max(whole, default=0)
    out["range"] = range_kind(a, b)
    out.update(res)
    return out


# ------------------------------------------------------------------ per-row ranges, curves
def check_sweep_ranges(rows: int, nparams: int, param_count: int, a, b, rtol: float = 1e-10,
                       atol: float = 0.0, panels: int = 0, max_depth: int = 60,
                       max_intervals: int = 0, max_total: int = 1 << 22,
                       unbounded: bool = False) -> dict:
    """The refusals of ``adapt_sweep_ranges_check``, with its wording and in its order; returns
    ``panels`` and ``max_intervals`` with their zeros resolved."""
    what = "adaptive sweep: "
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != (rows,) or b.shape != (rows,):
        raise ValueError(f"{what}{a.size} lower and {b.size} upper ends for {rows} rows")
    if unbounded:
        raise ValueError(f"{what}per-row ranges are finite: unbounded takes one shared range")
    res = check_sweep_options(rows, nparams, param_count, 0.0, 1.0, rtol, atol, panels,
                              max_depth, max_intervals, max_total)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(b - a)
    if not ok.all():
        r = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{what}row {r}: a = {a[r]:.17g} and b = {b[r]:.17g} must be finite, "
                         "and b - a too")
    return res


def adaptive_sweep_ranges_model(f, params, a, b, rtol: float = 1e-10, atol=0.0,
                                panels: int = 0, max_depth: int = 60, max_intervals: int = 0,
                                max_total: int = 1 << 22) -> dict:
    """``adaptive_sweep_model`` with row r on its own [a[r], b[r]]: ``adaptive_model`` row by row
    on the options resolved for all rows. ``atol`` is one number, or one per row (a curve's
    atol_c). A row with a[r] == b[r] is 0 with tol = atol, converged, no evaluations. Returns
    what ``adaptive_sweep_model`` returns, ``range`` aside."""
    p = np.asarray(params, dtype=np.float64)
    if p.ndim == 1 and p.size == 0:
        p = p.reshape(0, 0)
    if p.ndim != 2:
        raise ValueError("params must be K rows of nparams numbers (2-D)")
    rows, nparams = p.shape
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    atols = np.broadcast_to(np.asarray(atol, dtype=np.float64), (rows,))
    res = check_sweep_ranges(rows, nparams, p.size, a, b, rtol,
                             float(atols.max()) if rows else 0.0, panels, max_depth,
                             max_intervals, max_total)
    runs, sizes = [], []
    for k in range(rows):
        seen: list = []

        def counted(x, row=p[k], seen=seen):
            seen.append(x.shape[0])
            return f(x, *row)

        runs.append(adaptive_model(counted, float(a[k]), float(b[k]), rtol=rtol,
                                   atol=float(atols[k]), panels=res["panels"],
                                   max_depth=max_depth, max_intervals=res["max_intervals"]))
        sizes.append(seen)
    out = {}
    kinds = dict(converged=bool, capped=bool, value=np.float64, err_est=np.float64,
                 resabs=np.float64, tol=np.float64)
    for key in SWEEP_ROW_FIELDS:
        out[key] = np.array([r[key] for r in runs], dtype=kinds.get(key, np.int64))
    out["peak_row"] = np.array([r["peak"] for r in runs], dtype=np.int64)
    depth = max((len(v) for v in sizes), default=0)
    whole = [sum(v[t] for v in sizes if t < len(v)) for t in range(depth)]
    out["call_rounds"] = int(out["rounds"].max()) if rows else 0
    out["call_evals"] = int(out["evals"].sum())
    out["peak"] = max(whole, default=0)
    out.update(res)
    return out


CURVE_MAX_CELLS = 1 << 20


def curve_default_panels(cells: int) -> int:
    """A curve's ``panels = 0``: the largest power of two p <= 65536 with cells * p <= 65536, at
    least 1."""
    p = DEFAULTS["panels"]
    while p > 1 and cells * p > SWEEP_INITIAL_TOTAL:
        p >>= 1
    return p


def check_curve(x, rtol: float = 1e-10, atol: float = 0.0, panels: int = 0, max_depth: int = 60,
                max_intervals: int = 0, max_total: int = 1 << 22) -> dict:
    """The refusals of ``adapt_curve_check``, with its wording; returns the resolved ``panels``
    and ``max_intervals``."""
    what = "adaptive curve: "
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or not 2 <= x.size <= CURVE_MAX_CELLS + 1:
        raise ValueError(f"{what}{x.size} points: the grid must hold 2..2^20 + 1")
    if not np.isfinite(x).all():
        i = int(np.flatnonzero(~np.isfinite(x))[0])
        raise ValueError(f"{what}x[{i}] = {x[i]:.17g} must be finite")
    bad = ~(x[1:] > x[:-1]) if x[1] > x[0] else ~(x[1:] < x[:-1])
    if bad.any():
        i = int(np.flatnonzero(bad)[0]) + 1
        raise ValueError(f"{what}x[{i}] = {x[i]:.17g} after x[{i - 1}] = {x[i - 1]:.17g}: the "
                         "grid must be strictly increasing or strictly decreasing")
    with np.errstate(over="ignore"):
        if not np.isfinite(x[-1] - x[0]):
            raise ValueError(f"{what}x[0] = {x[0]:.17g} and x[M] = {x[-1]:.17g}: x[M] - x[0] "
                             "must be finite")
    cells = x.size - 1
    if panels == 0:
        panels = curve_default_panels(cells)
    return check_sweep_options(cells, 0, 0, 0.0, 1.0, rtol, atol, panels, max_depth,
                               max_intervals, max_total)


def curve_atol(x, atol: float) -> np.ndarray:
    """atol_c = (atol * |x[c + 1] - x[c]|) / |x[M] - x[0]|, in that order."""
    x = np.asarray(x, dtype=np.float64)
    return (atol * np.abs(np.diff(x))) / abs(x[-1] - x[0])


def adaptive_curve_model(f, x, rtol: float = 1e-10, atol: float = 0.0, panels: int = 0,
                         max_depth: int = 60, max_intervals: int = 0,
                         max_total: int = 1 << 22) -> dict:
    """The running integral F_j of f from x[0] to x[j] by the rule of ExprAdaptiveCurve: cell c
    is ``adaptive_model`` on [x[c], x[c + 1]] with atol_c, and the per-point value, err_est, tol
    and resabs are the cells' running sums (numpy's ``cumsum`` here, the device's fixed order
    there), ``converged`` whether every cell before the point converged. Returns those arrays
    (M + 1 entries), ``cells`` (the ranged sweep model's dict), ``atol_cell``, ``total`` and
    the call's ``call_rounds``, ``call_evals`` and ``peak``."""
    x = np.asarray(x, dtype=np.float64)
    res = check_curve(x, rtol, atol, panels, max_depth, max_intervals, max_total)
    atol_c = curve_atol(x, atol)
    cells = adaptive_sweep_ranges_model(lambda t: f(t), np.zeros((x.size - 1, 0)), x[:-1], x[1:],
                                        rtol=rtol, atol=atol_c, panels=res["panels"],
                                        max_depth=max_depth,
                                        max_intervals=res["max_intervals"], max_total=max_total)

    def running(v):
        return np.concatenate([[0.0], np.cumsum(v)])

    out = dict(x=x, value=running(cells["value"]), err_est=running(cells["err_est"]),
               tol=running(cells["tol"]), resabs=running(cells["resabs"]),
               converged=np.concatenate([[True], np.cumsum(~cells["converged"]) == 0]),
               cells=cells, atol_cell=atol_c)
    out["total"] = float(out["value"][-1])
    for key in ("call_rounds", "call_evals", "peak"):
        out[key] = cells[key]
    out.update(res)
    return out
