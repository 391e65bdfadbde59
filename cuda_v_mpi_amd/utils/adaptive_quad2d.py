"""The rule of the adaptive 2-D kernels (csrc/runtime/expr_adaptive2d.cpp, ExprAdaptive2D) in
numpy: the CPU model the device is held to.

The tensor product of the Gauss-Kronrod (7, 15) pair on a list of rectangles, each bisected
along the axis that carries more of its error, by rounds; the axis choice and the decisions of
miint/expr.hpp in the same order, on the doubles of the rule's own table (``gk15_nodes`` and its
weights) and at the nodes the kernels form (``gk15_abscissae`` per axis: fma(h, t, c)). As for
the 1-D model (``adaptive_quad``), what the model does not share with the device is the order
inside its sums (a product and an add where the kernels use one fma, numpy's pairwise ``sum``
over a round where the kernels use butterflies) and the math library behind f, so a value
agrees to rounding, not bit for bit, and a decision on the border of a bound may fall the other
way.

    r = adaptive2d_model(lambda x, y: 1.0 / np.sqrt(x * x + y * y), 0, 1, 0, 1, rtol=1e-8)
    r["value"], r["err_est"], r["converged"], r["splits_x"], r["splits_y"], r["rects"]

The rule takes its 225 values a rectangle from a callback (``product_rule``) and the rounds take
the rule as one (``rounds_model``), so the region between two curves (ExprAdaptiveRegion,
csrc/runtime/expr_adaptive_region.cpp) is the same model around other values: ``region_model``
maps y = g(x) + (h(x) - g(x)) v and shares the map's roundings with the kernel (the
subtraction, the fma, the product by h - g).

    r = region_model(lambda x, y: 1.0 + 0.0 * x, lambda x: -np.sqrt(1.0 - x * x),
                     lambda x: np.sqrt(1.0 - x * x), -1, 1)      # the unit disc's area
"""
from __future__ import annotations

import numpy as np

from .adaptive_quad import FLOOR

DEFAULTS = dict(rtol=1e-10, atol=0.0, panels_x=64, panels_y=64, max_depth=60,
                max_intervals=1 << 22)


def check_options(ax: float, bx: float, ay: float, by: float, rtol: float, atol: float,
                  panels_x: int, panels_y: int, max_depth: int, max_intervals: int) -> None:
    """The refusals of ``adapt2d_check``, with the numbers named."""
    what = "adaptive 2-D: "
    with np.errstate(invalid="ignore", over="ignore"):
        wx = np.float64(bx) - np.float64(ax)
        wy = np.float64(by) - np.float64(ay)
        area = wx * wy
    if not (np.isfinite(ax) and np.isfinite(bx) and np.isfinite(wx)):
        raise ValueError(f"{what}ax = {ax:.17g} and bx = {bx:.17g} must be finite, and bx - ax too")
    if not (np.isfinite(ay) and np.isfinite(by) and np.isfinite(wy)):
        raise ValueError(f"{what}ay = {ay:.17g} and by = {by:.17g} must be finite, and by - ay too")
    if not np.isfinite(area):
        raise ValueError(f"{what}the area (bx - ax) * (by - ay) = {float(area):.17g} must be "
                         "finite")
    if not (rtol >= 0 and atol >= 0 and np.isfinite(rtol) and np.isfinite(atol)
            and (rtol > 0 or atol > 0)):
        raise ValueError(f"{what}rtol = {rtol:.17g} and atol = {atol:.17g} must be finite "
                         "and >= 0, and not both 0")
    if not 1 <= max_intervals <= 1 << 26:
        raise ValueError(f"{what}max_intervals = {max_intervals} must be 1..2^26")
    if not (panels_x >= 1 and panels_y >= 1 and panels_x * panels_y <= max_intervals):
        raise ValueError(f"{what}panels_x * panels_y = {panels_x} * {panels_y} must be "
                         f"1..max_intervals = {max_intervals}, each factor at least 1")
    if not 0 <= max_depth <= 200:
        raise ValueError(f"{what}max_depth = {max_depth} must be 0..200 (per axis)")


def gk15x15(f, x0: np.ndarray, x1: np.ndarray, y0: np.ndarray, y1: np.ndarray):
    """K, err, ex, ey and R of every rectangle [x0_i, x1_i] x [y0_i, y1_i]: the rows' sums along
    x and then the rows themselves from the centre outwards, pair by pair, as the kernels add
    them. ``f(x, y)`` takes two arrays of one shape."""
    def values(x, y):
        xx = np.broadcast_to(x[:, None, :], (x.shape[0], 15, 15))   # [rect, row j, column i]
        yy = np.broadcast_to(y[:, :, None], (x.shape[0], 15, 15))
        return np.asarray(f(xx, yy), dtype=np.float64) + np.zeros(xx.shape)

    return product_rule(values, x0, x1, y0, y1)


def product_rule(values, x0: np.ndarray, x1: np.ndarray, y0: np.ndarray, y1: np.ndarray):
    """The rule of ``gk15x15`` on 225 values a rectangle that a callback supplies:
    ``values(x, y)`` takes the nodes of both axes (n x 15 each, ascending) and returns the
    n x 15 x 15 values summed, [rectangle, row j, column i]."""
    from .._native import native

    m = native()
    t, wk, wg = m.gk15_nodes(), m.gk15_weights(), m.gk7_weights()
    x = m.gk15_abscissae(x0, x1)            # n x 15, ascending
    y = m.gk15_abscissae(y0, y1)
    hx, hy = 0.5 * (x1 - x0), 0.5 * (y1 - y0)
    fx = values(x, y)
    assert t[7] == 0.0 and fx.shape == (x.shape[0], 15, 15)
    fa = np.abs(fx)
    # the row sums, every row at once: the centre column, then the pairs of columns outwards
    rk = wk[7] * fx[:, :, 7]
    rg = wg[3] * fx[:, :, 7]
    ra = wk[7] * fa[:, :, 7]
    for i in range(1, 8):
        f1, f2 = fx[:, :, 7 - i], fx[:, :, 7 + i]
        rk = rk + wk[7 + i] * (f1 + f2)
        ra = ra + wk[7 + i] * (fa[:, :, 7 - i] + fa[:, :, 7 + i])
        if i % 2 == 0:
            rg = rg + wg[3 + i // 2] * (f1 + f2)
    # the rows: the centre row, then the pairs of rows outwards
    kk, gk, aa = wk[7] * rk[:, 7], wk[7] * rg[:, 7], wk[7] * ra[:, 7]
    gg, kg = wg[3] * rg[:, 7], wg[3] * rk[:, 7]
    for j in range(1, 8):
        tk = rk[:, 7 - j] + rk[:, 7 + j]
        tg = rg[:, 7 - j] + rg[:, 7 + j]
        ta = ra[:, 7 - j] + ra[:, 7 + j]
        kk = kk + wk[7 + j] * tk
        gk = gk + wk[7 + j] * tg
        aa = aa + wk[7 + j] * ta
        if j % 2 == 0:
            gg = gg + wg[3 + j // 2] * tg
            kg = kg + wg[3 + j // 2] * tk
    s = hx * hy
    k = s * kk
    return k, np.abs(k - s * gg), np.abs(k - s * gk), np.abs(k - s * kg), s * aa


def first_rectangles(x0: float, x1: float, y0: float, y1: float, panels_x: int, panels_y: int):
    """The first list as ``miint_adapt2d_init`` forms it: x fastest, each axis's edges
    a + ((b - a) k) / panels with the last one b."""
    ex = x0 + ((x1 - x0) * np.arange(panels_x + 1, dtype=np.float64)) / float(panels_x)
    ey = y0 + ((y1 - y0) * np.arange(panels_y + 1, dtype=np.float64)) / float(panels_y)
    ex[-1], ey[-1] = x1, y1
    return (np.tile(ex[:-1], panels_y), np.tile(ex[1:], panels_y),
            np.repeat(ey[:-1], panels_x), np.repeat(ey[1:], panels_x))


def adaptive2d_model(f, ax: float, bx: float, ay: float, by: float, rtol: float = 1e-10,
                     atol: float = 0.0, panels_x: int = 64, panels_y: int = 64,
                     max_depth: int = 60, max_intervals: int = 1 << 22) -> dict:
    """The integral of f(x, y) over [ax, bx] x [ay, by] by the rounds of ExprAdaptive2D. ``f``
    maps two fp64 arrays of one shape to an fp64 array. Returns the fields of Adapt2DResult
    (``device_ms`` aside), ``peak`` (the longest active list) and the final partition ``rects``,
    an n x 4 array of (x0, x1, y0, y1) ordered by (y0, x0)."""
    return rounds_model(lambda *rects: gk15x15(f, *rects), ax, bx, ay, by, rtol, atol, panels_x,
                        panels_y, max_depth, max_intervals)


def rounds_model(rule, ax: float, bx: float, ay: float, by: float, rtol: float, atol: float,
                 panels_x: int, panels_y: int, max_depth: int, max_intervals: int) -> dict:
    """The rounds of ``adaptive2d_model`` around any rule: ``rule(x0, x1, y0, y1)`` returns K,
    err, ex, ey and R of every rectangle of a list."""
    ax, bx, ay, by = float(ax), float(bx), float(ay), float(by)
    panels_x, panels_y = int(panels_x), int(panels_y)
    check_options(ax, bx, ay, by, rtol, atol, panels_x, panels_y, max_depth, max_intervals)
    out = dict(value=0.0, err_est=0.0, resabs=0.0, tol=float(atol), converged=True, evals=0,
               rounds=0, intervals=0, splits=0, splits_x=0, splits_y=0, floor=0, forced=0,
               nonfinite=0, capped=False, peak=0, rects=np.empty((0, 4)))
    if ax == bx or ay == by:
        return out
    negate = (ax > bx) != (ay > by)
    bx0, bx1, by0, by1 = min(ax, bx), max(ax, bx), min(ay, by), max(ay, by)
    box_x, box_y = bx1 - bx0, by1 - by0
    x0, x1, y0, y1 = first_rectangles(bx0, bx1, by0, by1, panels_x, panels_y)
    dx = np.zeros(x0.size, dtype=np.int64)
    dy = np.zeros(x0.size, dtype=np.int64)
    s_acc = e_acc = r_acc = 0.0
    tol = float(atol)
    done = []
    with np.errstate(all="ignore"):
        while x0.size:
            n = x0.size
            out["rounds"] += 1
            out["evals"] += 225 * n
            out["peak"] = max(out["peak"], n)
            k, err, ex, ey, r = rule(x0, x1, y0, y1)
            t = rtol * abs(s_acc + float(k.sum()))
            tol = float(atol) if atol > t else t          # a NaN sum: a NaN tolerance
            wx, wy = x1 - x0, y1 - y0
            along_x = np.where(ex > ey, True, np.where(ey > ex, False,
                                                       wx * box_y >= wy * box_x))
            lo, hi = np.where(along_x, x0, y0), np.where(along_x, x1, y1)
            c = lo + 0.5 * (hi - lo)
            depth = np.where(along_x, dx, dy)
            nonfinite = ~(np.isfinite(k) & np.isfinite(err))
            within = ~nonfinite & ~(err > (tol * (wx * wy)) / (box_x * box_y))
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
            sx, sy = split & along_x, split & ~along_x
            out["intervals"] += n - n_split
            out["splits"] += n_split
            out["splits_x"] += int(sx.sum())
            out["splits_y"] += int(sy.sum())
            done.append(np.stack([x0[~split], x1[~split], y0[~split], y1[~split]], axis=1))
            # the children, in the parents' order: (lo, c), (c, hi) along the chosen axis
            ax_s, cs = along_x[split], c[split]
            px0, px1, py0, py1 = x0[split], x1[split], y0[split], y1[split]
            x0 = np.stack([px0, np.where(ax_s, cs, px0)], axis=1).ravel()
            x1 = np.stack([np.where(ax_s, cs, px1), px1], axis=1).ravel()
            y0 = np.stack([py0, np.where(ax_s, py0, cs)], axis=1).ravel()
            y1 = np.stack([np.where(ax_s, py1, cs), py1], axis=1).ravel()
            dx = np.repeat(dx[split] + ax_s, 2)
            dy = np.repeat(dy[split] + ~ax_s, 2)
    rects = np.concatenate(done)
    rects = rects[np.lexsort((rects[:, 0], rects[:, 2]))]
    out.update(value=-s_acc if negate else s_acc, err_est=e_acc, resabs=r_acc, tol=tol,
               rects=rects)
    out["converged"] = bool(e_acc <= tol and not out["capped"] and out["nonfinite"] == 0)
    return out


def region_values(f, g, h):
    """The 225 values a rectangle of (x, v) of the region rule (miint/expr.hpp,
    ExprAdaptiveRegion), as a callback for ``product_rule``: per x node g_i = g(x_i) and
    w_i = h(x_i) - g_i, per node pair y_ij = fma(w_i, v_j, g_i) and f(x_i, y_ij) * w_i, each
    rounded as the kernel rounds it."""
    from .._native import native

    def values(x, v):
        gx = np.asarray(g(x), dtype=np.float64) + np.zeros(x.shape)
        w = (np.asarray(h(x), dtype=np.float64) + np.zeros(x.shape)) - gx
        shape = (x.shape[0], 15, 15)                                  # [rect, row j, column i]
        xx = np.broadcast_to(x[:, None, :], shape)
        ww = np.broadcast_to(w[:, None, :], shape)
        yy = native().fma(ww, np.broadcast_to(v[:, :, None], shape),
                          np.broadcast_to(gx[:, None, :], shape))
        return (np.asarray(f(xx, yy), dtype=np.float64) + np.zeros(shape)) * ww

    return values


def region_model(f, g, h, ax: float, bx: float, rtol: float = 1e-10, atol: float = 0.0,
                 panels_x: int = 64, panels_y: int = 64, max_depth: int = 60,
                 max_intervals: int = 1 << 22) -> dict:
    """The integral of f(x, y) over { ax <= x <= bx, g(x) <= y <= h(x) } by the rounds of
    ExprAdaptiveRegion: ``adaptive2d_model``'s on [ax, bx] x [0, 1] in (x, v), the 225 values of
    a rectangle from ``region_values``. ``g`` and ``h`` map an fp64 array to one of its shape.
    The fields are those of ``adaptive2d_model``; ``rects`` holds (x0, x1, v0, v1) ordered by
    (v0, x0), and err_est, resabs and tol are those of the mapped integrand f (h - g). Where
    h < g the strip counts negatively."""
    values = region_values(f, g, h)
    return rounds_model(lambda *rects: product_rule(values, *rects), ax, bx, 0.0, 1.0, rtol, atol,
                        panels_x, panels_y, max_depth, max_intervals)


def region_corners(rects: np.ndarray, g, h) -> np.ndarray:
    """The corners in (x, y) of rectangles (x0, x1, v0, v1) of a region's partition: an
    n x 4 x 2 array of (x, y) at (x0, v0), (x1, v0), (x1, v1), (x0, v1), where
    y = g(x) + (h(x) - g(x)) v as the kernels form it."""
    from .._native import native

    rects = np.asarray(rects, dtype=np.float64).reshape(-1, 4)
    x = rects[:, [0, 1, 1, 0]]
    v = rects[:, [2, 2, 3, 3]]
    gx = np.asarray(g(x), dtype=np.float64) + np.zeros(x.shape)
    w = (np.asarray(h(x), dtype=np.float64) + np.zeros(x.shape)) - gx
    return np.stack([x, native().fma(w, v, gx)], axis=2)
