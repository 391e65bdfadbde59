"""Per-row ranges of ExprAdaptiveSweep and the running integral of ExprAdaptiveCurve bit for bit
on the host, on top of ``adaptive_exact.py``.

A ranged row is, by the sweep's contract, row 0 of the one-row call on its own range, so the
reference of a ranged call is ``adaptive_sweep_exact`` once per row; nothing of the rule is
restated here. What a ranged call adds is composed from the rows' runs:

  * the rows share rounds, so round t holds the t-th list of every row that is still active:
    ``lengths[t]`` is the sum of the rows' ``lengths[t]``, ``peak`` its maximum, ``call_rounds``
    the longest row's count, ``call_evals`` 15 per interval of all of them;
  * a row with a[r] == b[r] never reaches the device: 0, tol = atol, converged, no evaluations;
  * ``curve_prefix_exact``: miint_acurve_prefix's order. per = ceil(M / 256); thread t chains
    the cells [t per, min((t + 1) per, M)) from 0.0 in index order; the 256 runs' exclusive
    prefixes P_t are formed sequentially from 0.0; point j + 1 is P_t + (the chain through j).

As in adaptive_exact.py, f must be bit-reproducible for the comparison to mean anything.
"""
from __future__ import annotations

import numpy as np

from . import adaptive_exact as ax

BLOCK = 256
ROW_FIELDS = ax.ROW_FIELDS


def curve_atol(x, atol: float) -> np.ndarray:
    """atol_c = (atol * |x[c + 1] - x[c]|) / |x[M] - x[0]|, every operation rounded on its own in
    that order (the host forms it so in adapt_curve_atol)."""
    x = np.asarray(x, dtype=np.float64)
    return (np.float64(atol) * np.abs(x[1:] - x[:-1])) / abs(x[-1] - x[0])


def sweep_ranges_exact(f, params, a, b, rtol: float = 1e-10, atol=0.0, panels: int = 16,
                       max_depth: int = 60, max_intervals: int = 1 << 12) -> dict:
    """ExprAdaptiveSweep::integrate_ranges with ``panels`` and ``max_intervals`` given (per
    row). f(x, p0, ...) on arrays; ``atol`` is one number or one per row. Returns the per-row
    fields as arrays, ``lengths`` (the whole list of every round), ``call_rounds``,
    ``call_evals``, ``peak`` and ``row_lengths`` (each row's own list lengths)."""
    p = np.asarray(params, dtype=np.float64)
    rows = p.shape[0]
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    atols = np.broadcast_to(np.asarray(atol, dtype=np.float64), (rows,))
    runs = []
    for r in range(rows):
        if a[r] == b[r]:
            runs.append(dict(value=0.0, err_est=0.0, resabs=0.0, tol=float(atols[r]),
                             converged=True, evals=0, rounds=0, intervals=0, splits=0, floor=0,
                             forced=0, nonfinite=0, capped=False, lengths=[]))
            continue
        one = ax.adaptive_sweep_exact(f, p[r:r + 1], float(a[r]), float(b[r]), rtol=rtol,
                                      atol=float(atols[r]), panels=panels, max_depth=max_depth,
                                      max_intervals=max_intervals)
        run = {key: one[key][0] for key in ROW_FIELDS}
        run["lengths"] = one["lengths"]
        runs.append(run)
    kinds = dict(converged=bool, capped=bool, value=np.float64, err_est=np.float64,
                 resabs=np.float64, tol=np.float64)
    out = {key: np.array([run[key] for run in runs], dtype=kinds.get(key, np.int64))
           for key in ROW_FIELDS}
    depth = max((len(run["lengths"]) for run in runs), default=0)
    lengths = [sum(run["lengths"][t] for run in runs if t < len(run["lengths"]))
               for t in range(depth)]
    out.update(lengths=lengths, call_rounds=depth, call_evals=15 * sum(lengths),
               peak=max(lengths, default=0), row_lengths=[run["lengths"] for run in runs])
    return out


def curve_prefix_exact(v, per_of=None) -> np.ndarray:
    """miint_acurve_prefix on the cells' numbers v[0..M): the M + 1 points, point 0 being 0.0.
    ``per_of`` replaces per = ceil(M / 256) (for a test that must see the run bounds matter)."""
    v = np.asarray(v, dtype=np.float64)
    m = v.shape[0]
    per = (m + BLOCK - 1) // BLOCK if per_of is None else per_of(m)
    out = np.zeros(m + 1)
    with np.errstate(all="ignore"):
        prefix = 0.0
        for t in range(BLOCK):
            first = min(t * per, m)
            last = min(first + per, m)
            chain = 0.0
            for c in range(first, last):
                chain = chain + float(v[c])
                out[c + 1] = prefix + chain
            prefix = prefix + chain
    return out


def curve_unconverged_exact(converged) -> np.ndarray:
    """The cells before each point that did not converge (an integer prefix)."""
    bad = ~np.asarray(converged, dtype=bool)
    return np.concatenate([[0], np.cumsum(bad)]).astype(np.int64)


def curve_exact(f, x, rtol: float = 1e-10, atol: float = 0.0, panels: int = 16,
                max_depth: int = 60, max_intervals: int = 1 << 12) -> dict:
    """ExprAdaptiveCurve::integrate with ``panels`` and ``max_intervals`` given (per cell):
    ``cells`` (sweep_ranges_exact of the cells with atol_c), the per-point arrays ``value``,
    ``err_est``, ``tol``, ``resabs`` and ``converged``, and the call's counters."""
    x = np.asarray(x, dtype=np.float64)
    atol_c = curve_atol(x, atol)
    cells = sweep_ranges_exact(lambda t: f(t), np.zeros((x.shape[0] - 1, 0)), x[:-1], x[1:],
                               rtol=rtol, atol=atol_c, panels=panels, max_depth=max_depth,
                               max_intervals=max_intervals)
    out = dict(x=x, cells=cells, atol_cell=atol_c,
               converged=curve_unconverged_exact(cells["converged"]) == 0)
    for key in ("value", "err_est", "tol", "resabs"):
        out[key] = curve_prefix_exact(cells[key])
    for key in ("call_rounds", "call_evals", "peak", "lengths"):
        out[key] = cells[key]
    return out
