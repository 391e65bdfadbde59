"""The oscillatory integrator (csrc/runtime/expr_adaptive_osc.cpp, ExprAdaptiveOsc) in numpy:
the CPU model the device is held to.

Filon-Clenshaw-Curtis (13, 25) against cos(omega x) or sin(omega x) on a list of intervals,
bisected by ExprAdaptive's rounds. Everything the device computes with operations that IEEE
fixes is repeated here bit for bit: the nodes fma(hw, t_j, c), the fma chains of the five sums
in the order miint/expr.hpp states, the weights (``native().osc_weights``: the doubles of the
device's table, row d for par_d = omega hw0 2^-d), the block sums, the closing sum and the
prefix kernel's runs (``adaptive_exact``'s pieces), the decisions, the cap and the slots. What
is left to a math library is f itself and the one sincos(omega c) per interval. With omega = 0
that is sincos(0), which is exact, so for an f of exact operations the model and the device
agree on every bit; otherwise they agree to rounding.

    r = osc_model(lambda x: 1.0 / (1.0 + x * x), 0.0, 10.0, 1e4, "cos", rtol=1e-10, panels=64)
    r["value"], r["err_est"], r["converged"], r["partition"]

``osc_tail_model`` is the Fourier tail on (a, inf): the host loop of ``integrate_tail`` over
``osc_model``, with the native ``osc_epsilon``.
"""
from __future__ import annotations

import math

import numpy as np

from . import adaptive_exact as ax

EVALS = 25
TAIL_P = 0.9
TAIL_DEFAULTS = dict(panels=16, max_cycles=50)
DEFAULTS = dict(rtol=1e-10, atol=0.0, panels=65536, max_depth=60, max_intervals=1 << 22)


def _native():
    from .._native import native

    return native()


def check(a, b, omega, rtol, atol, panels, max_depth, max_intervals, tail=False,
          tail_panels=16, max_cycles=50):
    """``osc_check``: the native refusals, as ValueError."""
    m = _native()
    opt = m.AdaptOptions(float(rtol), float(atol), int(panels), int(max_depth),
                         int(max_intervals), False)
    try:
        m.osc_check(float(a), float(b), float(omega), opt, bool(tail),
                    m.OscTailOptions(int(tail_panels), int(max_cycles)))
    except RuntimeError as e:
        raise ValueError(str(e)) from None


class _Table:
    """The device table: row d holds the half tables for par0 2^-d, built when first needed."""

    def __init__(self, par0: float):
        self.par0, self.rows = par0, {}

    def row(self, d: int):
        if d not in self.rows:
            wc24, ws24, wc12, ws12 = _native().osc_weights(math.ldexp(self.par0, -d))
            self.rows[d] = (wc24[:13].copy(), ws24[:12].copy(), wc12[:7].copy(), ws12[:6].copy())
        return self.rows[d]

    def gather(self, depth: np.ndarray):
        out = [np.empty((depth.shape[0], k)) for k in (13, 12, 7, 6)]
        for d in np.unique(depth):
            sel = depth == d
            for dst, src in zip(out, self.row(int(d))):
                dst[sel] = src
        return out


def osc_rule(f, lo, hi, depth, omega: float, kind: str, table: _Table):
    """miint_osc_rule on every interval: K, err = |K - G|, R."""
    m = _native()
    fma = m.fma
    t, wcc = m.osc_nodes(), m.osc_cc_weights()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    wc24, ws24, wc12, ws12 = table.gather(np.asarray(depth))
    hw = 0.5 * (hi - lo)
    c = lo + hw

    def val(x):
        return np.asarray(f(x), dtype=np.float64) + np.zeros_like(x)

    f12 = val(c)
    ic24, ic12 = wc24[:, 12] * f12, wc12[:, 6] * f12
    is24 = is12 = None
    sa = wcc[12] * np.abs(f12)
    for j in range(11, -1, -1):
        fp, fm = val(fma(hw, t[j], c)), val(fma(hw, -t[j], c))
        s, d = fp + fm, fp - fm
        ic24 = fma(wc24[:, j], s, ic24)
        is24 = ws24[:, j] * d if is24 is None else fma(ws24[:, j], d, is24)
        if j % 2 == 0:
            ic12 = fma(wc12[:, j // 2], s, ic12)
            is12 = ws12[:, j // 2] * d if is12 is None else fma(ws12[:, j // 2], d, is12)
        sa = fma(wcc[j], np.abs(fp) + np.abs(fm), sa)
    p = omega * c
    e = fma(np.full_like(c, omega), c, -p)
    s0, c0 = np.sin(p), np.cos(p)
    sn, cs = fma(e, c0, s0), fma(-e, s0, c0)
    if kind == "cos":
        kv = hw * (cs * ic24 - sn * is24)
        gv = hw * (cs * ic12 - sn * is12)
    else:
        kv = hw * (sn * ic24 + cs * is24)
        gv = hw * (sn * ic12 + cs * is12)
    return kv, np.abs(kv - gv), hw * sa


def reason(r: dict) -> str:
    """``osc_reason``: why a finished finite run did not converge."""
    if r["converged"]:
        return ""
    if r["nonfinite"]:
        return (f"f was not finite on {r['nonfinite']} intervals (both ends of every interval "
                "are evaluated)")
    if r["capped"]:
        return "max_intervals was reached"
    if r["forced"]:
        return f"{r['forced']} intervals reached max_depth or could not be halved"
    return f"the rounding floor was reached on {r['floor']} intervals before the tolerance"


def _rounds(f, x0, x1, hw0, omega, kind, rtol, atol, panels, max_depth, max_intervals):
    """ExprAdaptive::rounds around the oscillatory rule on [x0, x1], x0 < x1."""
    width = x1 - x0
    table = _Table(omega * hw0)
    lo, hi = ax.init_edges(x0, x1, panels)
    depth = np.zeros(panels, dtype=np.int64)
    st = ax._Totals()
    done = np.full((max_intervals, 2), np.nan)
    out = dict(evals=0, rounds=0, capped=False, lengths=[], margin=math.inf)
    with np.errstate(all="ignore"):
        while True:
            n = lo.shape[0]
            assert 1 <= n <= max_intervals and out["rounds"] <= max_depth
            k, err, r = osc_rule(f, lo, hi, depth, omega, kind, table)
            sum_k = ax.close_sum(ax.block_sums(k))
            st.tol = ax._tolerance(rtol, atol, st.s, sum_k)
            w = hi - lo
            c = lo + 0.5 * w
            share = (st.tol * w) / width
            how = ax.decide(k, err, r, share, (depth >= max_depth) | (c == lo) | (c == hi))
            # how far the decisions are from their thresholds, relative (the tests ask > 1e-6)
            fin = np.isfinite(err) & (err > 0)
            if fin.any():
                near = [np.abs(err[fin] / share[fin] - 1.0)]
                beyond = fin & (err > share) & (r > 0)
                if beyond.any():
                    near.append(np.abs(err[beyond] / (ax.FLOOR * r[beyond]) - 1.0))
                out["margin"] = min(out["margin"], *(float(v.min()) for v in near))
            capped, base, _ = st.close_round(how, k, err, r, max_intervals)
            sp, child, slot = ax._slots(how == 5, capped, base)
            done[slot, 0], done[slot, 1] = lo[~sp], hi[~sp]
            out["rounds"] += 1
            out["evals"] += EVALS * n
            out["lengths"].append(n)
            if capped or not sp.any():
                out["capped"] = capped
                break
            nxt = 2 * int(sp.sum())
            nlo, nhi, nd = np.empty(nxt), np.empty(nxt), np.empty(nxt, dtype=np.int64)
            nlo[child], nhi[child] = lo[sp], c[sp]
            nlo[child + 1], nhi[child + 1] = c[sp], hi[sp]
            nd[child] = nd[child + 1] = depth[sp] + 1
            lo, hi, depth = nlo, nhi, nd
    done = done[:st.accepted]
    part = done[np.lexsort((done[:, 1], done[:, 0]))]
    out.update(value=st.s, err_est=st.e, resabs=st.r, tol=st.tol, intervals=st.accepted,
               splits=st.splits, floor=st.floor, forced=st.forced, nonfinite=st.nonfinite,
               partition=part, peak=max(out["lengths"]), max_depth_seen=int(depth.max()))
    out["converged"] = bool(st.e <= st.tol and not out["capped"] and st.nonfinite == 0)
    return out


def osc_model(f, a: float, b: float, omega: float, kind: str = "cos", rtol: float = 1e-10,
              atol: float = 0.0, panels: int = 65536, max_depth: int = 60,
              max_intervals: int = 1 << 22) -> dict:
    """The integral of f(x) cos(omega x) (or sin) on [a, b] as ExprAdaptiveOsc::integrate forms
    it. ``f`` maps an fp64 array to an fp64 array. Returns the fields of OscResult
    (``device_ms`` aside), the final partition running from a to b (n x 2), ``lengths`` (the
    list of every round), ``peak`` and ``margin``: the smallest relative distance of any
    decision from its threshold."""
    if kind not in ("cos", "sin"):
        raise ValueError(f"oscillatory: kind '{kind}' must be cos or sin")
    a, b, omega = float(a), float(b), float(omega)
    check(a, b, omega, rtol, atol, panels, max_depth, max_intervals)
    out = dict(value=0.0, err_est=0.0, resabs=0.0, tol=float(atol), converged=True, evals=0,
               rounds=0, intervals=0, splits=0, floor=0, forced=0, nonfinite=0, capped=False,
               range="finite", omega=omega, kind=kind, cycles=0, extrapolated=False, reason="",
               partition=np.empty((0, 2)), lengths=[], peak=0, margin=math.inf)
    if a == b:
        return out
    swapped = a > b
    x0, x1 = (b, a) if swapped else (a, b)
    hw0 = 0.5 * ((x1 - x0) / float(panels))
    out.update(_rounds(f, x0, x1, hw0, omega, kind, float(rtol), float(atol), int(panels),
                       int(max_depth), int(max_intervals)))
    if swapped:
        out["value"] = -out["value"]
        out["partition"] = out["partition"][::-1, ::-1].copy()
    out["reason"] = reason(out)
    return out


def osc_tail_model(f, a: float, omega: float, kind: str = "cos", atol: float = 1e-10,
                   rtol: float = 0.0, max_depth: int = 60, max_intervals: int = 1 << 22,
                   panels: int = 16, max_cycles: int = 50) -> dict:
    """ExprAdaptiveOsc::integrate_tail: f(x) cos(omega x) (or sin) on (a, inf) by cycles and
    Wynn's epsilon algorithm, line by line the host loop."""
    if kind not in ("cos", "sin"):
        raise ValueError(f"oscillatory: kind '{kind}' must be cos or sin")
    a, omega, atol = float(a), float(omega), float(atol)
    check(a, math.inf, omega, rtol, atol, panels, max_depth, max_intervals, True, panels,
          max_cycles)
    m = _native()
    out = dict(value=0.0, err_est=0.0, resabs=0.0, tol=atol, converged=False, evals=0, rounds=0,
               intervals=0, splits=0, floor=0, forced=0, nonfinite=0, capped=False,
               range="upper", omega=omega, kind=kind, cycles=0, extrapolated=False, reason="",
               sums=[], results=[])
    w = abs(omega)
    cycle = ((2.0 * math.floor(w) + 1.0) * 3.141592653589793) / w
    hw0 = 0.5 * (cycle / float(panels))
    share = 1.0 - TAIL_P
    psum = errsum = first_r = last_r = est = 0.0
    sums, results = out["sums"], out["results"]
    all_converged, stopped = True, False
    for k in range(1, max_cycles + 1):
        lo = a + float(k - 1) * cycle
        hi = a + float(k) * cycle
        cyc_atol = atol * share
        share = share * TAIL_P
        r = _rounds(f, lo, hi, hw0, omega, kind, 0.0, cyc_atol, int(panels), int(max_depth),
                    int(max_intervals))
        out["cycles"] += 1
        psum = psum + r["value"]
        errsum = errsum + r["err_est"]
        out["resabs"] = out["resabs"] + r["resabs"]
        for key in ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite"):
            out[key] += r[key]
        out["capped"] = out["capped"] or r["capped"]
        all_converged = all_converged and r["converged"]
        if k == 1:
            first_r = r["resabs"]
        last_r = r["resabs"]
        sums.append(psum)
        out["value"] = psum
        if r["nonfinite"] or not math.isfinite(psum):
            break
        if k < 3:
            continue
        est = 50.0 * abs(r["value"])
        if errsum + est <= atol:
            out["extrapolated"] = False
            stopped = True
            break
        results.append(float(m.osc_epsilon(np.array(sums))))
        out["value"] = results[-1]
        out["extrapolated"] = True
        if len(results) < 3:
            est = math.inf
            continue
        est = abs(results[-1] - results[-2]) + abs(results[-1] - results[-3])
        if errsum + est <= atol:
            stopped = True
            break
    if out["cycles"] < 3:
        est = math.inf
    out["err_est"] = errsum + est
    decays = out["cycles"] >= 2 and last_r < first_r
    out["converged"] = bool(stopped and all_converged and not out["capped"]
                            and out["nonfinite"] == 0 and decays)
    if not out["converged"]:
        if out["nonfinite"]:
            out["reason"] = (f"f was not finite on {out['nonfinite']} intervals (both ends of "
                             "every interval are evaluated)")
        elif out["capped"]:
            out["reason"] = "max_intervals was reached in a cycle"
        elif not decays:
            out["reason"] = ("no decay: the last cycle's integral of |f| is not below the first "
                             "one's, so the Fourier integral does not converge")
        elif not stopped:
            out["reason"] = (f"max_cycles = {max_cycles} cycles did not bring the estimate "
                             "within atol")
        else:
            out["reason"] = "a cycle did not reach its share of atol"
    return out
