"""The adaptive integrators (ExprAdaptive, ExprAdaptiveSweep, ExprAdaptive2D) bit for bit on
the host: every rounding and every sum in the order miint/expr.hpp and the generated kernels
(csrc/runtime/expr_adaptive.cpp, expr_adaptive_sweep.cpp, expr_adaptive2d.cpp, and the prelude
of expr_rtc.cpp) document, so that a device result can be compared with ``==`` on its bits.

What it takes for that to be meaningful: f itself must be bit-reproducible, i.e. built from
exact operations and single correctly rounded ``+``, ``-``, ``fabs`` and compare/select, with
no product that feeds an addition (tests/expr_adaptive_exact_cases.py keeps to that). Then
numpy evaluates f to the device's bits, and what is left is the kernels' own arithmetic:

  * ``fma``: one rounding of a * b + c, in integers (Python 3.10 has no math.fma); ``fma_vec``
    is the same function on arrays: error-free transformations decide every element whose
    rounding they can prove, the rest go through the scalar.
  * ``gk15`` / ``gk15x15``: the rule's chains, on the native table (gk15_nodes and weights).
  * the wave64 xor butterfly 32..1 (six pairwise adds of 64 lanes), the four waves' sums as
    (red[0] + red[1]) + (red[2] + red[3]), the closing workgroup's p[t], p[t + 256], ..., the
    prefix kernel's contiguous runs of per = ceil(nb / 256) workgroups, the sweep's one wave per
    row chaining l, l + 64, ...
  * the decisions in their order, the cap, the children at slots 2 p, 2 p + 1, the accepted
    intervals at base + (i - p).

utils/adaptive_quad.py is the loose model (numpy's pairwise sums, two roundings where the
device has one); nothing here is derived from it. Each run returns the device result's fields,
the partition in acceptance order (``done``; ``partition`` is the host's ordering of it), the
list length of every round (``lengths``) and, per round, what the structural tests need.
"""
from __future__ import annotations

import math

import numpy as np

FLOOR = float.fromhex("0x1.9p-47")  # 50 * 2^-52, the constant of the decide kernels
BLOCK = 256
WAVE = 64


# ------------------------------------------------------------------ fma
def fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding (to nearest, ties to even). Zeros, infinities and NaN take
    the plain path, which is already right for them."""
    a, b, c = float(a), float(b), float(c)
    if a == 0.0 or b == 0.0 or not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    if c == 0.0:
        return a * b  # one rounding, and the sign of an underflowed product
    ma, ea = math.frexp(a)
    mb, eb = math.frexp(b)
    mc, ec = math.frexp(c)
    ip, ep = int(ma * 9007199254740992.0) * int(mb * 9007199254740992.0), ea + eb - 106
    ic, ec = int(mc * 9007199254740992.0), ec - 53
    e = min(ep, ec)
    n = (ip << (ep - e)) + (ic << (ec - e))
    if n == 0:
        return 0.0
    try:
        return float(n << e) if e >= 0 else n / (1 << -e)  # int / int is correctly rounded
    except OverflowError:
        return math.inf if n > 0 else -math.inf


_fma_obj = np.frompyfunc(fma, 3, 1)
_SPLIT = 134217729.0  # 2^27 + 1 (Veltkamp)
_LO, _HI = 2.0 ** -400, 2.0 ** 400


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_vec(a, b, c) -> np.ndarray:
    """``fma`` element by element. p + e = a b exactly (Dekker), s + t = p + c exactly (Knuth),
    so the answer is the rounding of s + t + e. With r = fl(t + e) exact that is fl(s + r); else
    fl(s + r) = u is kept only where u + v = s + r leaves v further from half a step of u than
    the error of r could bridge. Everything else (and every operand outside 2^-400 .. 2^400,
    where the transformations could over- or underflow) is handed to the scalar."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64),
                                  np.asarray(c, np.float64))
    shape = a.shape
    a, b, c = a.ravel(), b.ravel(), c.ravel()
    with np.errstate(all="ignore"):
        p = a * b
        out = p + c
        aa, ab, ac = np.abs(a), np.abs(b), np.abs(c)
        sized = ((aa >= _LO) & (aa <= _HI) & (ab >= _LO) & (ab <= _HI)
                 & ((c == 0.0) | ((ac >= _LO) & (ac <= _HI))))
        plain = (a == 0.0) | (b == 0.0) | ~(np.isfinite(a) & np.isfinite(b) & np.isfinite(c))
        t1 = _SPLIT * a
        ah = t1 - (t1 - a)
        al = a - ah
        t2 = _SPLIT * b
        bh = t2 - (t2 - b)
        bl = b - bh
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        s, t = _two_sum(p, c)
        r, r_err = _two_sum(t, e)
        u, v = _two_sum(s, r)
        au = np.abs(u)
        exact = r_err == 0.0
        step = np.spacing(au)
        mant = np.frexp(au)[0]
        safe = ((mant != 0.5) & (au >= _LO)
                & (np.abs(v) + 4.0 * np.abs(r_err) < 0.5 * step * (1.0 - 2.0 ** -40)))
        proven = sized & ~plain & (exact | safe)
        out = np.where(proven, u, out)
        out = np.where((c == 0.0) & ~plain, p, out)
        slow = np.flatnonzero(~(plain | proven | (c == 0.0)))
    if slow.size:
        out[slow] = _fma_obj(a[slow], b[slow], c[slow]).astype(np.float64)
    return out.reshape(shape)


# ------------------------------------------------------------------ the rule
_TABLE = None


def table():
    """(t[8], wk[8], wg[4]): the non-negative nodes from the centre outwards, their Kronrod
    weights, the Gauss weights of nodes 0, 2, 4, 6: the native table's doubles."""
    global _TABLE
    if _TABLE is None:
        from .._native import native

        m = native()
        t15, wk15, wg7 = m.gk15_nodes(), m.gk15_weights(), m.gk7_weights()
        _TABLE = ([float(v) for v in t15[7:]], [float(v) for v in wk15[7:]],
                  [float(v) for v in wg7[3:]])
        assert _TABLE[0][0] == 0.0 and len(_TABLE[0]) == 8 and len(_TABLE[2]) == 4
    return _TABLE


def gk15(f, lo, hi):
    """miint_gk15 on every interval: K, err = |K - G|, R."""
    t, wk, wg = table()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    hw = 0.5 * (hi - lo)
    c = lo + hw
    f0 = f(c)
    sk, sg, sa = wk[0] * f0, wg[0] * f0, wk[0] * np.abs(f0)
    for j in range(1, 8):
        f1, f2 = f(fma_vec(hw, -t[j], c)), f(fma_vec(hw, t[j], c))
        sk = fma_vec(wk[j], f1 + f2, sk)
        sa = fma_vec(wk[j], np.abs(f1) + np.abs(f2), sa)
        if j % 2 == 0:
            sg = fma_vec(wg[j // 2], f1 + f2, sg)
    kv, gv = hw * sk, hw * sg
    return kv, np.abs(kv - gv), hw * sa


def gk15x15(f, x0, x1, y0, y1):
    """miint_gk15x15 on every rectangle: K, err, ex, ey, R. f(x, y) on arrays."""
    t, wk, wg = table()
    hx = 0.5 * (x1 - x0)
    cx = x0 + hx
    hy = 0.5 * (y1 - y0)
    cy = y0 + hy
    xm = [None] + [fma_vec(hx, -t[i], cx) for i in range(1, 8)]
    xp = [None] + [fma_vec(hx, t[i], cx) for i in range(1, 8)]
    kk = gg = gk = kg = aa = pk = pg = pa = None
    for row in range(15):
        j = (row + 1) >> 1
        y = cy if row == 0 else fma_vec(hy, -t[j] if row & 1 else t[j], cy)
        f0 = f(cx, y)
        rk, rg, ra = wk[0] * f0, wg[0] * f0, wk[0] * np.abs(f0)
        for i in range(1, 8):
            f1, f2 = f(xm[i], y), f(xp[i], y)
            rk = fma_vec(wk[i], f1 + f2, rk)
            ra = fma_vec(wk[i], np.abs(f1) + np.abs(f2), ra)
            if i % 2 == 0:
                rg = fma_vec(wg[i // 2], f1 + f2, rg)
        if row == 0:
            kk, gk, aa = wk[0] * rk, wk[0] * rg, wk[0] * ra
            gg, kg = wg[0] * rg, wg[0] * rk
        elif row & 1:
            pk, pg, pa = rk, rg, ra
        else:
            tk, tg, ta = pk + rk, pg + rg, pa + ra
            kk, gk, aa = fma_vec(wk[j], tk, kk), fma_vec(wk[j], tg, gk), fma_vec(wk[j], ta, aa)
            if j % 2 == 0:
                gg, kg = fma_vec(wg[j // 2], tg, gg), fma_vec(wg[j // 2], tk, kg)
    s = hx * hy
    kv = s * kk
    return kv, np.abs(kv - s * gg), np.abs(kv - s * gk), np.abs(kv - s * kg), s * aa


# ------------------------------------------------------------------ the sums
_XOR = [np.arange(WAVE) ^ o for o in (32, 16, 8, 4, 2, 1)]


def wave_sum(v: np.ndarray) -> np.ndarray:
    """The butterfly over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32, ..., 1, as
    every lane does it; lane 0's value."""
    assert v.shape[-1] == WAVE
    for idx in _XOR:
        v = v + v[..., idx]
    return v[..., 0]


def block_sums(v: np.ndarray) -> np.ndarray:
    """MIINT_BLOCK_SUM and MIINT_RED per workgroup of 256 lanes, lane i holding v[i] and the
    lanes past the end +0.0: one double per workgroup."""
    n = v.shape[0]
    nb = (n + BLOCK - 1) // BLOCK
    lanes = np.zeros(nb * BLOCK)
    lanes[:n] = v
    red = wave_sum(lanes.reshape(nb, 4, WAVE))
    return (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])


def strided_chain(p: np.ndarray, lanes: int) -> np.ndarray:
    """Lane l's v = 0.0; v += p[l]; v += p[l + lanes]; ... in order."""
    v = np.zeros(lanes)
    for s in range(0, p.shape[0], lanes):
        part = p[s:s + lanes]
        v[:part.shape[0]] = v[:part.shape[0]] + part
    return v


def close_sum(p: np.ndarray) -> float:
    """MIINT_CLOSE with scale 1.0."""
    return float(block_sums(strided_chain(p, BLOCK))[0] * 1.0)


def prefix_sums(blk: np.ndarray, per_of=None):
    """miint_adapt_prefix's five sums: thread t chains the rows of blk (nb x 5) of its run
    [t per, min(t per + per, nb)) from 0.0, then the block reduction. ``per_of`` replaces
    per = ceil(nb / 256) (for a test that must see the run bounds matter)."""
    nb = blk.shape[0]
    per = (nb + BLOCK - 1) // BLOCK if per_of is None else per_of(nb)
    s = np.zeros((BLOCK, blk.shape[1]))
    for t in range(BLOCK):
        first = t * per
        last = min(first + per, nb)
        for b in range(first, last):
            s[t] = s[t] + blk[b]
    return [float(block_sums(s[:, q])[0]) for q in range(blk.shape[1])], per


def row_wave_sum(v: np.ndarray) -> float:
    """The sweep's sum of a row's segment: one wave, lane l chaining l, l + 64, ..."""
    return float(wave_sum(strided_chain(v, WAVE)))


# ------------------------------------------------------------------ pieces shared by the rounds
def init_edges(a: float, b: float, panels: int):
    """miint_adapt_init: lo_i = a + ((b - a) i) / panels, hi_i the next one's lo, the last b."""
    w, p = b - a, float(panels)
    i = np.arange(panels + 1, dtype=np.float64)
    e = a + (w * i) / p
    e[-1] = b
    return e[:-1].copy(), e[1:].copy()


def decide(k, err, r, share, forced_now, order="nwfF", floor=FLOOR):
    """how per interval: 1 nonfinite, 2 within, 3 floor, 4 forced, 5 split, the device's chain.
    ``share`` is the interval's part of the tolerance, ``forced_now`` the depth / midpoint
    test. ``order`` names the chain (n, w, f, F); another order is for the mutation tests."""
    tests = {"n": (~(np.isfinite(k) & np.isfinite(err)), 1), "w": (~(err > share), 2),
             "f": (err <= floor * r, 3), "F": (forced_now, 4)}
    how = np.full(k.shape, 5, dtype=np.int64)
    for key in reversed(order):
        cond, code = tests[key]
        how = np.where(cond, code, how)
    return how


def _tolerance(rtol, atol, s_acc, sum_k):
    t = rtol * abs(s_acc + sum_k)
    return atol if atol > t else t


def _masked(v, m):
    return np.where(m, v, 0.0)


class _Totals:
    """st[] of the 1-D and 2-D rounds, and what miint_adapt*_prefix's thread 0 does with it."""

    def __init__(self):
        self.s = self.e = self.r = 0.0
        self.tol = 0.0
        self.accepted = self.splits = self.floor = self.forced = self.nonfinite = 0

    def close_round(self, how, k, err, r, max_intervals, per_of=None):
        """The per-workgroup five sums, the prefix kernel, the cap. Returns (capped, info)."""
        n = how.shape[0]
        sp = how == 5
        blk = np.stack([block_sums(_masked(k, ~sp)), block_sums(_masked(err, ~sp)),
                        block_sums(_masked(r, ~sp)), block_sums(_masked(k, sp)),
                        block_sums(_masked(err, sp))], axis=1)
        red, per = prefix_sums(blk, per_of)
        ns = int(sp.sum())
        capped = self.accepted + (n - ns) + 2 * ns > max_intervals
        self.floor += int((how == 3).sum())
        self.forced += int((how == 4).sum())
        self.nonfinite += int((how == 1).sum())
        rk, re = red[0], red[1]
        if capped:
            rk = rk + red[3]
            re = re + red[4]
        self.s = self.s + rk
        self.e = self.e + re
        self.r = self.r + red[2]
        base = self.accepted
        self.accepted = base + (n if capped else n - ns)
        self.splits += 0 if capped else ns
        nblk = blk.shape[0]
        pad = np.zeros(nblk * BLOCK, dtype=np.int64)
        pad[:n] = sp
        in_blk = pad.reshape(nblk, BLOCK).sum(axis=1)
        lanes = np.minimum(BLOCK, n - BLOCK * np.arange(nblk))
        mixed = (in_blk > 0) & (in_blk < lanes)  # both split and accepted intervals
        info = dict(n=n, nb=nblk, per=per, splits=ns, capped=capped,
                    split_blocks=np.flatnonzero(in_blk > 0),
                    mixed_blocks=int(mixed.sum()), within=int((how == 2).sum()),
                    floor=int((how == 3).sum()), forced=int((how == 4).sum()))
        return capped, base, info


def _slots(sp: np.ndarray, capped: bool, base: int):
    """miint_adapt_scatter's addresses: p = the splits before i (0 everywhere in a capped
    round); a split interval's children at 2 p and 2 p + 1, an accepted one at base + (i - p)."""
    n = sp.shape[0]
    if capped:
        sp = np.zeros(n, dtype=bool)
    p = np.concatenate([[0], np.cumsum(sp)[:-1]]).astype(np.int64)
    i = np.arange(n)
    return sp, 2 * p[sp], (base + (i - p))[~sp]


# ------------------------------------------------------------------ ExprAdaptive
def range_kind(a: float, b: float) -> str:
    if math.isnan(a) or math.isnan(b) or a == b:
        return "finite"
    lo, hi = min(a, b), max(a, b)
    if math.isinf(lo) and math.isinf(hi):
        return "both"
    return "upper" if math.isinf(hi) else "lower" if math.isinf(lo) else "finite"


def mapped(f, a: float, b: float):
    """g of miint/expr.hpp on t, with x and t * t from the native adapt_range_map."""
    from .._native import native

    m, kind = native(), range_kind(a, b)

    def g(t):
        x, jac, x2 = m.adapt_range_map(a, b, np.ascontiguousarray(t))
        return (f(x) + f(x2)) / jac if kind == "both" else f(x) / jac

    return g


def adaptive_exact(f, a: float, b: float, rtol: float = 1e-10, atol: float = 0.0,
                   panels: int = 65536, max_depth: int = 60, max_intervals: int = 1 << 22,
                   unbounded: bool = False, order: str = "nwfF", floor_const: float = FLOOR,
                   per_of=None) -> dict:
    """ExprAdaptive::integrate. f maps an fp64 array to an fp64 array in the device's bits.
    ``order``, ``floor_const`` and ``per_of`` exist for the tests that show a changed reference
    is noticed; leave them alone otherwise."""
    a, b = float(a), float(b)
    kind = range_kind(a, b)
    assert kind == "finite" or unbounded
    out = dict(value=0.0, err_est=0.0, resabs=0.0, tol=float(atol), converged=True, evals=0,
               rounds=0, intervals=0, splits=0, floor=0, forced=0, nonfinite=0, capped=False,
               range=kind, done=np.empty((0, 2)), partition=np.empty((0, 2)), lengths=[],
               round_info=[], within=0)
    if a == b:
        return out
    swapped = a > b
    if kind != "finite":
        f, x0, x1 = mapped(f, a, b), 0.0, 1.0
    else:
        x0, x1 = (b, a) if swapped else (a, b)
    width = x1 - x0
    lo, hi = init_edges(x0, x1, panels)
    depth = np.zeros(panels, dtype=np.int64)
    st = _Totals()
    done = np.full((max_intervals, 2), np.nan)
    with np.errstate(all="ignore"):
        while True:
            n = lo.shape[0]
            assert 1 <= n <= max_intervals and out["rounds"] <= max_depth
            k, err, r = gk15(f, lo, hi)
            sum_k = close_sum(block_sums(k))
            st.tol = _tolerance(rtol, atol, st.s, sum_k)
            w = hi - lo
            c = lo + 0.5 * w
            how = decide(k, err, r, (st.tol * w) / width,
                         (depth >= max_depth) | (c == lo) | (c == hi), order, floor_const)
            capped, base, info = st.close_round(how, k, err, r, max_intervals, per_of)
            sp, child, slot = _slots(how == 5, capped, base)
            done[slot, 0], done[slot, 1] = lo[~sp], hi[~sp]
            out["rounds"] += 1
            out["evals"] += 15 * n
            out["lengths"].append(n)
            out["round_info"].append(info)
            out["within"] += info["within"]
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
    part = done[np.lexsort((done[:, 1], done[:, 0]))]  # std::sort of (lo, hi) pairs
    if swapped and kind == "finite":
        part = part[::-1, ::-1].copy()
    out.update(value=-st.s if swapped else st.s, err_est=st.e, resabs=st.r, tol=st.tol,
               intervals=st.accepted, splits=st.splits, floor=st.floor, forced=st.forced,
               nonfinite=st.nonfinite, done=done, partition=part)
    out["converged"] = bool(st.e <= st.tol and not out["capped"] and st.nonfinite == 0)
    return out


# ------------------------------------------------------------------ ExprAdaptiveSweep
ROW_FIELDS = ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds", "intervals",
              "splits", "floor", "forced", "nonfinite", "capped")


def adaptive_sweep_exact(f, params, a: float, b: float, rtol: float = 1e-10, atol: float = 0.0,
                         panels: int = 16, max_depth: int = 60, max_intervals: int = 1 << 12,
                         row_sum=row_wave_sum) -> dict:
    """ExprAdaptiveSweep::integrate on a finite range with ``panels`` and ``max_intervals``
    given (per row). f(x, p0, p1, ...) on arrays. The whole list, the rows' segments and the
    list of active rows are kept as the device keeps them. ``row_sum`` is the order of a row's
    sums (another one is for the mutation tests)."""
    p = np.asarray(params, dtype=np.float64)
    rows = p.shape[0]
    a, b = float(a), float(b)
    swapped = a > b
    x0, x1 = (b, a) if swapped else (a, b)
    width = x1 - x0
    elo, ehi = init_edges(x0, x1, panels)
    lo, hi = np.tile(elo, rows), np.tile(ehi, rows)
    row = np.repeat(np.arange(rows), panels)
    depth = np.zeros(rows * panels, dtype=np.int64)
    active = list(range(rows))
    seg_start = [r * panels for r in range(rows)]
    seg_len = [panels] * rows
    st = [dict(s=0.0, e=0.0, r=0.0, tol=0.0, evals=0, rounds=0, accepted=0, splits=0, floor=0,
               forced=0, nonfinite=0, capped=False, within=0) for _ in range(rows)]
    lengths, actives, rnd = [], [], 0
    with np.errstate(all="ignore"):
        while True:
            n = lo.shape[0]
            rnd += 1
            lengths.append(n)
            actives.append(list(active))
            k, err, r = gk15(lambda x: f(x, *(p[row, j] for j in range(p.shape[1]))), lo, hi)
            w = hi - lo
            c = lo + 0.5 * w
            rank = np.full(n, -1, dtype=np.int64)
            next_len = []
            for rw in active:
                s0, ln = seg_start[rw], seg_len[rw]
                sl = slice(s0, s0 + ln)
                t = st[rw]
                sum_k = row_sum(k[sl])
                tol = _tolerance(rtol, atol, t["s"], sum_k)
                how = decide(k[sl], err[sl], r[sl], (tol * w[sl]) / width,
                             (depth[sl] >= max_depth) | (c[sl] == lo[sl]) | (c[sl] == hi[sl]))
                sp = how == 5
                rank[sl] = np.where(sp, np.cumsum(sp) - 1, -1)
                ak, ae, ar = (row_sum(_masked(v[sl], ~sp)) for v in (k, err, r))
                pk, pe = (row_sum(_masked(v[sl], sp)) for v in (k, err))
                ns = int(sp.sum())
                capped = t["accepted"] + (ln - ns) + 2 * ns > max_intervals
                if capped:
                    ak = ak + pk
                    ae = ae + pe
                t["s"], t["e"], t["r"], t["tol"] = t["s"] + ak, t["e"] + ae, t["r"] + ar, tol
                t["evals"] += 15 * ln
                t["rounds"] = rnd
                t["accepted"] += ln if capped else ln - ns
                t["splits"] += 0 if capped else ns
                t["floor"] += int((how == 3).sum())
                t["forced"] += int((how == 4).sum())
                t["nonfinite"] += int((how == 1).sum())
                t["within"] += int((how == 2).sum())
                t["capped"] = capped
                next_len.append(0 if capped else 2 * ns)
            # miint_asweep_prefix: the rows that stay, their segments, in slot order
            off, nxt_active = 0, []
            for slot, rw in enumerate(active):
                if next_len[slot] == 0:
                    continue
                seg_start[rw], seg_len[rw] = off, next_len[slot]
                nxt_active.append(rw)
                off += next_len[slot]
            if off == 0:
                break
            # miint_asweep_scatter: children at start(row) + 2 rank, + 1
            go = (rank >= 0) & ~np.array([st[rw]["capped"] for rw in row])
            q = np.array([seg_start[rw] for rw in row[go]], dtype=np.int64) + 2 * rank[go]
            nlo, nhi = np.full(off, np.nan), np.full(off, np.nan)
            nd, nrow = np.full(off, -1, dtype=np.int64), np.full(off, -1, dtype=np.int64)
            nlo[q], nhi[q], nlo[q + 1], nhi[q + 1] = lo[go], c[go], c[go], hi[go]
            nd[q] = nd[q + 1] = depth[go] + 1
            nrow[q] = nrow[q + 1] = row[go]
            assert (nrow >= 0).all()
            lo, hi, depth, row, active = nlo, nhi, nd, nrow, nxt_active
    out = dict(value=np.array([-t["s"] if swapped else t["s"] for t in st]),
               err_est=np.array([t["e"] for t in st]), resabs=np.array([t["r"] for t in st]),
               tol=np.array([t["tol"] for t in st]),
               capped=np.array([t["capped"] for t in st], dtype=bool))
    for key, name in (("evals", "evals"), ("rounds", "rounds"), ("intervals", "accepted"),
                      ("splits", "splits"), ("floor", "floor"), ("forced", "forced"),
                      ("nonfinite", "nonfinite"), ("within", "within")):
        out[key] = np.array([t[name] for t in st], dtype=np.int64)
    out["converged"] = (out["err_est"] <= out["tol"]) & ~out["capped"] & (out["nonfinite"] == 0)
    out.update(call_rounds=rnd, call_evals=15 * sum(lengths), peak=max(lengths), lengths=lengths,
               actives=actives)
    return out


# ------------------------------------------------------------------ ExprAdaptive2D
def choose_x(ex, ey, wx, wy, box_x, box_y, tie="ge"):
    """The split axis: x if ex > ey, y if ey > ex, on a tie x when wx Wy >= wy Wx. Returns
    (along_x, tied). ``tie``: 'ge' is the device's rule; 'gt' is for the mutation tests."""
    rel = wx * box_y >= wy * box_x if tie == "ge" else wx * box_y > wy * box_x
    tied = ~(ex > ey) & ~(ey > ex)
    return np.where(ex > ey, True, np.where(ey > ex, False, rel)), tied


def adaptive2d_exact(f, ax: float, bx: float, ay: float, by: float, rtol: float = 1e-10,
                     atol: float = 0.0, panels=(64, 64), max_depth: int = 60,
                     max_intervals: int = 1 << 22, tie: str = "ge") -> dict:
    """ExprAdaptive2D::integrate. f(x, y) on arrays. ``partition`` is ordered by (y0, x0) as the
    host orders it; ``ties`` counts the rectangles split (or forced) on an ex == ey tie, and
    ``ties_to_y`` those of them the rule sent along y."""
    ax, bx, ay, by = float(ax), float(bx), float(ay), float(by)
    px, py = (panels, panels) if isinstance(panels, int) else panels
    out = dict(value=0.0, err_est=0.0, resabs=0.0, tol=float(atol), converged=True, evals=0,
               rounds=0, intervals=0, splits=0, splits_x=0, splits_y=0, floor=0, forced=0,
               nonfinite=0, capped=False, done=np.empty((0, 4)), partition=np.empty((0, 4)),
               lengths=[], round_info=[], ties=0, ties_to_y=0, within=0, forced_by_depth=0)
    if ax == bx or ay == by:
        return out
    negate = (ax > bx) != (ay > by)
    x0, x1, y0, y1 = min(ax, bx), max(ax, bx), min(ay, by), max(ay, by)
    box_x, box_y = x1 - x0, y1 - y0
    exl, exh = init_edges(x0, x1, px)
    eyl, eyh = init_edges(y0, y1, py)
    xl, xh = np.tile(exl, py), np.tile(exh, py)  # i = iy * px + ix
    yl, yh = np.repeat(eyl, px), np.repeat(eyh, px)
    depth = np.zeros(px * py, dtype=np.int64)  # x depth in the low half, y depth in the high
    st = _Totals()
    sx = sy = 0
    done = np.full((max_intervals, 4), np.nan)
    with np.errstate(all="ignore"):
        while True:
            n = xl.shape[0]
            assert 1 <= n <= max_intervals and out["rounds"] <= 2 * max_depth
            k, err, ex, ey, r = gk15x15(f, xl, xh, yl, yh)
            sum_k = close_sum(block_sums(k))
            st.tol = _tolerance(rtol, atol, st.s, sum_k)
            wx, wy = xh - xl, yh - yl
            along_x, tied = choose_x(ex, ey, wx, wy, box_x, box_y, tie)
            lo, hi = np.where(along_x, xl, yl), np.where(along_x, xh, yh)
            c = lo + 0.5 * (hi - lo)
            dep = np.where(along_x, depth & 0xffff, depth >> 16)
            how = decide(k, err, r, (st.tol * (wx * wy)) / (box_x * box_y),
                         (dep >= max_depth) | (c == lo) | (c == hi))
            capped, base, info = st.close_round(how, k, err, r, max_intervals)
            sp, child, slot = _slots(how == 5, capped, base)
            done[slot] = np.stack([xl, xh, yl, yh], axis=1)[~sp]
            out["rounds"] += 1
            out["evals"] += 225 * n
            out["lengths"].append(n)
            out["round_info"].append(info)
            out["within"] += info["within"]
            out["ties"] += int((tied & (how >= 4)).sum())
            out["ties_to_y"] += int((tied & ~along_x & (how >= 4)).sum())
            out["forced_by_depth"] += int(((how == 4) & (dep >= max_depth)).sum())
            if capped or not sp.any():
                out["capped"] = capped
                break
            sx += int((sp & along_x).sum())
            sy += int((sp & ~along_x).sum())
            nxt = 2 * int(sp.sum())
            new = [np.empty(nxt) for _ in range(4)]
            nd = np.empty(nxt, dtype=np.int64)
            gx = along_x[sp]
            cs = c[sp]
            for off in (0, 1):  # the lower child, then the upper one
                q = child + off
                new[0][q] = np.where(gx & (off == 1), cs, xl[sp])
                new[1][q] = np.where(gx & (off == 0), cs, xh[sp])
                new[2][q] = np.where(~gx & (off == 1), cs, yl[sp])
                new[3][q] = np.where(~gx & (off == 0), cs, yh[sp])
                nd[q] = depth[sp] + np.where(gx, 1, 0x10000)
            xl, xh, yl, yh = new
            depth = nd
    done = done[:st.accepted]
    part = done[np.lexsort((done[:, 0], done[:, 2]))]
    out.update(value=-st.s if negate else st.s, err_est=st.e, resabs=st.r, tol=st.tol,
               intervals=st.accepted, splits=st.splits, splits_x=sx, splits_y=sy,
               floor=st.floor, forced=st.forced, nonfinite=st.nonfinite, done=done,
               partition=part)
    out["converged"] = bool(st.e <= st.tol and not out["capped"] and st.nonfinite == 0)
    return out
