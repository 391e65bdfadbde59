"""The exact integer reference of the train scan (cuda_v_mpi_amd/utils/exact_scan.py), checked
on the CPU: against a brute force in rationals, against the host engine, and — for every input
the GPU tests launch — that the exactness budget holds. The last test freezes the one step of
the argument that is not obvious: trainscan.hip's closed-form tile sums stay exact.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest
import torch

import scan_exact_cases as cases
from cuda_v_mpi_amd.utils import exact_scan as xs


def _brute(tab, d, k, i0, n, window, carries):
    """x, vel, pos as Fractions in true units (not 2**-k), from the definition."""
    T = [int(v) for v in tab]
    dt = Fraction(d, 2**k)
    lo, hi = window if window is not None else (0, i0 + n)
    x = []
    for i in range(i0, i0 + n):
        if not lo <= i < hi:
            x.append(Fraction(0))
            continue
        t = dt * i
        s = min(int(t), len(T) - 2)  # t >= 0: int() is the floor
        x.append(T[s] + (T[s + 1] - T[s]) * (t - s))
    vel, pos = [], []
    v, p = Fraction(carries[0]), Fraction(carries[1])
    for xi in x:
        v += xi
        p += v
        vel.append(v)
        pos.append(p)
    return x, vel, pos


SMALL = xs.jagged_table(12, 7, seed=3)


@pytest.mark.parametrize("d,k,i0,n,window,carries", [
    (1, 3, 0, 50, None, (0, 0)),
    (1, 3, 5, 60, None, (0, 0)),              # starts mid-segment
    (3, 4, 7, 80, None, (0, 0)),              # dt = 3/16: segments of uneven sample counts
    (1, 0, 0, 40, None, (0, 0)),              # every sample on a knot, most past the end
    (5, 2, 3, 90, None, (0, 0)),              # runs far past the table's end (flat tail)
    (1, 3, 5, 60, (20, 41), (0, 0)),          # window inside the slice
    (1, 3, 5, 60, (0, 5), (0, 0)),            # window wholly before
    (1, 3, 5, 60, (30, 30), (0, 0)),          # empty window
    (1, 3, 5, 60, (60, 500), (0, 0)),         # window cut by the slice's end
    (1, 3, 5, 60, None, (98764, -7901234)),   # carries, in units of 1/8
    (3, 4, 7, 80, (11, 70), (-5, 12)),
])
def test_exact_scan_equals_rational_brute_force(d, k, i0, n, window, carries):
    ref = xs.exact_scan(SMALL, d, k, i0, n, window, carries)
    unit = Fraction(1, 2**k)
    x, vel, pos = _brute(SMALL, d, k, i0, n, window, [c * unit for c in carries])
    assert [v * unit for v in ref.x.tolist()] == x
    assert [v * unit for v in ref.vel.tolist()] == vel
    assert [v * unit for v in ref.pos.tolist()] == pos
    x0, vel0, pos0 = _brute(SMALL, d, k, i0, n, window, (0, 0))
    assert (ref.totals[0] * unit, ref.totals[1] * unit) == (vel0[-1], pos0[-1])
    assert ref.x.dtype == ref.vel.dtype == ref.pos.dtype == torch.int64
    # to_f64 is the exact quotient
    assert [Fraction(v) for v in xs.to_f64(ref.pos, k).tolist()] == pos


def test_jagged_table_shape():
    t = xs.jagged_table(2048, 7, seed=1)
    assert t.dtype == np.int64 and t.shape == (2048,)
    assert t.min() >= -7 and t.max() <= 7 and len(set(t.tolist())) == 15
    assert t[-1] == t[-2] != 0
    assert np.array_equal(t, xs.jagged_table(2048, 7, seed=1))
    free = [xs.jagged_table(64, 3, seed=s, flat_tail=False) for s in range(40)]
    assert any(f[-1] != f[-2] for f in free)
    # jagged: neighbouring slopes differ almost everywhere (a smooth table would hide a
    # sample given to the neighbouring segment)
    slopes = np.diff(t)
    assert (np.diff(slopes) != 0).mean() > 0.8


def test_flat_tail_extrapolates_a_nonzero_constant():
    tab = cases.table("jag7")
    ref = xs.exact_scan(tab, 1, 6, 2047 * 64 - 3, 200)
    assert ref.x[3:].unique().tolist() == [int(tab[-1]) * 64] and tab[-1] != 0


@pytest.mark.parametrize("name,sps,k,seconds,threads", [
    ("jag1", cases.CLASS_SPS, cases.CLASS_K, cases.CLASS_SECONDS, 3),  # the class-level case
    ("jag7", 64, 6, 2047, 4),                                          # the whole table
    ("jag7", 1, 0, 2047, 1),
])
def test_host_engine_scalars_are_the_exact_ones(native, name, sps, k, seconds, threads):
    """The host engine's closed tile sums and carries are exact on these inputs too."""
    tab = cases.table(name)
    n = sps * seconds
    assert xs.budget_bits(tab, 1, k, 0, n) < 53
    ref = xs.exact_scan(tab, 1, k, 0, n)
    r = native.host_trainscan(sps, seconds, native.HostPool(threads), None, False,
                              [float(v) for v in tab])
    assert r["distance"] * sps == float(xs.to_f64(ref.vel[-1:], k))
    assert r["sum_of_sums"] == float(xs.to_f64(ref.pos[-1:], k))
    assert ref.totals == (int(ref.vel[-1]), int(ref.pos[-1]))


def test_every_gpu_case_keeps_the_budget():
    """A condition on the inputs, not a measurement: an input at 2**53 or above would make a
    bitwise comparison a bad test. The GPU tests assert the same before they launch."""
    n = 0
    for label, case in cases.every_gpu_case():
        assert cases.budget(case) < 53, label
        n += 1
    assert n == 6 * 12 + 1 + 3 * 6 + 3 * 2 + 1 + 1
    assert cases.budget(cases.FLAT_TAIL) > 49  # the case is near the limit on purpose
    assert cases.budget(cases.BIG) < 51


def test_budget_bits_is_the_stated_bound():
    tab = cases.table("jag7")
    x = xs.exact_samples(tab, 3, 10, 37, 5000, (100, 4000))
    want = 77 + (5000 + 4096) * (13 + int(x.abs().sum()))
    assert 2 ** xs.budget_bits(tab, 3, 10, 37, 5000, (100, 4000), (-13, 77)) == \
        pytest.approx(want, rel=1e-12)
    assert xs.budget_bits(tab, 1, 6, 0, 100, (500, 600)) == 0.0  # nothing to sum


# ---------------------------------------------------------------- tile_sums_closed, emulated
def _ex(v: Fraction) -> float:
    """The fp64 result of an operation whose exact value is v: it must be representable."""
    f = float(v)
    assert Fraction(f) == v, f"{v} is not an fp64"
    return f


def _F(f: float) -> Fraction:
    return Fraction(f)


def _tile_sums_closed(tab, sps, i0, n, win_lo, win_hi, t):
    """trainscan.hip tile_sums_closed, operation by operation in fp64 (every operation's exact
    result is asserted representable, so plain rounding never happens), integers as there."""
    kTile = 4096
    dt = 1.0 / sps
    nseg = len(tab) - 1
    g0 = t * kTile
    g1 = min(g0 + kTile, n)
    it0 = i0 + g0
    ia = max(it0, win_lo)
    ib = min(i0 + g1, win_hi)
    s1 = s2 = 0.0
    sixth = 1.0 / 6.0
    while ia < ib:
        sg = min(ia // sps, nseg - 1)
        base = sg * sps
        end = ib if (sg == nseg - 1 or base + sps > ib) else base + sps
        ja, jb = float(ia - base), float(end - base)
        m = _ex(_F(jb) - _F(ja))
        sj = _ex(_F(_ex(_F(0.5) * _F(m))) * _F(_ex(_F(_ex(_F(ja) + _F(jb))) - 1)))

        def sq(x):
            a = _ex(_F(x) - 1)
            b = _ex(_F(_ex(_F(2.0) * _F(x))) - 1)
            return _ex(_F(_ex(_F(a) * _F(x))) * _F(b))
        dsq = _ex(_F(sq(jb)) - _F(sq(ja)))
        sj2 = dsq * sixth  # the one rounding: it must land on the exact quotient
        assert _F(sj2) == _F(dsq) / 6
        v0 = float(tab[sg])
        c = _ex(_F(_ex(_F(float(tab[sg + 1])) - _F(v0))) * _F(dt))
        w0 = float((g1 - g0) + it0 - base)
        s1 = _ex(_F(s1) + _F(_ex(_F(c) * _F(sj) + _F(_ex(_F(m) * _F(v0))))))
        inner = _ex(_F(w0) * _F(c) - _F(v0))                               # fma(w0, c, -v0)
        wmv = _ex(_F(_ex(_F(w0) * _F(m))) * _F(v0))                        # w0 * m * v0
        term = _ex(_F(_ex(_F(inner) * _F(sj) + _F(wmv))) - _F(_ex(_F(c) * _F(sj2))))
        s2 = _ex(_F(s2) + _F(term))
        ia = end
    return s1, s2


@pytest.mark.parametrize("k", [0, 2, 6, 10])
@pytest.mark.parametrize("i0,n,window", [
    (0, 5 * 4096 + 77, None),
    (37, 3 * 4096, None),                                   # tiles start mid-segment
    (37, 4 * 4096 + 1, (37 + 4096 + 100, 37 + 3 * 4096 - 5)),  # a fill window
    (37, 2 * 4096 + 9, (37 + 100, 37 + 900)),                  # ... inside one tile
])
def test_tile_sums_closed_emulation_is_exact(k, i0, n, window):
    """sps in {1, 4, 64, 1024} on the 2048-entry table; at sps = 1 and 4 the slices run past
    the table's end, and a second slice per sps starts at the table's last segments."""
    sps = 2**k
    tab = cases.table("jag7")
    for shift in (0, max(0, 2047 * sps - 4096 - 50)):  # near the start; across the table's end
        a = i0 + shift
        win = None if window is None else (window[0] + shift, window[1] + shift)
        x = xs.exact_samples(tab, 1, k, a, n, win).numpy()
        lo, hi = win if win is not None else (0, 2**63)
        for t in range((n + 4095) // 4096):
            xt = x[t * 4096:(t + 1) * 4096]
            nt = len(xt)
            w = np.arange(nt, 0, -1, dtype=np.int64)  # sample l is in n_t - l of the prefixes
            s1, s2 = _tile_sums_closed([int(v) for v in tab], sps, a, n, lo, hi, t)
            assert _F(s1) * sps == int(xt.sum()), (shift, t)
            assert _F(s2) * sps == int((w * xt).sum()), (shift, t)
