"""An exact reference of the train scan, in integers only.

The train scan (csrc/kernels/trainscan.hip, scan.hip) samples a piecewise-linear table T at
t = dt * i, v_i = fma(T[s+1] - T[s], t - s, T[s]) with s = min(floor(t), entries - 2), and
writes vel = running sum of v and pos = running sum of vel. With integer table entries and
dt = d / 2**k every sample is an integer multiple of 2**-k, and so is every partial sum any
kernel can form, in any order: while the magnitudes stay below 2**53 in that unit, fp64
computes all of them exactly, and every path must return bitwise the same arrays. This
module computes those arrays in int64 (torch, on the CPU or on a device) in units of 2**-k:
no floating point anywhere, so the reference has no rounding of its own to argue about.

    tab = jagged_table(2048, 7, seed=1)
    assert budget_bits(tab, d=1, k=6, i0=0, n=4097) < 53     # a condition on the INPUT
    ref = exact_scan(tab, d=1, k=6, i0=0, n=4097)
    torch.equal(vel, to_f64(ref.vel, 6))
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

# the widest weight any kernel gives one partial sum: the slice length plus one padded tile
# (tile count x prefix t0 * C1, the look-back's gap * A, a partial tile's padding correction)
PAD = 4096


class ExactScan(NamedTuple):
    x: torch.Tensor      # samples, int64, units of 2**-k
    vel: torch.Tensor    # C1 + cumsum(x)
    pos: torch.Tensor    # C2 + cumsum(vel)
    totals: tuple        # (T1, T2) = (sum x, sum of cumsum(x)): no carries


def jagged_table(entries: int, amplitude: int, seed: int, flat_tail: bool = True) -> np.ndarray:
    """`entries` random integers in [-amplitude, amplitude] (int64). With `flat_tail` the last
    two entries are equal and non-zero: samples past the table's end extrapolate the last
    segment, which is then a non-zero constant, so a tile dropped out there still shows."""
    if entries < 2 or amplitude < 1:
        raise ValueError("jagged_table needs entries >= 2 and amplitude >= 1")
    rng = np.random.default_rng(seed)
    t = rng.integers(-amplitude, amplitude + 1, size=entries, dtype=np.int64)
    if flat_tail:
        tail = int(rng.integers(1, amplitude + 1)) * (1 if rng.integers(0, 2) else -1)
        t[-2:] = tail
    return t


def _as_table(table, device) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(table), device=device)
    if t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 2:
        raise ValueError("table must be a 1-D int64 array of at least 2 entries")
    return t


def _window(i0: int, n: int, window) -> tuple[int, int]:
    """Slice-local [a, b) of the samples inside `window` (global indices; None: all)."""
    lo, hi = (0, i0 + n) if window is None else window
    a, b = max(lo, i0), min(hi, i0 + n)
    return (a - i0, b - i0) if a < b else (0, 0)


def exact_samples(table, d: int, k: int, i0: int, n: int, window=None,
                  device="cpu") -> torch.Tensor:
    """Samples i0 .. i0 + n - 1 in units of 2**-k; zero outside `window`."""
    if d < 1 or k < 0 or i0 < 0 or n < 1:
        raise ValueError("exact_samples needs d >= 1, k >= 0, i0 >= 0, n >= 1")
    T = _as_table(table, device)
    x = torch.zeros(n, dtype=torch.int64, device=device)
    a, b = _window(i0, n, window)
    if a == b:
        return x
    num = torch.arange(i0 + a, i0 + b, dtype=torch.int64, device=device) * d
    s = torch.clamp(num >> k, max=T.numel() - 2)
    v0 = T[s]
    x[a:b] = (v0 << k) + (T[s + 1] - v0) * (num - (s << k))
    return x


def exact_scan(table, d: int, k: int, i0: int, n: int, window=None, carries=(0, 0),
               device="cpu") -> ExactScan:
    """x, vel = C1 + cumsum(x), pos = C2 + cumsum(vel) and the totals, all int64 in units of
    2**-k. `carries` = (C1, C2) in the same unit. Sample i0 + g sits at num = (i0 + g) * d,
    in segment s = min(num >> k, entries - 2), with value
    T[s] * 2**k + (T[s+1] - T[s]) * (num - (s << k))."""
    c1, c2 = (int(c) for c in carries)
    x = exact_samples(table, d, k, i0, n, window, device)
    vel = torch.cumsum(x, 0)
    pos = torch.cumsum(vel, 0)
    totals = (int(vel[-1]), int(pos[-1]))
    if c1:
        vel += c1
        pos += c1 * torch.arange(1, n + 1, dtype=torch.int64, device=device)
    if c2:
        pos += c2
    return ExactScan(x, vel, pos, totals)


def budget_bits(table, d: int, k: int, i0: int, n: int, window=None, carries=(0, 0)) -> float:
    """log2 of |C2| + (n + PAD) * (|C1| + sum |x_i|) in units of 2**-k: a bound on every
    intermediate of every kernel (any partial sum of samples is at most sum |x_i|, and no
    kernel weights one by more than n + PAD). Below 53, fp64 holds them all exactly. Only
    the samples inside the window are formed, so a long slice with a short window is cheap."""
    a, b = _window(i0, n, window)
    sx = 0
    if a < b:
        lo = i0 + a
        # in pieces: the sum of |x| over 2**28 samples must not need 2 GB at once
        for p0 in range(lo, i0 + b, 1 << 22):
            m = min(1 << 22, i0 + b - p0)
            sx += int(exact_samples(table, d, k, p0, m).abs().sum())
    c1, c2 = (abs(int(c)) for c in carries)
    bound = c2 + (n + PAD) * (c1 + sx)
    return math.log2(bound) if bound > 0 else 0.0


def to_f64(v: torch.Tensor, k: int) -> torch.Tensor:
    """value / 2**k as fp64: exact for |value| < 2**53 (the conversion and the scaling by a
    power of two both are), which budget_bits < 53 guarantees for every reference array."""
    if v.dtype != torch.int64:
        raise ValueError("to_f64 converts the int64 reference arrays")
    return v.to(torch.float64) * (2.0 ** -k)


def dt_of(d: int, k: int) -> float:
    """d / 2**k as the fp64 the kernels take (exact)."""
    return d * 2.0 ** -k
