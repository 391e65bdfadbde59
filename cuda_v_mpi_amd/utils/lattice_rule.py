"""The rule of the lattice kernels (csrc/runtime/expr_lattice.cpp, ExprLattice) in numpy: the
CPU model the device is held to, the criterion its generating vectors are chosen by, and an
integer reference for the exact tests.

A randomly shifted rank-1 lattice rule with n = 2^m points in d <= 16 dimensions. Point i of
shift r has, in dimension j, the 32-bit fixed-point fraction

    u = (((i * z_j) mod n) << (32 - m)) + shift[r][j]   (mod 2^32)

tent (the default):  s = (int32)u >> 31, w = (u ^ s) & 0x7FFFFFFF, t = fma(w, 2^-31, 2^-32),
                     which is 1 - |2 tau - 1| of the centred fraction tau = (u + 1/2) / 2^32
periodic:            t = fma(u, 2^-32, 2^-33)

and the coordinate x_j = fma(t, b_j - a_j, a_j). Every t is a dyadic rational strictly inside
(0, 1): (2w + 1) / 2^32 or (2u + 1) / 2^33, exact in fp64. Shifts are the high 32 bits of
splitmix64 at the counter r * 16 + j. est_r = (vol * scale) * S_r / n, value = (sum est_r) / R
in index order, err_est = sqrt(sum (est_r - value)^2 / (R (R - 1))): one standard error.

What the model does not share with the device is the order of S_r's sum (numpy's pairwise
``sum`` here, four accumulators per lane and butterflies there) and the math library behind f,
so a smooth estimate agrees to rounding; an integrand whose samples sum exactly in fp64 agrees
bit for bit.

    r = lattice_model(lambda x: np.exp(-(x * x).sum(axis=-1)), [(0, 1)] * 6, m=16)
    r["value"], r["err_est"], r["estimates"]
"""
from __future__ import annotations

import math

import numpy as np

MAX_DIM = 16
M_MIN, M_MAX = 2, 30
MAX_SHIFTS = 4096
MASK64 = (1 << 64) - 1
_CHUNK = 1 << 16   # points evaluated at a time


# ------------------------------------------------------------------------------- shifts
def splitmix64_high32(seed: int, q: int) -> int:
    """The high 32 bits of splitmix64 at counter q, in Python integers."""
    z = (seed + (q + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z >> 32


def lattice_shifts(seed: int, shifts: int, d: int) -> np.ndarray:
    """shift[r][j] for r < shifts, j < d: splitmix64 at the counter r * 16 + j (uint32)."""
    return np.array([[splitmix64_high32(int(seed), r * MAX_DIM + j) for j in range(d)]
                     for r in range(shifts)], dtype=np.uint32).reshape(shifts, d)


# --------------------------------------------------------------------- generating vectors
def korobov(a: int, m: int, d: int) -> list:
    """z_j = a^j mod 2^m for j < d."""
    n = 1 << m
    return [pow(int(a), j, n) for j in range(d)]


def check_z(z, m: int, d: int) -> list:
    z = [int(v) for v in z]
    if len(z) != d:
        raise ValueError(f"lattice: {len(z)} generating entries for d = {d}")
    for j, v in enumerate(z):
        if not (0 < v < (1 << m)) or v % 2 == 0:
            raise ValueError(f"lattice: z[{j}] = {v} must be odd and below n = 2^{m}")
    return z


def generator(m: int, d: int) -> list:
    """The built-in vector for m (the table lives in C++: ``lattice_generator``)."""
    from .._native import native

    return [int(v) for v in native().lattice_generator(int(m), int(d))]


def criterion(a: int, m: int, d: int = MAX_DIM) -> float:
    """e^2(a) = -1 + (1/n) sum_i prod_{j<d} (1 + gamma_j 2 pi^2 B2({i z_j / n})) for the
    Korobov vector z_j = a^j mod n, B2(t) = t^2 - t + 1/6, gamma_j = 1 / (j + 1)^2: the squared
    worst-case error in the weighted Korobov space of smoothness 1. B2 is even about 1/2, so
    points i and n - i contribute the same product: only i <= n / 2 are formed. Chunks of 2^18
    points, each summed by numpy, the chunks' sums added in order."""
    n = 1 << m
    z = korobov(a, m, d)
    half = n // 2
    total = 0.0
    step = 1 << 18
    for i0 in range(0, half + 1, step):
        i = np.arange(i0, min(i0 + step, half + 1), dtype=np.int64)
        prod = np.ones(i.size)
        for j in range(d):
            t = ((i * z[j]) & (n - 1)).astype(np.float64) / n   # exact: i z_j < 2^62
            prod *= 1.0 + (2.0 * math.pi ** 2 / (j + 1) ** 2) * (t * t - t + 1.0 / 6.0)
        wgt = np.full(i.size, 2.0)
        wgt[i == 0] = 1.0
        wgt[i == half] = 1.0
        total += float((wgt * prod).sum())
    return total / n - 1.0


def search(m: int, candidates: int = 64, seed: int = 2024, d: int = MAX_DIM):
    """The a with the least ``criterion`` among ``candidates`` draws congruent to 3 or 5 mod 8
    (multiplicative order 2^(m-2)) below 2^m from a generator seeded with (seed, m); ties go to
    the smaller a. Returns (a, e2)."""
    if m < 3:
        raise ValueError("lattice search: m must be >= 3")
    rng = np.random.default_rng([int(seed), int(m)])
    hi = rng.integers(0, 1 << (m - 3), size=candidates)
    low = rng.integers(0, 2, size=candidates)
    cands = sorted({int(8 * h + (3 if b == 0 else 5)) for h, b in zip(hi, low)})
    best = None
    for a in cands:
        e2 = criterion(a, m, d)
        if best is None or e2 < best[1]:
            best = (a, e2)
    return best


# ------------------------------------------------------------------------------ points
def fractions_u32(m: int, z, shift_row, begin: int = 0, count: int | None = None) -> np.ndarray:
    """u of points [begin, begin + count) for one shift row: a (count, d) uint32 array."""
    n = 1 << m
    count = n - begin if count is None else count
    i = np.arange(begin, begin + count, dtype=np.uint64)[:, None]
    zz = np.asarray(z, dtype=np.uint64)[None, :]
    frac = ((i * zz) & np.uint64(n - 1)) << np.uint64(32 - m)     # i z_j < 2^60
    return ((frac + np.asarray(shift_row, dtype=np.uint64)[None, :])
            & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def numerators(u: np.ndarray, periodic: bool = False) -> np.ndarray:
    """The exact numerators of t (uint64): tent 2w + 1 over 2^32, periodic 2u + 1 over 2^33."""
    u = np.asarray(u, dtype=np.uint32)
    if periodic:
        return 2 * u.astype(np.uint64) + np.uint64(1)
    s = (u.view(np.int32) >> 31).view(np.uint32)
    w = (u ^ s) & np.uint32(0x7FFFFFFF)
    return 2 * w.astype(np.uint64) + np.uint64(1)


def denominator(periodic: bool = False) -> int:
    return 1 << 33 if periodic else 1 << 32


def unit_coords(u: np.ndarray, periodic: bool = False) -> np.ndarray:
    """t in (0, 1) as fp64: numerators / denominator, exact (the device's fma is exact too)."""
    return numerators(u, periodic).astype(np.float64) / float(denominator(periodic))


def _fma(t: np.ndarray, w: float, a: float) -> np.ndarray:
    """fma(t, w, a) by an error-free product and sum: equal to the fused result but for a
    double rounding on a rare tie. Exact whenever t * w is (power-of-two widths)."""
    split = 134217729.0   # 2^27 + 1
    p = t * w
    th = t * split
    th = th - (th - t)
    tl = t - th
    wh = w * split
    wh = wh - (wh - w)
    wl = w - wh
    e = ((th * wh - p) + th * wl + tl * wh) + tl * wl
    s = p + a
    bb = s - p
    e2 = (p - (s - bb)) + (a - bb)
    return s + (e + e2)


def box_arrays(box):
    lo = np.array([float(p[0]) for p in box], dtype=np.float64)
    hi = np.array([float(p[1]) for p in box], dtype=np.float64)
    return lo, hi - lo     # b_j - a_j rounded once


def coords(t: np.ndarray, box) -> np.ndarray:
    lo, width = box_arrays(box)
    with np.errstate(all="ignore"):
        return np.stack([_fma(t[:, j], float(width[j]), float(lo[j])) for j in range(len(box))],
                        axis=1)


def exact_points(m: int, z, shift_words, box, periodic: bool = False, begin: int = 0,
                 count: int | None = None):
    """The integer reference: for every shift row the exact numerators N of the coordinates'
    unit fractions, as Python-int object arrays of shape (R, count, d); coordinate j of a point
    is a_j + (b_j - a_j) N / D with D = ``denominator(periodic)``."""
    rows = np.asarray(shift_words, dtype=np.uint32).reshape(-1, len(box))
    return np.stack([numerators(fractions_u32(m, z, row, begin, count), periodic)
                     for row in rows]).astype(object)


# --------------------------------------------------------------------------- estimates
def check_rule(box, m: int, shifts: int, z=None, scale: float = 1.0) -> None:
    """The refusals of ``lattice_check``, with the numbers named."""
    d = len(box)
    if not 1 <= d <= MAX_DIM:
        raise ValueError(f"lattice: d = {d} must be 1..{MAX_DIM}")
    if not M_MIN <= m <= M_MAX:
        raise ValueError(f"lattice: m = {m} must be {M_MIN}..{M_MAX}")
    if not 1 <= shifts <= MAX_SHIFTS:
        raise ValueError(f"lattice: shifts = {shifts} must be 1..{MAX_SHIFTS}")
    lo, width = box_arrays(box)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(width))
            and np.all(np.isfinite(lo + width)) and np.isfinite(scale)):
        raise ValueError("lattice: the box and the scale must be finite")
    if z is not None:
        check_z(z, m, d)


def finish(sums, vol_scale: float, n: int) -> dict:
    """est_r, value and err_est from the shifts' sums, in the kernels' order."""
    est = [float(vol_scale * float(s) / n) for s in sums]
    r = len(est)
    acc = 0.0
    for e in est:
        acc += e
    value = acc / r
    if r == 1:
        err = math.inf
    else:
        q = 0.0
        for e in est:
            q += (e - value) * (e - value)
        err = math.sqrt(q / (float(r) * float(r - 1)))
    return dict(value=value, err_est=err, estimates=np.array(est, dtype=np.float64))


def lattice_model(f, box, m: int, shifts: int = 16, seed: int = 0, periodic: bool = False,
                  z=None, shift_words=None, begin: int = 0, count: int | None = None,
                  scale: float = 1.0) -> dict:
    """The rule on points [begin, begin + count) (default: all n). ``f`` maps a (k, d) fp64
    array of points to k values. Returns value, err_est, estimates, sums, abs_sums (the sums of |f|),
    vol_scale, m, n, shifts (the words), evals, levels, converged."""
    d = len(box)
    if shift_words is not None:
        words = np.asarray(shift_words, dtype=np.uint32).reshape(-1, d)
        shifts = words.shape[0]
    check_rule(box, m, shifts, z, scale)
    if shift_words is None:
        words = lattice_shifts(seed, shifts, d)
    z = generator(m, d) if z is None else check_z(z, m, d)
    n = 1 << m
    count = n - begin if count is None else count
    if not (0 <= begin and 0 <= count and begin + count <= n):
        raise ValueError(f"lattice: slice [{begin}, {begin} + {count}) outside [0, {n})")
    lo, width = box_arrays(box)
    vol = 1.0
    for w in width:
        vol *= float(w)
    sums, abs_sums = np.zeros(shifts), np.zeros(shifts)
    if vol != 0.0:
        with np.errstate(all="ignore"):
            for r in range(shifts):
                parts, aparts = [], []
                for c0 in range(begin, begin + count, _CHUNK):
                    c = min(_CHUNK, begin + count - c0)
                    x = coords(unit_coords(fractions_u32(m, z, words[r], c0, c), periodic), box)
                    fx = np.asarray(f(x), dtype=np.float64)
                    parts.append(float(fx.sum()))
                    aparts.append(float(np.abs(fx).sum()))
                sums[r] = math.fsum(parts)
                abs_sums[r] = math.fsum(aparts)
    out = finish(sums, vol * float(scale), n)
    out.update(sums=sums, abs_sums=abs_sums, vol_scale=vol * float(scale), m=m, n=n, shifts=words, evals=shifts * count, levels=1,
               converged=False)
    return out


def lattice_to_tolerance(f, box, rtol: float = 0.0, atol: float = 0.0, m_min: int = 12,
                         m_max: int | None = None, shifts: int = 16, seed: int = 0,
                         periodic: bool = False, shift_words=None, scale: float = 1.0) -> dict:
    """Walk m from m_min to m_max (clamped to the largest built-in m), each level a fresh rule
    with the same shifts; stop at the first level with err_est <= max(atol, rtol |value|)."""
    from .._native import native

    top = int(native().LATTICE_BUILTIN_M_MAX)
    m_max = top if m_max is None else min(int(m_max), top)
    rtol, atol = float(rtol or 0.0), float(atol or 0.0)
    if not (rtol >= 0 and atol >= 0 and math.isfinite(rtol) and math.isfinite(atol)
            and (rtol > 0 or atol > 0)):
        raise ValueError(f"lattice: rtol = {rtol:.17g} and atol = {atol:.17g} must be finite "
                         "and >= 0, and not both 0")
    if not int(native().LATTICE_BUILTIN_M_MIN) <= m_min <= m_max:
        raise ValueError(f"lattice: m_min = {m_min} and m_max = {m_max} must lie in the "
                         "built-in range, m_min <= m_max")
    evals = levels = 0
    for m in range(m_min, m_max + 1):
        out = lattice_model(f, box, m, shifts=shifts, seed=seed, periodic=periodic,
                            shift_words=shift_words, scale=scale)
        evals += out["evals"]
        levels += 1
        if out["err_est"] <= max(atol, rtol * abs(out["value"])):
            out["converged"] = True
            break
    out.update(evals=evals, levels=levels)
    return out
