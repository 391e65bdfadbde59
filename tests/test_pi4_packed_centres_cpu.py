"""The series_exact tiles form their sub-tile centres and slopes in packed fp32 too
(integrands.hpp Pi4::centres_f32 / slopes_f32): e_m, A, B and 2 B are rounded to fp32 once per
tile, and the two sub-tiles at +c0 and -c0 get their centres and slopes from three
v_pk_fma_f32 on (c0, -c0) SGPR pairs, instead of three v_fma_f64 and two conversions each.
And the pair loop runs in a pinned order (Pi4::subtile_squares, one asm statement per
sub-tile): the residuals of two pairs, then their squares into two running sums, so that no
v_pk_fma_f32 reads what the instruction before it wrote and no wait state stands between them.

Pinned on the gfx950 assembly through tools/isa_guard.py: at most 430 VALU per 384-sample tile
(measured 427; 466 with fp64 centres), at most 8 v_cvt_f32_f64 and 12 v_fma_f64 left in the tile
block (measured 3 and 5: the seed, the closed-form linear sum, the fold), at most 16 s_nop
(measured 11; 192 in the compiler's order), no packed FMA directly behind the one whose result
it reads, the timeline twin at the plain kernel's occupancy.

And a numpy model of one tile, with the fp32 operations in the tile's order, against exact
rational arithmetic and the x87 sum of the true function: the bound derived above
Pi4::tile_acc says every rounding of the squared residual is 2^-24 of a quantity below
E = 2e-6, four of them in all (|de| <= 4 * 2^-24 * E ~ 4.8e-13), so the squared term is off by
at most 2 E |de| + 2^-24 E^2 + 7e-20 ~ 2.2e-18 of a value of order 1: under 1/50 ulp.
Measured in the model: 3.6e-3 ulp (1/280) at the worst, in the middle of [0, 1] at
N = 96 000 001; 1.3e-7 ulp at N = 1e10."""
from __future__ import annotations

import os
import re
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import isa_guard  # noqa: E402

TILE = 384
TL = r"riemann_timeline_kernel(?:_o8)?ILNS_7DivModeE3ENS_3Pi4EEEv"


# ------------------------------------------------------------------ the kernels' assembly
@pytest.fixture(scope="module")
def functions():
    if not os.path.exists(isa_guard.HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        return list(isa_guard.functions(isa_guard.compile_asm("riemann", d)))


def kernel(functions, name):
    _, pat, tile = isa_guard.GUARDED[name]
    sym, body, info = next(f for f in functions if re.search(pat, f[0]))
    return isa_guard.stats(body, info, tile), body, info


def tile_block(body: str) -> list[str]:
    """Instructions of the straight-line block with the most VALU (one tile)."""
    blocks, _ = isa_guard.cfg(body)
    return max(blocks, key=lambda b: sum(1 for s in b if s.startswith("v_")))


@pytest.mark.parametrize("name", ["pi4_series_exact", "ms_pi4_series_exact"])
def test_tile_block_forms_its_centres_in_packed_fp32(functions, name):
    st, body, _ = kernel(functions, name)
    block = tile_block(body)
    ops = [s.split()[0] for s in block]
    valu = sum(1 for o in ops if o.startswith("v_"))
    cvt = sum(1 for o in ops if o.startswith("v_cvt_f32_f64"))
    fma64 = sum(1 for o in ops if o == "v_fma_f64")
    print(f"{name}: {valu} VALU per tile, {cvt} v_cvt_f32_f64, {fma64} v_fma_f64, "
          f"{ops.count('v_pk_fma_f32')} v_pk_fma_f32, {ops.count('s_nop')} s_nop")
    assert valu <= 430 and st["max_block_valu"] <= 430
    assert cvt <= 8
    assert fma64 <= 12
    # 384 for the samples, 18 for the six +-c0 centre and slope pairs
    assert ops.count("v_pk_fma_f32") >= 384 + 18
    assert ops.count("s_nop") <= 16


@pytest.mark.parametrize("name", ["pi4_series_exact", "ms_pi4_series_exact"])
def test_no_packed_fma_reads_what_the_instruction_before_it_wrote(functions, name):
    """The distance rule of the hand-ordered pair loop: inside an asm statement the compiler
    adds no wait states, so a v_pk_fma_f32 never directly follows the packed operation that
    wrote one of its sources (an s_nop between them counts as the wait)."""
    block = tile_block(kernel(functions, name)[1])
    prev_dst = None
    for ins in block:
        op, _, rest = ins.partition(" ")
        args = [a.strip() for a in rest.split(" op_sel")[0].split(",")]
        if op == "v_pk_fma_f32":
            assert prev_dst is None or prev_dst not in args[1:], ins
        prev_dst = args[0] if op.startswith("v_pk_") else None


def test_residency_is_kept(functions):
    ms, _, _ = kernel(functions, "ms_pi4_series_exact")
    assert ms["occupancy"] >= 7 and ms["vgpr"] <= 64 and ms["scratch"] == 0
    one, _, _ = kernel(functions, "pi4_series_exact")
    assert one["occupancy"] >= 8 and one["scratch"] == 0


def test_timeline_twin_keeps_the_plain_kernels_occupancy(functions):
    _, _, plain_info = kernel(functions, "ms_pi4_series_exact")
    tl = [f for f in functions if re.search(TL, f[0])]
    assert len(tl) == 1
    assert isa_guard.field(tl[0][2], "ScratchSize") == 0
    assert isa_guard.field(tl[0][2], "Occupancy") == isa_guard.field(plain_info, "Occupancy")


# ------------------------------------------------------------------ the numpy model of a tile
KPAIRS, KSUB, KSUBS = 16, 32, 12
MEAN_K2 = 85.25
SUM_K2 = 4718560.0
E_MAX = 2e-6  # |e| of every sample of an admitted launch (series_ok)
# the bound of the comment above Pi4::tile_acc, relative to a value of order 1 ...
D_E = 4 * 2.0**-24 * E_MAX
BOUND = 2 * E_MAX * D_E + 2.0**-24 * E_MAX**2 + 7e-20
# ... and in ulp of the value (an ulp is at least 2^-53 of it)
BOUND_ULP = BOUND / 2.0**-53


def fl(x: Fraction) -> float:
    """Round to nearest fp64 (int / int true division is correctly rounded)."""
    return x.numerator / x.denominator


def fma64(a: float, b: float, c: float) -> float:
    return fl(Fraction(a) * Fraction(b) + Fraction(c))


def fma32(a, b, c):
    """fp32 fma on arrays: the product of two fp32 is exact in fp64; the sum rounds at 2^-53
    before it rounds to fp32 (a double rounding, 2^-29 of an fp32 ulp at the most)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) +
            np.asarray(c, np.float64)).astype(np.float32)


def model_tile(a: float, b: float, n: int, tile: int):
    """One 384-sample tile of the left rule as Pi4::tile_acc<384, kSeriesExact> evaluates it.
    Returns (tile value without h * 4, x87 sum of the true function at the same coordinates,
    per-sample error of the squared term in ulp of the sample's value, max |e|)."""
    h = (b - a) / n
    xm = fl(Fraction(a) + Fraction(TILE * tile + 0.5 * (TILE - 1)) * Fraction(h))
    # seed_exact: s ~ 1 / d_m, e_m from the exact d_m, A from q = x_m s
    dm = fma64(xm, xm, 1.0)
    s = 1.0 / dm
    q = xm * s
    qe = fl(Fraction(xm) * Fraction(s) - Fraction(q))
    em = fma64(-xm, qe, fma64(-xm, q, 1.0 - s))
    A = (-2.0 * h) * q
    B = -(h * h) * s
    lin = fma64(SUM_K2, B, float(TILE) * em)
    # seed_f32
    emf, af, bf = np.float32(em), np.float32(A), np.float32(B)
    b2f = np.float32(bf + bf)
    # the six +-c0 pairs: (c0, -c0), (cm, -cm) -> centres and slopes, low and high halves
    i = np.arange(KSUBS // 2)
    c0 = (KSUB * (i + 0.5))
    cm = (c0 + MEAN_K2 / c0)
    c0f = np.stack([c0, -c0], axis=1).astype(np.float32)
    cmf = np.stack([cm, -cm], axis=1).astype(np.float32)
    ecs = fma32(c0f, fma32(cmf, bf, af), emf)
    aqs = fma32(c0f, b2f, af)
    kf = (np.arange(KPAIRS) + 0.5).astype(np.float32)
    # two packed running sums (lane 0 the +k samples', lane 1 the -k samples'): the pairs of
    # a sub-tile go two at a time, the first's squares into ta, the second's into tb
    t2 = [np.zeros(2, np.float32), np.zeros(2, np.float32)]
    sq = np.zeros(TILE, np.float32)
    e32 = np.zeros(TILE, np.float32)
    for sub in range(KSUBS):
        lo = sub >= KSUBS // 2  # the +c0 sub-tile reads the low halves
        p = sub - KSUBS // 2 if lo else KSUBS // 2 - 1 - sub
        ec, aq = ecs[p, 0 if lo else 1], aqs[p, 0 if lo else 1]
        for j in range(KPAIRS):
            e = fma32(np.array([kf[j], -kf[j]], np.float32), aq, ec)
            t2[j % 2] = fma32(e, e, t2[j % 2])
            up, un = sub * KSUB + KSUB // 2 + j, sub * KSUB + KSUB // 2 - 1 - j
            e32[up], e32[un] = e
            sq[up], sq[un] = (e.astype(np.float64) ** 2).astype(np.float32)
    tt = (t2[0].astype(np.float64) + t2[1].astype(np.float64)).astype(np.float32)  # exact sum, one rounding
    t = lin + (float(tt[0]) + float(tt[1]))
    value = fma64(s, t, s * float(TILE))
    # exact: e_u = 1 - (1 + x_u^2) s at x_u = x_m + k_u h, and the true function there
    xs = [Fraction(xm) + Fraction(u - 0.5 * (TILE - 1)) * Fraction(h) for u in range(TILE)]
    e_exact = [1 - (1 + x * x) * Fraction(s) for x in xs]
    err = np.array([abs(float(Fraction(float(sq[u])) - e_exact[u] ** 2)) for u in range(TILE)])
    vals = np.array([s * float(1 + e_exact[u] + e_exact[u] ** 2) for u in range(TILE)])
    x87 = np.array([np.longdouble(fl(x)) + np.longdouble(float(x - Fraction(fl(x)))) for x in xs])
    true = (np.longdouble(1) / (np.longdouble(1) + x87 * x87)).sum()
    return value, float(true), s * err / np.spacing(vals), max(abs(float(e)) for e in e_exact)


N = 96_000_001
TILES = N // TILE
CASES = [  # (a, b, n, tile)
    pytest.param(0.0, 1.0, N, 0, id="unit-first"),
    pytest.param(0.0, 1.0, N, TILES // 2, id="unit-middle"),
    pytest.param(0.0, 1.0, N, TILES - 1, id="unit-last"),
    # the tile whose samples straddle x = 0 (sample 96 000 000.67 of the launch)
    pytest.param(-1.0, 0.5, 144_000_001, 250_000, id="across-zero"),
    pytest.param(8.0, 9.0, N, 1000, id="eight-to-nine"),
    pytest.param(0.0, 1.0, 10**10, 10**10 // 3 // TILE, id="n-1e10"),
]


@pytest.mark.parametrize("a,b,n,tile", CASES)
def test_model_of_one_tile(a, b, n, tile):
    """The squared term of every sample inside the derived bound, and the tile's value equal
    to the x87 sum of the true function to 1e-15."""
    h = (b - a) / n
    if a < 0:
        assert a + TILE * tile * h < 0.0 < a + TILE * (tile + 1) * h
    value, true, err_ulp, e_max = model_tile(a, b, n, tile)
    print(f"[{a}, {b}] n={n} tile={tile}: max |e| {e_max:.3e}, squared "
          f"term off by at most {err_ulp.max():.3e} ulp of the value (bound {BOUND_ULP:.3e}), "
          f"tile rel {(value - true) / true:.3e}")
    assert e_max <= E_MAX
    assert err_ulp.max() <= BOUND_ULP, err_ulp.max()
    assert value == pytest.approx(true, rel=1e-15, abs=0)


def test_the_bound_is_under_a_fiftieth_of_an_ulp():
    assert BOUND_ULP < 1 / 50
