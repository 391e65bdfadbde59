"""The long tile of div series_exact (integrands.hpp Pi4Long), checked without a GPU.

Assembly of its one-step, multi-step and queue kernels through tools/isa_guard.py: at most
1.06 VALU per sample in the tile block (1601 per 1536 measured: 1536 + 36 v_pk_fma_f32 for the
samples and the twelve +-c0 centre and slope pairs, and what is paid once per tile), no packed
FMA directly behind the packed operation it reads from, at most 64 VGPRs, no scratch, and the
occupancy of the same kernel form's Pi4 row; and every row of tools/isa_baseline.json that
existed before this tile is still the parent's.

A numpy model of one long tile, fp32 operations in the kernel's order, against exact rational
arithmetic: every sample's squared term inside the bound derived above Pi4Long (|de| <= 5 u E,
|d(e^2)| <= 2 E |de| + u E^2 + 2 E 651 h^2 of a value of order 1, u = 2^-24, E = 2e-6), and
the tile's value inside pi4_truth's bound for the long tile against the truth.

The dispatcher, host only: the long tile runs exactly where 768 |h| <= 2e-6."""
from __future__ import annotations

import hashlib
import json
import os
import re
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from cuda_v_mpi_amd.models import integrands
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import pi4_truth as pt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import isa_guard  # noqa: E402

TILE, SUB, SUBS, KPAIRS = 1536, 64, 24, 16
LONG = {"pi4_series_exact_long": "pi4_series_exact",
        "ms_pi4_series_exact_long": "ms_pi4_series_exact",
        "q_pi4_series_exact_long": "q_pi4_series_exact"}


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
    return isa_guard.stats(body, info, tile), body


def tile_block(body: str) -> list[str]:
    """Instructions of the straight-line block with the most VALU (one tile)."""
    blocks, _ = isa_guard.cfg(body)
    return max(blocks, key=lambda b: sum(1 for s in b if s.startswith("v_")))


@pytest.mark.parametrize("name", sorted(LONG))
def test_tile_block_counts_and_residency(functions, name):
    st, body = kernel(functions, name)
    short, _ = kernel(functions, LONG[name])
    ops = [s.split()[0] for s in tile_block(body)]
    valu = sum(1 for o in ops if o.startswith("v_"))
    print(f"{name}: {valu} VALU per tile ({valu / TILE:.4f} per sample), "
          f"{ops.count('v_pk_fma_f32')} v_pk_fma_f32, {ops.count('s_nop')} s_nop, "
          f"{st['vgpr']} VGPRs, {st['sgpr']} SGPRs, occupancy {st['occupancy']} "
          f"(Pi4 row: {short['occupancy']})")
    assert valu <= st["max_block_valu"] <= 1.06 * TILE
    assert ops.count("v_pk_fma_f32") >= 1536 + 36
    assert st["vgpr"] <= 64 and st["scratch"] == 0 and st["hot_loop_scratch_ops"] == 0
    assert st["occupancy"] >= short["occupancy"]


@pytest.mark.parametrize("name", sorted(LONG))
def test_no_packed_fma_reads_what_the_instruction_before_it_wrote(functions, name):
    """Inside an asm statement the compiler adds no wait states, so a v_pk_fma_f32 never
    directly follows the packed operation that wrote one of its sources (an s_nop or any other
    instruction between them counts as the wait)."""
    prev_dst = None
    for ins in tile_block(kernel(functions, name)[1]):
        op, _, rest = ins.partition(" ")
        args = [a.strip() for a in re.split(r" (?:op_sel|neg_)", rest)[0].split(",")]
        if op == "v_pk_fma_f32":
            assert prev_dst is None or prev_dst not in args[1:], ins
        prev_dst = args[0] if op.startswith("v_pk_") else None


# the rows of tools/isa_baseline.json before the long tile: their names, and the SHA-256 of
# json.dumps(rows, sort_keys=True)
PARENT_ROWS = 37
PARENT_SHA256 = "2229d37249d43f43d483e0d8c0042cfdb1043da22dd5288b8beca7ada04857ec"


def test_existing_baseline_rows_did_not_move():
    with open(isa_guard.BASELINE) as f:
        base = json.load(f)
    assert set(LONG) <= set(base)
    old = {k: v for k, v in base.items() if k not in LONG}
    assert len(old) == PARENT_ROWS
    assert hashlib.sha256(json.dumps(old, sort_keys=True).encode()).hexdigest() == PARENT_SHA256


def test_baseline_rows_of_the_long_kernels():
    with open(isa_guard.BASELINE) as f:
        base = json.load(f)
    for name, short in LONG.items():
        row = base[name]
        assert row["max_block_valu"] <= 1.06 * TILE and row["vgpr"] <= 64 and row["scratch"] == 0
        assert row["occupancy"] >= base[short]["occupancy"]


# ------------------------------------------------------------------ the numpy model of a tile
MEAN_K2 = 341.25
SUM_K2 = 301989760.0
E_MAX = 2e-6          # |e| of every sample of an admitted launch (series_ok_long)
H_MAX = E_MAX / 768   # the largest admitted step
U32 = 2.0**-24
# the bound of the comment above Pi4Long, relative to a value of order 1 ...
D_E = 5 * U32 * E_MAX
BOUND = 2 * E_MAX * D_E + U32 * E_MAX**2 + 2 * E_MAX * 651 * H_MAX**2
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
    """One 1536-sample tile of the left rule as Pi4Long::tile_acc evaluates it. Returns (the
    tile's value without h * 4, per-sample error of the squared term in ulp of the sample's
    value, max |e|)."""
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
    # seed_f32: p1 = (A, B), p2 = (e_m + 341.25 B, 2 B)
    af, bf = np.float32(A), np.float32(B)
    basef, b2f = np.float32(fma64(MEAN_K2, B, em)), np.float32(bf + bf)
    kf = (np.arange(2 * KPAIRS) + 0.5).astype(np.float32)
    ta, tb = np.zeros(2, np.float32), np.zeros(2, np.float32)
    sq = np.zeros(TILE, np.float32)
    for i in range(SUBS // 2):
        # the pair of sub-tiles at -c0 and +c0: in, A', e_c on (c0, -c0)
        c0 = np.float32(SUB * (i + 0.5))
        cc = np.array([c0, -c0], np.float32)
        ecs = fma32(cc, fma32(cc, bf, af), basef)
        aqs = fma32(cc, b2f, af)
        for half in (1, 0):  # the sub-tile at -c0 (high halves) first
            centre = (TILE // 2) + int(cc[half])  # index of the first sample right of it
            for j in range(KPAIRS):
                k0 = np.array([kf[j], -kf[j]], np.float32)
                k1 = np.array([kf[j + KPAIRS], -kf[j + KPAIRS]], np.float32)
                e0 = fma32(k0, aqs[half], ecs[half])
                e1 = fma32(k1, aqs[half], ecs[half])
                ta = fma32(e0, e0, ta)
                tb = fma32(e1, e1, tb)
                for e, jj in ((e0, j), (e1, j + KPAIRS)):
                    sq[centre + jj], sq[centre - 1 - jj] = (e.astype(np.float64) ** 2).astype(np.float32)
    tt = (ta.astype(np.float64) + tb.astype(np.float64)).astype(np.float32)
    t = lin + (float(tt[0]) + float(tt[1]))
    value = fma64(s, t, s * float(TILE))
    # exact: e_u = 1 - (1 + x_u^2) s at x_u = x_m + k_u h
    xs = [Fraction(xm) + Fraction(u - 0.5 * (TILE - 1)) * Fraction(h) for u in range(TILE)]
    e_exact = [1 - (1 + x * x) * Fraction(s) for x in xs]
    err = np.array([abs(float(Fraction(float(sq[u])) - e_exact[u] ** 2)) for u in range(TILE)])
    vals = np.array([s * float(1 + e_exact[u] + e_exact[u] ** 2) for u in range(TILE)])
    return value, s * err / np.spacing(vals), max(abs(float(e)) for e in e_exact)


N = 384_000_001
TILES = N // TILE
CASES = [  # (a, b, n, tile)
    pytest.param(0.0, 1.0, N, 0, id="unit-first"),
    pytest.param(0.0, 1.0, N, TILES // 2, id="unit-middle"),
    pytest.param(0.0, 1.0, N, TILES - 1, id="unit-last"),
    # the tile whose samples straddle x = 0 (sample 384 000 000.67 of the launch)
    pytest.param(-1.0, 0.5, 576_000_001, 250_000, id="across-zero"),
    pytest.param(8.0, 9.0, N, 1000, id="eight-to-nine"),
    pytest.param(0.0, 1.0, 10**10, 10**10 // 3 // TILE, id="n-1e10"),
]


@pytest.mark.parametrize("a,b,n,tile", CASES)
def test_model_of_one_tile(a, b, n, tile):
    """The squared term of every sample inside the derived bound, and the tile's value inside
    pi4_truth's bound of the long tile against the true sum of its samples."""
    h = (b - a) / n
    assert pt.long_tile_admitted(h)
    if a < 0:
        assert a + TILE * tile * h < 0.0 < a + TILE * (tile + 1) * h
    value, err_ulp, e_max = model_tile(a, b, n, tile)
    g = pt.geometry(integrands.IntegrandSpec("pi4", a, b), n, "left", TILE * tile, TILE)
    S = pt.true_sum(g)
    err, bound = float(abs(pt.MP.mpf(value) - S)), pt.tile_truth_bound(pt.LONG_PATH, g, float(S))
    print(f"[{a}, {b}] n={n} tile={tile}: max |e| {e_max:.3e}, squared term off by at most "
          f"{err_ulp.max():.3e} ulp of the value (bound {BOUND_ULP:.3e}); tile against the "
          f"truth {err:.3e} (bound {bound:.3e}, {err / bound:.3f})")
    assert e_max <= E_MAX
    assert err_ulp.max() <= BOUND_ULP, err_ulp.max()
    assert err <= bound


def test_the_derived_bounds():
    """The per-sample bound of the squared term is under 1/40 ulp; the long tile's bound
    against its definition, at the largest admitted step, is the fold's 2 U64 and the fp32 sums'
    384 u E^2 for the most part, and not below the short tile's at the same step."""
    assert BOUND_ULP < 1 / 40
    g = pt.geometry(integrands.pi4(), N, "left", TILE * (TILES // 2), TILE)
    long, short = pt.tile_defn_rel(pt.LONG_PATH, g), pt.tile_defn_rel("fp64-series_exact", g)
    assert short <= long <= 3.6e-16   # 2 U64 + 384 u E^2 + E^3 + the squares' 2.7e-18
    assert pt.tile_len(pt.LONG_PATH) == TILE and pt.LONG_PATH not in pt.PATHS


# ------------------------------------------------------------------ the dispatcher (host only)
def tile_len(a, b, n, **kw):
    return kernels.riemann_tile_len(integrands.IntegrandSpec("pi4", a, b), n, **kw)


@pytest.mark.parametrize("a,b,n", [(0.0, 1.0, 384_000_000), (-1.0, 0.5, 576_000_000),
                                   (8.0, 9.0, 384_000_000)])
def test_long_tile_runs_exactly_where_the_step_admits_it(native, monkeypatch, a, b, n):
    monkeypatch.delenv("MIINT_PI4_TILE", raising=False)
    lo, hi = n + 1, n - 1
    assert 768 * ((b - a) / lo) <= 2e-6 < 768 * ((b - a) / hi)
    assert native.series_ok_long((b - a) / lo) and not native.series_ok_long((b - a) / hi)
    want = TILE if _auto_is_long() else 384   # auto: one choice wherever both are admitted
    assert tile_len(a, b, lo) == want and tile_len(a, b, lo, tile="long") == TILE
    assert tile_len(a, b, lo, tile="short") == 384
    assert tile_len(a, b, hi) == 384 and tile_len(a, b, hi, tile="short") == 384
    with pytest.raises(RuntimeError, match="tile = long"):
        tile_len(a, b, hi, tile="long")
    # a slice, another rule, the far end of the interval: a function of the step alone
    assert tile_len(a, b, lo, rule="mid", i_begin=lo - 5000, n_local=5000, tile="long") == TILE


def _auto_is_long() -> bool:
    """What `auto` picks where both tiles are admitted (kPi4LongTileAuto)."""
    return kernels.riemann_tile_len(integrands.pi4(), 10**9) == TILE


def test_auto_and_the_environment_override(native, monkeypatch):
    monkeypatch.delenv("MIINT_PI4_TILE", raising=False)
    auto = tile_len(0.0, 1.0, 10**9)
    assert auto in (384, TILE)
    monkeypatch.setenv("MIINT_PI4_TILE", "short")
    assert tile_len(0.0, 1.0, 10**9) == 384 and tile_len(0.0, 1.0, 10**9, tile="long") == TILE
    monkeypatch.setenv("MIINT_PI4_TILE", "long")
    assert tile_len(0.0, 1.0, 10**9) == TILE and tile_len(0.0, 1.0, 10**9, tile="short") == 384
    assert tile_len(0.0, 1.0, 96_000_001) == 384   # the override refuses nothing
    monkeypatch.setenv("MIINT_PI4_TILE", "wide")
    with pytest.raises(RuntimeError, match="MIINT_PI4_TILE"):
        tile_len(0.0, 1.0, 10**9)


def test_what_the_long_tile_is_refused_for(native, monkeypatch):
    monkeypatch.delenv("MIINT_PI4_TILE", raising=False)
    with pytest.raises(RuntimeError, match="tile = long"):
        tile_len(0.0, 1.0, 96_000_001, tile="long")
    for kw in (dict(dtype="fp32"), dict(div="series"), dict(div="ieee"), dict(div="series_direct")):
        assert tile_len(0.0, 1.0, 10**9, **kw) != TILE
        with pytest.raises(RuntimeError, match="tile = long"):
            tile_len(0.0, 1.0, 10**9, tile="long", **kw)
    with pytest.raises(RuntimeError, match="tile = long"):
        kernels.riemann_tile_len(integrands.sin(), 10**9, tile="long")
    with pytest.raises(RuntimeError, match="auto, short or long"):
        tile_len(0.0, 1.0, 10**9, tile="wide")


def test_degenerate_and_far_launches_go_where_they_went(native, monkeypatch):
    """a == b (h = 0) keeps the 384-sample tile, whose launches return 0; a far coordinate
    keeps the per-sample tiles and the library division (Pi4Wide)."""
    monkeypatch.delenv("MIINT_PI4_TILE", raising=False)
    assert not native.series_ok_long(0.0)
    assert tile_len(0.75, 0.75, 10**9) == 384
    with pytest.raises(RuntimeError, match="tile = long"):
        tile_len(0.75, 0.75, 10**9, tile="long")
    far = 2.0 ** 250
    D, V = native.DType, native.DivMode
    args = (0, far, 0.0, 0.0, 0, 10**6, [], 0.0, 0.0)
    assert str(native.riemann_effective_div(*args, D.fp64, V.series_exact)).endswith("ieee")
    assert not native.riemann_pi4_ieee_narrow(*args, D.fp64)
    assert tile_len(far, far, 10**9) == 32
    # just inside the narrow range, a fine step: the series tiles as before, the short one
    assert tile_len(2.0 ** 248, 2.0 ** 248, 10**9) == 384
