"""Every train-scan path, element by element and bit for bit, on a jagged table.

With integer table entries and dt = d / 2**k every sample, and every partial sum any kernel
can form in any order, is an integer multiple of 2**-k; below 2**53 of them fp64 holds all of
it exactly (cuda_v_mpi_amd/utils/exact_scan.py). So each path — the 3-kernel path, the
closed-form tile sums with the block-aggregate hand-off ("fused") or with the per-workgroup
fold ("fold", what TrainScan runs on one GPU), the one-pass look-back, and interp_scan followed
by inclusive_scan ("lookback") — must return exactly the int64 reference: a dropped, doubled
or misplaced sample, a wrong tile count, carry weight or segment index changes bits. No
tolerance anywhere; each test first asserts that its input keeps the budget.

The inputs live in scan_exact_cases.py (test_exact_scan_cpu.py checks their budgets on any
box). The reference of a case is computed once, on the device, and shared.
"""
from __future__ import annotations

import time

import pytest
import torch

import scan_exact_cases as cases
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import exact_scan as xs

pytestmark = pytest.mark.gpu

_TABLES: dict = {}
_REFS: dict = {}


def _table_f64(name: str) -> torch.Tensor:
    if name not in _TABLES:
        _TABLES[name] = torch.as_tensor(cases.table(name), device="cuda").to(torch.float64)
    return _TABLES[name]


def _reference(case):
    """(vel, pos, totals) of the case as fp64 device tensors; computed once, never modified."""
    if case not in _REFS:
        assert cases.budget(case) < 53, f"bad test input: {case} leaves the exactness budget"
        name, d, k, i0, n, window, _ = case
        ref = xs.exact_scan(cases.table(name), d, k, i0, n, window, cases.int_carries(case),
                            device="cuda")
        tot = xs.to_f64(torch.tensor(ref.totals, dtype=torch.int64, device="cuda"), k)
        _REFS[case] = (xs.to_f64(ref.vel, k), xs.to_f64(ref.pos, k), tot)
    return _REFS[case]


def _launch(algo: str, case):
    name, d, k, i0, n, window, carries = case
    tab, dt = _table_f64(name), xs.dt_of(d, k)
    has_carries = carries != (0.0, 0.0)
    if algo == "lookback":
        c1 = torch.tensor([carries[0]], dtype=torch.float64, device="cuda")
        c2 = torch.tensor([carries[1]], dtype=torch.float64, device="cuda")
        vel = kernels.interp_scan(n, i0=i0, dt=dt, window=window, table=tab,
                                  carry=c1 if has_carries else None)
        pos = kernels.inclusive_scan(vel, carry=c2 if has_carries else None)
        return vel, pos, None
    c = torch.tensor(carries, dtype=torch.float64, device="cuda") if has_carries else None
    return kernels.trainscan(n, i0=i0, dt=dt, window=window, carries=c, algo=algo, table=tab)


def _same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want).flatten()  # NaN != anything: counted too
    i = int(bad[0])
    pytest.fail(f"{what}: {bad.numel()} of {want.numel()} elements differ, first at {i}: "
                f"got {got[i].item()!r}, exact {want[i].item()!r}")


def _check(algo: str, case, label: str = "") -> None:
    want_vel, want_pos, want_tot = _reference(case)
    vel, pos, totals = _launch(algo, case)
    tag = f"{algo} {label or case[1:]}"
    _same(vel, want_vel, f"vel [{tag}]")
    _same(pos, want_pos, f"pos [{tag}]")
    if algo in ("fused", "onepass"):  # the only forms that write {T1, T2}
        _same(totals, want_tot, f"totals [{tag}]")
    else:
        assert totals is None


# ------------------------------------------------------------------ 4a sampling rates
@pytest.mark.parametrize("algo,dt", cases.algo_dts())
def test_sampling_rates(cuda, algo, dt):
    """n in {1, 4095, 4096, 4097, 2 tiles + 1, one block of 256 tiles + a tile + 1} at i0 in
    {0, 37}: one tile, a partial last tile, and two blocks (the fold runs with b = 1, the
    hand-off with two aggregates)."""
    for case in cases.sampling_cases(dt):
        _check(algo, case, f"dt={dt} n={case[4]} i0={case[3]}")


@pytest.mark.parametrize("dt", [d for d in cases.DTS if d not in cases.CLOSED])
def test_fold_refuses_where_it_does_not_apply(cuda, dt):
    d, k = cases.DTS[dt]
    with pytest.raises(RuntimeError, match="fold mode"):
        kernels.trainscan(4097, dt=xs.dt_of(d, k), algo="fold", table=_table_f64("jag7"))


def test_fold_refuses_beyond_64_blocks_and_carries(cuda):
    tab = _table_f64("jag7")
    with pytest.raises(RuntimeError, match="fold mode"):
        kernels.trainscan(64 * cases.BLOCK + 1, dt=1 / 64, algo="fold", table=tab)
    c = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="fold mode"):
        kernels.trainscan(4097, dt=1 / 64, algo="fold", carries=c, table=tab)


@pytest.mark.parametrize("dt", list(cases.DTS))
def test_interp_fill_on_the_jagged_table(cuda, dt):
    """The samples themselves (interp_fill's per-workgroup chunk windows), not yet summed."""
    d, k = cases.DTS[dt]
    tab = cases.table("jag7")
    for n, i0 in ((1, 0), (4097, 37), (cases.BLOCK + cases.TILE + 1, 37)):
        want = xs.to_f64(xs.exact_samples(tab, d, k, i0, n, device="cuda"), k)
        got = kernels.interp_fill(n, i0=i0, dt=xs.dt_of(d, k), table=_table_f64("jag7"))
        _same(got, want, f"interp_fill dt={dt} n={n} i0={i0}")


# ------------------------------------------------------------------ 4b flat tail
@pytest.mark.parametrize("algo", ["fused", "fold", "onepass"])
def test_flat_tail_four_blocks(cuda, algo):
    """3 * 2**20 + 4097 samples at dt = 1/64: all but the first 131 008 extrapolate the table's
    flat, non-zero last segment; four blocks of tiles (b runs to 3 in the fold, four hand-off
    aggregates). The budget is near 2**52 on purpose: the weights are at their largest."""
    _check(algo, cases.FLAT_TAIL, "flat tail")


# ------------------------------------------------------------------ 4c fill windows
@pytest.mark.parametrize("algo,dt", [p for p in cases.algo_dts() if p[1] in cases.WINDOW_DTS])
def test_fill_windows(cuda, algo, dt):
    """Samples outside the window are zero: the hot form (Sampler::plain_tile) may be taken
    only for tiles wholly inside it, the closed-form sums must clip their runs to it."""
    for w, case in cases.window_cases(dt).items():
        _check(algo, case, f"window {w} dt={dt}")


# ------------------------------------------------------------------ 4d carries
@pytest.mark.parametrize("dt", cases.CARRY_DTS)
@pytest.mark.parametrize("algo", ["fused", "lookback"])
def test_carries(cuda, algo, dt):
    """{C1, C2} = {12345.5, -987654.25}: C1 enters pos with weight (index + 1) — fma(t0, c1, .)
    per tile in ts_write — so every element checks it, not only the last."""
    for case in cases.carry_cases(dt):
        _check(algo, case, f"carries dt={dt} n={case[4]}")


# ------------------------------------------------------------------ 4e inclusive_scan, any data
@pytest.fixture(scope="module")
def random_ints(cuda):
    g = torch.Generator(device="cpu").manual_seed(77)
    return torch.randint(-2**20, 2**20 + 1, (1_000_003,), generator=g,
                         dtype=torch.int64).to("cuda")


@pytest.mark.parametrize("carry", [None, -987654.25])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 1_000_003])
def test_inclusive_scan_random_integers(random_ints, n, carry):
    """Integers within +-2**20 (sums below 2**40, the carry in quarters: exact) against the
    int64 cumsum, in units of 1/4."""
    x = random_ints[:n]
    want = torch.cumsum(x, 0) * 4 + (int(carry * 4) if carry is not None else 0)
    c = None if carry is None else torch.tensor([carry], dtype=torch.float64, device="cuda")
    got = kernels.inclusive_scan(x.to(torch.float64), carry=c)
    _same(got, xs.to_f64(want, 2), f"inclusive_scan n={n} carry={carry}")


# ------------------------------------------------------------------ 4f more than 256 blocks
def test_more_than_256_blocks(cuda):
    """2**28 + 3 * 4096 + 17 samples: 65 540 tiles in 257 blocks, so the last workgroup of
    ts_tile_scan_closed<true> makes a second trip through its block-aggregate loop. The
    samples that are not zero sit in a window of 2**13 in the middle, so pos grows linearly
    and stays exact. About 13 GB: every array is freed as soon as it is compared."""
    case = cases.BIG
    name, d, k, i0, n, window, _ = case
    assert cases.budget(case) < 51
    t0 = time.perf_counter()
    vel, pos, totals = kernels.trainscan(n, i0=i0, dt=xs.dt_of(d, k), window=window,
                                         algo="fused", table=_table_f64(name))
    x = xs.exact_samples(cases.table(name), d, k, i0, n, window, device="cuda")
    want = torch.cumsum(x, 0)
    del x
    t1 = int(want[-1])
    ok_vel = torch.equal(vel, xs.to_f64(want, k))
    del vel
    want = torch.cumsum(want, 0)  # the vel reference is released here
    t2 = int(want[-1])
    ok_pos = torch.equal(pos, xs.to_f64(want, k))
    del pos, want
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"more than 256 blocks: {time.perf_counter() - t0:.3f} s")
    assert ok_vel and ok_pos
    assert totals.tolist() == [t1 / 2**k, t2 / 2**k]


# ------------------------------------------------------------------ 4g staged windows, poisoned
@pytest.fixture()
def poison(native, cuda):
    native.set_lds_poison(True)
    try:
        yield
    finally:
        native.set_lds_poison(False)


@pytest.mark.parametrize("algo", ["fused", "fold", "onepass"])
def test_staged_window_poisoned(poison, algo):
    """dt = 1/1024 stages 6 table entries per tile; with the rest of the LDS window NaN, a
    read outside what was staged turns the arrays NaN (and torch.equal fails on NaN)."""
    d, k = cases.DTS["1/1024"]
    _check(algo, ("jag7", d, k, 37, 2 * cases.TILE + 1, None, (0.0, 0.0)), "poisoned")
    _check(algo, cases.window_cases("1/1024")["cuts_both_ends"], "poisoned, window")
