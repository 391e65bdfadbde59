"""The bit-exact reference of the adaptive integrators (cuda_v_mpi_amd/utils/adaptive_exact.py)
checked on its own, without a GPU: its fma against libm, its rule against exact rationals, the
identities of its results, its agreement with the loose numpy model where no decision is
borderline, and, from the reference alone, that every case of expr_adaptive_exact_cases.py
takes the path it is there for. The last section changes the reference in one place at a time
(the decision order, the floor constant, the butterfly order, the prefix runs, the tie rule, a
sweep row's order) and shows that the cases notice.

test_expr_adaptive_exact_gpu.py holds the device to these same reference runs bit for bit.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math
import os
import random
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive_exact_cases as ec
from cuda_v_mpi_amd.utils import adaptive_exact as ax
from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_model

U = 2.0 ** -53


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------ fma
def _triples(count=200_000, seed=1):
    """Plain triples, exact and near cancellation, products of 27-bit factors that land on or
    beside a tie, and the far ends of the exponent range."""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        a = rng.uniform(-2, 2) * 2.0 ** rng.randint(-30, 30)
        b = rng.uniform(-2, 2) * 2.0 ** rng.randint(-30, 30)
        kind = i % 5
        if kind == 0:
            c = rng.uniform(-2, 2) * 2.0 ** rng.randint(-60, 60)
        elif kind == 1:
            c = -a * b
        elif kind == 2:
            c = -a * b * (1 + rng.choice([-1, 1]) * 2.0 ** -rng.randint(40, 53))
        elif kind == 3:
            a = float(rng.randint(1, 2 ** 27))
            b = float(rng.randint(1, 2 ** 27)) * 2.0 ** -rng.randint(50, 56)
            c = math.ldexp(rng.randint(1, 3), rng.randint(-20, 20))
        else:
            a = rng.uniform(-1, 1) * 2.0 ** rng.randint(-600, 600)
            b = rng.uniform(-1, 1) * 2.0 ** rng.randint(-600, 600)
            c = rng.uniform(-1, 1) * 2.0 ** rng.randint(-1074, 1000)
        out.append((a, b, c))
    return out


def test_fma_is_libms_on_200000_triples():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    t = _triples()
    want = np.array([libm.fma(*x) for x in t])
    scalar = np.array([ax.fma(*x) for x in t])
    arr = np.array(t)
    vec = ax.fma_vec(arr[:, 0], arr[:, 1], arr[:, 2])
    assert int((_bits(scalar) != _bits(want)).sum()) == 0
    assert int((_bits(vec) != _bits(want)).sum()) == 0
    # two roundings differ from one on a good share of these: the check can tell them apart
    with np.errstate(all="ignore"):
        twice = arr[:, 0] * arr[:, 1] + arr[:, 2]
    assert int((_bits(twice) != _bits(want)).sum()) > 1000


def test_fma_special_values_take_the_plain_path():
    inf, nan = math.inf, math.nan
    for a, b, c in [(0.0, 5.0, -0.0), (-0.0, 5.0, 0.0), (inf, 2.0, 1.0), (inf, 0.0, 1.0),
                    (1.0, 2.0, nan), (1e308, 10.0, -inf), (2.0, 3.0, 0.0), (2.0, 3.0, -0.0)]:
        got, vec = ax.fma(a, b, c), float(ax.fma_vec(a, b, c))
        want = a * b + c
        assert (math.isnan(got) and math.isnan(want)) or _bits(got) == _bits(want)
        assert (math.isnan(vec) and math.isnan(want)) or _bits(vec) == _bits(want)
    assert ax.fma(1e200, 1e200, 1.0) == inf and ax.fma(-1e200, 1e200, 1.0) == -inf
    assert ax.fma(2.0 ** -600, 2.0 ** -600, 2.0 ** -1074) == 2.0 ** -1074  # a subnormal result


# ------------------------------------------------------------------ the rule
def _gk15_scalar(f, lo, hi):
    """miint_gk15 with the scalar fma, one interval: the text of the macro, line by line."""
    t, wk, wg = ax.table()
    hw = 0.5 * (hi - lo)
    c = lo + hw
    f0 = f(c)
    sk, sg, sa = wk[0] * f0, wg[0] * f0, wk[0] * abs(f0)
    for j in range(1, 8):
        f1, f2 = f(ax.fma(hw, -t[j], c)), f(ax.fma(hw, t[j], c))
        sk = ax.fma(wk[j], f1 + f2, sk)
        sa = ax.fma(wk[j], abs(f1) + abs(f2), sa)
        if j % 2 == 0:
            sg = ax.fma(wg[j // 2], f1 + f2, sg)
    kv, gv = hw * sk, hw * sg
    return kv, abs(kv - gv), hw * sa


INTERVALS = [(0.0, 1.0), (0.0, 1.0 / 3.0), (-1.0, 2.5), (0.3, 0.3000001), (1e-9, 7.0),
             (-3.0, -1.0 / 7.0)] + [(i / 16.0, (i + 1) / 16.0) for i in range(16)]


@pytest.mark.parametrize("name", ["x", "one", "kink"])
def test_rule_matches_the_scalar_chain_and_the_rational_integral(name):
    """K of x and of 1.0 against the exact integral. The bound, in u = 2^-53 of R: the node
    (1, f = x takes it over), the pair sum (1), eight chained fma (8), the weight's own
    rounding (1), hw, c and the product hw * sk (3): 14; the test uses 16."""
    f = {"x": lambda x: x + 0.0, "one": lambda x: 1.0 + 0.0 * x,
         "kink": lambda x: abs(x - 1.0 / 3.0)}[name]
    lo = np.array([p[0] for p in INTERVALS])
    hi = np.array([p[1] for p in INTERVALS])
    k, err, r = ax.gk15(f, lo, hi)
    for i, (a, b) in enumerate(INTERVALS):
        ks, es, rs = _gk15_scalar(f, a, b)
        assert (_bits(k[i]), _bits(err[i]), _bits(r[i])) == (_bits(ks), _bits(es), _bits(rs))
        if name == "kink":
            continue
        fa, fb = Fraction(a), Fraction(b)
        truth = (fb * fb - fa * fa) / 2 if name == "x" else fb - fa
        assert abs(Fraction(float(k[i])) - truth) <= Fraction(16 * U) * Fraction(float(r[i]))
        assert err[i] <= 16 * U * r[i]  # K and G are both exact for a line


def test_the_sums_have_the_documented_orders():
    """Each order against a literal transcription on values where the order shows."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64)
    lanes = list(v)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i ^ o] for i in range(64)]
    assert float(ax.wave_sum(v)) == lanes[0]
    w = rng.standard_normal(700) * 10.0 ** rng.integers(-8, 8, 700)
    got = ax.block_sums(w)
    assert got.shape == (3,)
    for b in range(3):
        part = np.zeros(256)
        chunk = w[256 * b:256 * b + 256]
        part[:chunk.size] = chunk
        red = [float(ax.wave_sum(part[64 * q:64 * q + 64])) for q in range(4)]
        assert got[b] == (red[0] + red[1]) + (red[2] + red[3])
    chain = [0.0] * 256
    for i, x in enumerate(w):
        chain[i % 256] += x
    assert ax.close_sum(w) == float(ax.block_sums(np.array(chain))[0])
    blk = rng.standard_normal((600, 5))
    sums, per = ax.prefix_sums(blk)
    assert per == 3
    s = np.zeros((256, 5))
    for t in range(200):
        for b in range(3 * t, 3 * t + 3):
            s[t] += blk[b]
    assert sums == [float(ax.block_sums(s[:, q])[0]) for q in range(5)]
    row = [0.0] * 64
    for i, x in enumerate(w[:150]):
        row[i % 64] += x
    assert ax.row_wave_sum(w[:150]) == float(ax.wave_sum(np.array(row)))


# ------------------------------------------------------------------ identities
def _tiles(part, a, b):
    assert part[0, 0] == a and part[-1, 1] == b
    assert np.array_equal(_bits(part[:-1, 1]), _bits(part[1:, 0]))


@pytest.mark.parametrize("case", ec.CASES_1D, ids=repr)
def test_identities_1d(case):
    r = ec.reference(case)
    panels = case.opts["panels"]
    assert r["intervals"] == panels + r["splits"]
    assert r["evals"] == 15 * (r["intervals"] + r["splits"]) == 15 * sum(r["lengths"])
    assert r["rounds"] == len(r["lengths"]) and r["lengths"][0] == panels
    assert r["done"].shape == (r["intervals"], 2) and not np.isnan(r["done"]).any()
    assert r["intervals"] == r["within"] + r["floor"] + r["forced"] + r["nonfinite"] + (
        r["round_info"][-1]["splits"] if r["capped"] else 0)
    if r["range"] == "finite":
        _tiles(r["partition"], case.a, case.b)
    else:
        _tiles(r["partition"], 0.0, 1.0)
    assert r["intervals"] <= case.opts.get("max_intervals", 1 << 22)


@pytest.mark.parametrize("case", ec.CASES_2D, ids=repr)
def test_identities_2d(case):
    r = ec.reference(case)
    px, py = case.opts["panels"]
    assert r["intervals"] == px * py + r["splits"] and r["splits"] == r["splits_x"] + r["splits_y"]
    assert r["evals"] == 225 * (r["intervals"] + r["splits"])
    p = r["partition"]
    assert np.all(p[:, 0] < p[:, 1]) and np.all(p[:, 2] < p[:, 3])
    area = sum((Fraction(x1) - Fraction(x0)) * (Fraction(y1) - Fraction(y0))
               for x0, x1, y0, y1 in p.tolist())
    ax_, bx, ay, by = (Fraction(v) for v in case.box)
    assert area == abs(bx - ax_) * abs(by - ay)
    # no two rectangles share their lower corner, and every one lies in the box
    assert len({(x0, y0) for x0, _, y0, _ in p.tolist()}) == len(p)
    assert p[:, 0].min() == min(case.box[:2]) and p[:, 1].max() == max(case.box[:2])


@pytest.mark.parametrize("case", ec.SWEEP_CASES, ids=repr)
def test_identities_sweep(case):
    r = ec.reference(case)
    panels = case.opts["panels"]
    assert np.array_equal(r["intervals"], panels + r["splits"])
    assert np.array_equal(r["evals"], 15 * (r["intervals"] + r["splits"]))
    assert r["call_evals"] == int(r["evals"].sum()) == 15 * sum(r["lengths"])
    assert r["call_rounds"] == int(r["rounds"].max()) and r["peak"] == len(case.params) * panels
    assert np.all(r["intervals"] <= case.opts["max_intervals"])


# ------------------------------------------------------------------ the loose model agrees
@pytest.mark.parametrize("panels", [1, 16])
@pytest.mark.parametrize("name", ["kink", "step"])
def test_counters_and_partition_equal_the_loose_models(name, panels):
    """No decision of these runs is borderline, so the model (pairwise sums, two roundings for
    one fma) must take every one of them the same way; its sums may differ in their last bits."""
    f = {"kink": lambda x: np.abs(x - 1.0 / 3.0),
         "step": lambda x: np.where(x < 0.3, 1.0, 0.0)}[name]
    r = ax.adaptive_exact(f, 0.0, 1.0, panels=panels)
    m = adaptive_model(f, 0.0, 1.0, panels=panels)
    for key in ("rounds", "evals", "intervals", "splits", "floor", "forced", "nonfinite",
                "capped", "converged"):
        assert r[key] == m[key], key
    assert np.array_equal(_bits(r["partition"][:, 0]), _bits(m["lo"]))
    assert np.array_equal(_bits(r["partition"][:, 1]), _bits(m["hi"]))
    assert abs(r["value"] - m["value"]) <= 64 * U * r["resabs"]


# ------------------------------------------------------------------ each case does its job
def _ref(name):
    return ec.reference(ec.BY_NAME.get(name) or ec.BY_NAME_2D.get(name) or ec.BY_NAME_SWEEP[name])


def test_every_branch_is_taken_and_for_the_stated_reason():
    r = _ref("x-floor")
    assert r["floor"] >= 1 and r["forced"] == 0 and r["rounds"] == 1  # rounding noise over tol
    r = _ref("zig-depth3")
    assert r["forced"] >= 1 and r["rounds"] == 4 and r["forced"] == r["lengths"][-1]
    r = _ref("zig-depth0")
    assert r["rounds"] == 1 and r["forced"] == 256 and r["splits"] == 0 and not r["converged"]
    assert sum(_ref(c.name)["within"] for c in ec.CASES_1D) >= 1
    print({c.name: {k: _ref(c.name)[k] for k in ("within", "floor", "forced")}
           for c in ec.CASES_1D + ec.CASES_2D})


def test_the_step_runs_to_full_depth_and_the_midpoint_test_never_fires():
    """The case meant to reach `forced` by c == lo. From the reference: the run bisects
    down to intervals one or two doubles wide (57 rounds from [-1, 1]), and no interval is ever
    forced. It cannot be: c rounds onto an end only when hw is at most half a step of the
    doubles there, and then every node fma(hw, -+t, c), |t| < 1, rounds onto c as well. Fifteen
    equal samples leave err at the rounding of two weight sums, a few 2^-53 of R, so `within`
    or `floor` has accepted the interval before the midpoint is looked at. (The lone exception,
    lo a power of two whose lower neighbours are twice as dense, is never reached either: its
    ancestors [lo, lo + w] keep every node on one side of lo.) The device is held to the same
    run bit for bit, so a kernel that did force here would fail."""
    r = _ref("box-midpoint")
    w = r["partition"][:, 1] - r["partition"][:, 0]
    lo = r["partition"][:, 0]
    steps = w[lo != 0.0] / np.spacing(np.abs(lo[lo != 0.0]))
    assert r["rounds"] >= 54 and float(steps.min()) <= 2.0
    assert r["forced"] == 0 and r["floor"] == 0 and r["converged"]


def test_panels_and_workgroup_shapes():
    assert [_ref(f"zig-{p}")["round_info"][0]["nb"] for p in (1, 3, 256, 257)] == [1, 1, 1, 2]
    assert _ref("zig-257")["lengths"][0] % 256 == 1
    # many kinks: rounds with at least three workgroups that hold both kinds
    mixed = [i["mixed_blocks"] for i in _ref("zig-1000")["round_info"]]
    assert sum(m >= 3 for m in mixed) >= 5
    for name in ("zig-1", "zig-3", "zig-256", "zig-257"):
        assert max(i["mixed_blocks"] for i in _ref(name)["round_info"]) >= 3


def test_per_two_round_exists_with_splits_where_required():
    r = _ref("zig-per2")
    first = r["round_info"][0]
    assert (first["n"], first["nb"], first["per"]) == (65537, 257, 2)
    assert {0, 1, 256} <= set(first["split_blocks"].tolist())  # thread 0's run, the last one
    assert first["splits"] >= 1000 and not r["capped"] and r["converged"]
    assert all(i["per"] == 1 for i in r["round_info"][1:])
    c = _ref("zig-per2-capped")
    info = c["round_info"][0]
    assert c["capped"] and c["rounds"] == 1 and c["splits"] == 0 and c["intervals"] == 65537
    assert info["per"] == 2 and info["splits"] > 64  # pending sums to add, over the cap by many
    # the capped total is the uncapped first round's accepted and pending sums, added once
    assert c["value"] != r["value"] and c["resabs"] < r["resabs"]
    print("per = 2 reference wall time, s:", ec.WALL.get("zig-per2"),
          "capped:", ec.WALL.get("zig-per2-capped"))


def test_tolerance_regimes_and_reversal():
    a, r = _ref("zig-atol"), _ref("zig-rtol")
    assert a["tol"] == 1e-6 and a["tol"] > 1e-12 * abs(a["value"]) * 2
    assert r["tol"] > 1e-12 and 0.5 < r["tol"] / (1e-6 * abs(r["value"])) < 2.0
    f, b = _ref("zig-3"), _ref("zig-reversed")
    assert _bits(b["value"]) == _bits(-f["value"]) and b["evals"] == f["evals"]
    assert np.array_equal(_bits(b["partition"]), _bits(f["partition"][::-1, ::-1]))
    assert np.array_equal(_bits(b["done"]), _bits(f["done"]))  # the rounds ran on [b, a]


def test_infinite_ranges():
    for kind in ("upper", "lower", "both"):
        for panels in (1, 16):
            r = _ref(f"box-{kind}-{panels}")
            assert r["range"] == kind and r["lengths"][0] == panels and r["splits"] >= 50
            assert abs(r["value"] - 1.0) <= 1e-9  # the box lies inside every one of the ranges


def test_sweep_structure():
    c, r = ec.SWEEP, ec.reference(ec.SWEEP)
    assert len(c.params) >= 70 and c.opts["panels"] % 64 != 0 and c.opts["panels"] > 64
    assert (r["rounds"] == 1).sum() >= 10 and (r["rounds"] > 20).sum() >= 10
    assert c.params[40] == c.params[10]
    for key in ax.ROW_FIELDS:
        assert _bits(r[key][40].astype(np.float64)) == _bits(r[key][10].astype(np.float64)), key
    # rows leave: the list of active rows shrinks after round 1 and keeps row order
    assert len(r["actives"][0]) == 72 and len(r["actives"][1]) == 60
    assert all(a == sorted(a) for a in r["actives"])
    assert r["intervals"].argmax() == ec.HARD_ROW and (r["intervals"] == 171).sum() == 1
    k = ec.reference(ec.SWEEP_CAPPED)
    assert k["capped"].nonzero()[0].tolist() == [ec.HARD_ROW] and not k["converged"][ec.HARD_ROW]
    others = np.arange(72) != ec.HARD_ROW
    for key in ax.ROW_FIELDS:  # a > b there: the values negated, the rest untouched
        want = -r[key] if key == "value" else r[key]
        assert np.array_equal(_bits(k[key][others].astype(np.float64)),
                              _bits(want[others].astype(np.float64))), key
    # a row's decisions are ExprAdaptive's: the counters of one row alone, by the 1-D rounds
    p0, p1 = c.params[ec.HARD_ROW]
    one = ax.adaptive_exact(lambda x: p1 * np.abs(x - p0), 0.0, 1.0, panels=150, rtol=1e-10)
    for key in ("rounds", "evals", "intervals", "splits", "floor", "forced"):
        assert one[key] == r[key][ec.HARD_ROW], key


def test_two_dimensional_structure():
    assert _ref("sum-17x16")["round_info"][0]["nb"] == 2
    assert _ref("sum-3x5")["lengths"][0] == 15 and _ref("sum-1x1")["lengths"][0] == 1
    rx, ry = _ref("ridge-x"), _ref("ridge-y")
    assert rx["splits_x"] >= 3 and rx["splits_y"] == 0
    assert ry["splits_y"] >= 3 and ry["splits_x"] == 0
    sq, wide = _ref("sum-1x1"), _ref("sum-wide-box")
    assert sq["ties"] >= 1 and sq["ties_to_y"] == 0          # a square box: a tie goes to x
    assert wide["ties_to_y"] >= 1                            # a 2 x 1 box, square cells: to y
    dx, dy = _ref("step-x-depth"), _ref("step-y-depth")
    assert dx["forced_by_depth"] >= 1 and dx["splits_y"] == 0 and dx["forced"] >= 1
    assert dy["forced_by_depth"] >= 1 and dy["splits_x"] == 0
    for key in ("rounds", "evals", "intervals", "forced", "forced_by_depth"):
        assert dx[key] == dy[key], key                       # the transpose, depth in the high half
    assert (dx["splits_x"], dx["splits_y"]) == (dy["splits_y"], dy["splits_x"])
    assert _bits(dx["value"]) == _bits(dy["value"])
    cap = _ref("sum-capped")
    assert cap["capped"] and cap["rounds"] == 1 and cap["intervals"] == 272
    assert cap["round_info"][0]["splits"] > 28 and cap["round_info"][0]["nb"] == 2
    assert _bits(_ref("sum-flipped")["value"]) == _bits(-_ref("sum-3x5")["value"])


# ------------------------------------------------------------------ a changed reference is seen
def _same(a, b, keys=("value", "err_est", "resabs", "tol", "rounds", "evals", "intervals",
                      "splits", "floor", "forced")):
    return all(_bits(float(a[k])) == _bits(float(b[k])) for k in keys)


def _rerun(name, **changed):
    c = ec.BY_NAME[name]
    return ax.adaptive_exact(ec.F[c.expr], c.a, c.b, **c.opts, **changed)


def test_a_changed_decision_order_is_noticed():
    assert _same(_rerun("x-floor"), _ref("x-floor"))
    swapped = _rerun("x-floor", order="nfwF")     # floor before within
    assert swapped["floor"] != _ref("x-floor")["floor"]
    # forced before within: at depth 5 many intervals of this run are within tolerance
    base, forced_first = _rerun("zig-atol", max_depth=5), _rerun("zig-atol", max_depth=5,
                                                                 order="nFwf")
    assert base["within"] >= 50 and forced_first["forced"] > base["forced"]


def test_a_changed_floor_constant_is_noticed():
    """zig-floor asks for more than rounding allows, so only the floor (or an err of exactly 0)
    ends a branch, thousands of them before the cap: some land between any two constants a few
    per cent apart."""
    want = _ref("zig-floor")
    assert want["floor"] >= 1000 and max(want["lengths"]) > 10000 and want["capped"]
    for const in (49.0, 51.0):
        changed = _rerun("zig-floor", floor_const=const * 2.0 ** -52)
        assert changed["floor"] != want["floor"] and changed["evals"] != want["evals"], const
    assert _rerun("x-floor", floor_const=2.0 ** -52)["floor"] != _ref("x-floor")["floor"]


def test_a_changed_butterfly_order_is_noticed(monkeypatch):
    """Totals of many same-sized terms absorb most one-bit differences below them, so a given
    case sees another order only sometimes; these four do, in their value, tol or resabs."""
    monkeypatch.setattr(ax, "_XOR", ax._XOR[::-1])   # 1, 2, ..., 32
    for name in ("zig-1", "zig-256", "zig-rtol", "zig-per2"):
        assert not _same(_rerun(name), _ref(name)), name


def test_changed_prefix_run_bounds_are_noticed():
    # floor(nb / 256) workgroups a run: the 257th, which holds a split, is left out
    lost = _rerun("zig-per2-capped", per_of=lambda nb: max(nb // 256, 1))
    assert not _same(lost, _ref("zig-per2-capped"))
    # runs of three: nothing lost, the grouping of the sums alone
    regrouped = _rerun("zig-per2-capped", per_of=lambda nb: (nb + 255) // 256 + 1)
    assert not _same(regrouped, _ref("zig-per2-capped"))


def test_a_changed_tie_rule_is_noticed():
    c = ec.BY_NAME_2D["sum-1x1"]
    other = ax.adaptive2d_exact(ec.F[c.expr], *c.box, **c.opts, tie="gt")
    want = _ref("sum-1x1")
    assert (other["splits_x"], other["splits_y"]) != (want["splits_x"], want["splits_y"])


def test_a_changed_row_sum_order_is_noticed():
    c = ec.SWEEP
    chained = ax.adaptive_sweep_exact(ec.F[c.expr], np.array(c.params), c.a, c.b, **c.opts,
                                      row_sum=lambda v: float(sum(v.tolist(), 0.0)))
    want = ec.reference(c)
    assert not np.array_equal(_bits(chained["value"]), _bits(want["value"]))
    assert np.array_equal(chained["intervals"], want["intervals"])
