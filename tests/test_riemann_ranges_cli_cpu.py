"""CPU tests of the native CLI's --ranges and --curve-rtol / --curve-atol modes (csrc/cli/
riemann.cpp): every refusal comes before any device call and names the conflict, and the
refusals the CLI had keep their words."""
from __future__ import annotations

import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _riemann(*args, env=None):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def _refused(*args, env=None) -> str:
    p = _riemann(*args, env=env)
    assert p.returncode == 1 and p.stdout == "", (p.stdout, p.stderr)
    return p.stderr


CURVE = ("--expr", "exp(-x*x)", "--curve-rtol", "1e-9", "--a", "0", "--b", "3", "--points", "10")
WHO = "--curve-rtol / --curve-atol"
CONFLICTS = [
    (("--n", "1e6"), "--n"), (("--rule", "mid"), "--rule"), (("--running",), "--running"),
    (("--rtol", "1e-8"), "--rtol"), (("--atol", "1e-8"), "--atol"),
    (("--row-rtol", "1e-8"), "--row-rtol"), (("--area-rtol", "1e-8"), "--area-rtol"),
    (("--ya", "0", "--yb", "1"), "--ya"), (("--box", "0:1,0:1"), "--box"),
    (("--osc", "cos", "--omega", "3"), "--osc"), (("--params", "rows.txt"), "--params"),
    (("--linspace", "p0=0:1:4"), "--linspace"), (("--ranges", "r.txt"), "--ranges"),
    (("--gpus", "2"), "--gpus 2"), (("--loopback", "2"), "--loopback"),
    (("--device", "cpu"), "--device cpu"),
]


@pytest.mark.parametrize("extra,named", CONFLICTS, ids=[n for _, n in CONFLICTS])
def test_the_curve_flags_refuse_another_modes_flags(extra, named):
    for tol in ("--curve-rtol", "--curve-atol"):
        args = [tol if v == "--curve-rtol" else v for v in CURVE]
        err = _refused(*args, *extra)
        assert WHO in err and named in err, err


def test_the_curve_refuses_ranks_bad_grids_bad_numbers_and_infinite_ends(tmp_path):
    err = _refused(*CURVE, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert "WORLD_SIZE = 2" in err and WHO in err
    assert "--expr" in _refused("--curve-rtol", "1e-9", "--a", "0", "--b", "1", "--points", "4")
    assert "need a grid" in _refused("--expr", "x", "--curve-rtol", "1e-9", "--a", "0", "--b", "1")
    assert "need a grid" in _refused("--expr", "x", "--curve-atol", "1e-9", "--points", "4")
    for ends in (("--a", "0", "--b", "inf"), ("--a", "-inf", "--b", "0")):
        assert "has an infinite end" in _refused("--expr", "x", "--curve-rtol", "1e-9", *ends,
                                                 "--points", "4")
    assert "they need --curve-rtol / --curve-atol" in _refused("--expr", "x", "--a", "0", "--b",
                                                               "1", "--points", "4")
    base = ("--expr", "x", "--curve-rtol", "1e-9", "--a", "0", "--b", "1")
    assert "--points 0 must be 1..2^20" in _refused(*base, "--points", "0")
    assert "--points must be a whole number" in _refused(*base, "--points", "2.5")
    assert "--curve-rtol must be a number" in _refused("--expr", "x", "--curve-rtol", "tiny",
                                                       "--a", "0", "--b", "1", "--points", "4")
    assert "rtol = 0 and atol = 0" in _refused("--expr", "x", "--curve-rtol", "0", "--a", "0",
                                               "--b", "1", "--points", "4")
    assert "x[1] = 1 after x[0] = 1" in _refused("--expr", "x", "--curve-rtol", "1e-9", "--a",
                                                 "1", "--b", "1", "--points", "4")
    assert "panels = 64 must be 1..max_intervals = 32" in _refused(
        *base, "--points", "4", "--panels", "64", "--max-intervals", "32")
    assert "rejected" in _refused("--expr", "x; y", "--curve-rtol", "1e-9", "--a", "0", "--b",
                                  "1", "--points", "4")
    grid = tmp_path / "grid.txt"
    grid.write_text("# a grid\n0\n0.5\n\n0.25\n1\n")
    at = ("--expr", "x", "--curve-rtol", "1e-9", "--at", str(grid))
    assert "x[2] = 0.25 after x[1] = 0.5" in _refused(*at)
    assert "--at FILE is the whole grid" in _refused(*at, "--a", "0")
    assert "--at FILE is the whole grid" in _refused(*at, "--points", "3")
    grid.write_text("0\n0.5 0.75\n")
    assert "line 2: expected `x`, got '0.5 0.75'" in _refused(*at)
    grid.write_text("0\nhalf\n")
    assert "line 2: expected `x`" in _refused(*at)
    grid.write_text("0\ninf\n")
    assert "x[1] = inf must be finite" in _refused(*at)
    grid.write_text("0\n")
    assert "1 points: the grid must hold" in _refused(*at)
    assert "cannot open" in _refused("--expr", "x", "--curve-rtol", "1e-9", "--at",
                                     str(tmp_path / "none.txt"))


SWEEP = ("--expr", "1.0/((x-p0)*(x-p0)+1e-6)", "--linspace", "p0=-0.5:0.7:4")


def test_ranges_refuse_a_shared_range_a_missing_row_tolerance_and_bad_files(tmp_path):
    ranges = tmp_path / "ranges.txt"
    ranges.write_text("-1 0\n-0.5 0.5\n# the third\n0 1\n1 0.25\n")
    tol = ("--row-rtol", "1e-8")
    for ends in (("--a", "-1"), ("--b", "1"), ("--a", "-1", "--b", "1")):
        err = _refused(*SWEEP, *tol, "--ranges", str(ranges), *ends)
        assert "--ranges gives every row its own a and b: --a / --b do not go with it" in err
    for other in ((), ("--rtol", "1e-8"), ("--n", "1e6"), ("--osc", "cos", "--omega", "2")):
        err = _refused(*SWEEP, "--ranges", str(ranges), *other)
        assert "--ranges" in err and "it needs --row-rtol R / --row-atol T" in err
    assert "--row-rtol / --row-atol" in _refused(*SWEEP, *tol, "--ranges", str(ranges), "--n",
                                                 "1e6")
    ranges.write_text("-1 0\n-0.5 0.5\n0 1\n")
    assert "3 ranges for 4 rows" in _refused(*SWEEP, *tol, "--ranges", str(ranges))
    ranges.write_text("-1 0\n-0.5 0.5\n0 1 2\n1 0\n")
    assert "line 3: expected `a b`, got '0 1 2'" in _refused(*SWEEP, *tol, "--ranges",
                                                             str(ranges))
    ranges.write_text("-1 0\n-0.5\n0 1\n1 0\n")
    assert "line 2: expected `a b`" in _refused(*SWEEP, *tol, "--ranges", str(ranges))
    ranges.write_text("-1 0\n-0.5 0.5\n0 inf\n1 0\n")
    assert "row 2: a = 0 and b = inf must be finite" in _refused(*SWEEP, *tol, "--ranges",
                                                                 str(ranges))
    assert "cannot open" in _refused(*SWEEP, *tol, "--ranges", str(tmp_path / "none.txt"))


def test_the_old_refusals_keep_their_words_and_the_usage_names_the_new_modes():
    err = _refused("--expr", "x", "--a", "0", "--b", "1", "--running", "--rtol", "1e-8")
    assert "--rtol / --atol choose the samples themselves: --running does not go" in err
    err = _refused(*SWEEP, "--a", "-1", "--b", "1", "--row-rtol", "1e-8", "--rule", "mid")
    assert "--row-rtol / --row-atol choose the samples themselves: --rule" in err
    err = _refused(*SWEEP, "--a", "-1", "--b", "1", "--max-total", "4096")
    assert "--max-total belongs to --row-rtol / --row-atol" in err
    err = _refused("--expr", "x", "--a", "0", "--b", "inf")
    assert "an infinite range needs --expr with --rtol / --atol or --row-rtol" in err
    p = _riemann("--help")
    assert p.returncode == 0
    for word in ("--ranges FILE", "--curve-rtol R", "--curve-atol T", "--points M", "--at FILE"):
        assert word in p.stdout, word
