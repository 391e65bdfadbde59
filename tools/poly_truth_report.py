#!/usr/bin/env python3
"""profiles/r17/poly_truth.md from the `POLYTRUTH` lines of the truth-referenced polynomial tests.

    python -m pytest tests/test_poly_truth_gpu.py -q -s > gpu.log      (on an MI355X)
    python -m pytest tests/test_poly_truth_cpu.py -q -s > cpu.log      (anywhere)
    python tools/poly_truth_report.py gpu.log cpu.log [parent.log] > body.md

Prints the tables only (the largest error / bound per kind and path, the CPU defects and the
case that detects each, the emulations' distance to the truth, every case with its measured
error, bound and ratio); the prose around them is written by hand. The third log, optional, is
test_degenerate_and_underflow of the same test file run against another build of the
extension: its `POLYTRUTH degenerate|underflow` lines (what ran, the value and the unscaled
sum each case returned) are listed with the cases that failed there.
"""
from __future__ import annotations

import collections
import re
import sys

ROW = re.compile(r"POLYTRUTH (\S+) (\S+) (\S+) err=(\S+) bound=(\S+) ratio=(\S+)")
RAN = re.compile(r"POLYTRUTH (degenerate|underflow) (\S+) ran=(\S+) value=(\S+) sum=(\S+) truth=(\S+)")
DEFECT = re.compile(r"POLYTRUTH defect (.*?): ratio (\S+) at (\S+)")
EMU = re.compile(r"POLYTRUTH cpu-emulation (\S+) worst ratio (\S+) at (\S+)")
FAILED = re.compile(r"FAILED \S+::(\S+\[.*\])")


def lines(path):
    with open(path) as f:
        # pytest -q -s glues its progress dots to the line a test prints
        return [ln[ln.index("POLYTRUTH"):].rstrip() for ln in f if "POLYTRUTH" in ln]


PREAMBLE = """# The polynomial kernels against an exact rational truth

Made by `tools/poly_truth_report.py` from the `POLYTRUTH` lines of
`tests/test_poly_truth_gpu.py` (MI355X) and `tests/test_poly_truth_cpu.py`. The truth is exact:
a, h, the rule offset and the coefficients are doubles, so every sample, every p(x_i) and every
sum is a rational that Python integers compute (`cuda_v_mpi_amd/utils/poly_truth.py`). Every
bound is derived there from the kernels' operations, in units of M(x) = sum |c_i| |x|^i; the
ratios below are measurements, written here and asserted nowhere (the tests assert
error <= bound only).

Launch values hold the even part E of a Taylor-pair sub-tile only: (E + k O) + (E - k O) = 2 E.
The odd part is held by the `point` rows (fp64 `point_values`); the fp32 paths have no point
kernel, so their O is not observable (test_poly_truth_cpu.py asserts both statements).

Before `poly_series_in_range` (kernels.hpp) a series request ran the Taylor-pair tiles at any
step. With a == b (h = 0) they return NaN (u_m = x_m * inf, then 0 * inf in the shift); with a
step that makes some c_i h^i a denormal or zero they lose that term's low bits or the term. The
parent table lists what that build returned; on this build the same requests run Horner per
sample.
"""


def main(argv):
    print(PREAMBLE)
    gpu, cpu = lines(argv[1]), lines(argv[2])
    rows = [m.groups() for m in map(ROW.match, gpu) if m]
    worst = collections.defaultdict(lambda: (-1.0, None))
    for kind, cid, path, err, bound, ratio in rows:
        worst[(kind, path)] = max(worst[(kind, path)], (float(ratio), cid))
    print("## Largest error / bound per kind and path\n\n| kind | path | ratio | case |\n|---|---|---|---|")
    for kind, path in sorted(worst):
        print(f"| {kind} | {path} | {worst[(kind, path)][0]:.4f} | `{worst[(kind, path)][1]}` |")
    print("\n## CPU: the emulated tiles against the truth, largest error / bound per path\n\n"
          "| path | ratio | case |\n|---|---|---|")
    for m in filter(None, map(EMU.match, cpu)):
        print(f"| {m.group(1)} | {m.group(2)} | `{m.group(3)}` |")
    print("\n## CPU defects (test_poly_truth_cpu.py): error / bound of the detecting case\n\n"
          "| defect | error / bound | at |\n|---|---|---|")
    for m in filter(None, map(DEFECT.match, cpu)):
        print(f"| {m.group(1)} | {m.group(2)} | `{m.group(3)}` |")
    if len(argv) > 3:
        with open(argv[3]) as f:
            text = f.read()
        failed = {m.group(1) for m in FAILED.finditer(text)}
        ran = [m.groups() for m in map(RAN.match, lines(argv[3])) if m]
        bad = [r for r in ran if any(r[1] in f for f in failed)]
        print(f"\n## Degenerate and underflow cases on the parent commit's build: {len(bad)} of "
              f"{len(ran)} fail\n\n| case | ran | value | unscaled sum | true sum |\n|---|---|---|---|---|")
        for kind, cid, path, value, total, truth in bad:
            print(f"| `{cid}` | {path} | {value} | {total} | {truth} |")
    ran = [m.groups() for m in map(RAN.match, gpu) if m]
    print(f"\n## The same cases on this build ({len(ran)} rows)\n\n"
          "| case | ran | value | unscaled sum | true sum |\n|---|---|---|---|---|")
    for kind, cid, path, value, total, truth in ran:
        print(f"| `{cid}` | {path} | {value} | {total} | {truth} |")
    print(f"\n## Every case ({len(rows)} rows)\n\n| kind | case | path | measured | bound | ratio |\n|---|---|---|---|---|---|")
    for kind, cid, path, err, bound, ratio in rows:
        print(f"| {kind} | `{cid}` | {path} | {err} | {bound} | {ratio} |")


if __name__ == "__main__":
    main(sys.argv)
