#!/usr/bin/env python3
"""profiles/r18/table_truth.md from the `TABLETRUTH` lines of the truth-referenced table tests.

    python -m pytest tests/test_table_truth_gpu.py -q -s > gpu.log      (on an MI355X)
    python -m pytest tests/test_table_truth_cpu.py -q -s > cpu.log      (anywhere)
    python tools/table_truth_report.py gpu.log cpu.log > profiles/r18/table_truth.md

The largest error / bound per kind and path, the CPU emulations' distance to the truth, the CPU
defects and the case that detects each, the host engine's rows, and every GPU case with its
measured error, bound and ratio.
"""
from __future__ import annotations

import collections
import re
import sys

ROW = re.compile(r"TABLETRUTH (\S+) (\S+) (\S+) err=(\S+) bound=(\S+) ratio=(\S+)")
DEFECT = re.compile(r"TABLETRUTH defect (.*?): ratio (\S+) at (\S+)")
EMU = re.compile(r"TABLETRUTH cpu-emulation (\S+) worst ratio (\S+) at (\S+)")

PREAMBLE = """# The velocity-table kernels against an exact rational truth

Made by `tools/table_truth_report.py` from the `TABLETRUTH` lines of
`tests/test_table_truth_gpu.py` (MI355X) and `tests/test_table_truth_cpu.py`. The truth is exact:
a, h, the rule offset and the table's entries are doubles, so every sample, every interpolated
value and every sum is a rational that Python integers compute
(`cuda_v_mpi_amd/utils/table_truth.py`; sums in closed form, segment by segment). Every bound is
derived there from the kernels' operations, in units of M(x) = |v_s| + |d_s||x - s| and, for a
tile's own operations, M + 64|h| max|d|; the ratios below are measurements, written here and
asserted nowhere (the tests assert error <= bound only).

Two defects were found. The fp32 per-sample form (`TableF32::pointf`) formed its slope from
fp32-rounded entries, which loses the extrapolation on an end segment whose entries round to one
float: by its exactly rounded emulation the parent's build misses the bound of the `far-3e9` and
`far-neg-2p60` launches on both fp32 requests by 1.5e4 to 8.8e5 bounds (the `defect` rows below);
the slope is now subtracted in fp64 and converted once. `Table::series_point`, the point
kernel's copy of the segment tile, took the kink branch for a reversed tile across a knot
(`rev-mix`, fp64 series points: -43.995 returned where 1.4224 is true, on the device); it now
branches as `tile_acc` does. Launch values were not affected by the second.
"""


def lines(path):
    with open(path) as f:
        # pytest -q -s glues its progress dots to the line a test prints
        return [ln[ln.index("TABLETRUTH"):].rstrip() for ln in f if "TABLETRUTH" in ln]


def main(argv):
    print(PREAMBLE)
    gpu, cpu = lines(argv[1]), lines(argv[2])
    rows = [m.groups() for m in map(ROW.match, gpu) if m]
    worst = collections.defaultdict(lambda: (-1.0, None))
    for kind, cid, path, err, bound, ratio in rows:
        worst[(kind, path)] = max(worst[(kind, path)], (float(ratio), cid))
    print("## Largest error / bound per kind and path (MI355X)\n\n| kind | path | ratio | case |\n|---|---|---|---|")
    for kind, path in sorted(worst):
        print(f"| {kind} | {path} | {worst[(kind, path)][0]:.4f} | `{worst[(kind, path)][1]}` |")
    per_path = collections.defaultdict(lambda: (-1.0, None))
    for kind, cid, path, err, bound, ratio in rows:
        per_path[path] = max(per_path[path], (float(ratio), f"{kind} {cid}"))
    print("\n## Largest error / bound per path (MI355X)\n\n| path | ratio | case |\n|---|---|---|")
    for path in sorted(per_path):
        print(f"| {path} | {per_path[path][0]:.4f} | `{per_path[path][1]}` |")
    print("\n## CPU: the emulated tiles against the truth, largest error / bound per path\n\n"
          "| path | ratio | case |\n|---|---|---|")
    for m in filter(None, map(EMU.match, cpu)):
        print(f"| {m.group(1)} | {m.group(2)} | `{m.group(3)}` |")
    print("\n## CPU defects (test_table_truth_cpu.py): error / bound of the detecting case\n\n"
          "| defect | error / bound | at |\n|---|---|---|")
    for m in filter(None, map(DEFECT.match, cpu)):
        print(f"| {m.group(1)} | {m.group(2)} | `{m.group(3)}` |")
    host = [m.groups() for m in map(ROW.match, cpu) if m]
    print(f"\n## The host engine's table path ({len(host)} rows)\n\n| case | measured | bound | ratio |\n|---|---|---|---|")
    for kind, cid, path, err, bound, ratio in host:
        print(f"| `{cid}` | {err} | {bound} | {ratio} |")
    print(f"\n## Every GPU case ({len(rows)} rows)\n\n| kind | case | path | measured | bound | ratio |\n|---|---|---|---|---|---|")
    for kind, cid, path, err, bound, ratio in rows:
        print(f"| {kind} | `{cid}` | {path} | {err} | {bound} | {ratio} |")


if __name__ == "__main__":
    main(sys.argv)
