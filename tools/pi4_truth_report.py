#!/usr/bin/env python3
"""profiles/r13/pi4_truth.md from the `PI4TRUTH` lines of the truth-referenced pi4 tests.

    python -m pytest tests/test_pi4_truth_gpu.py -q -s > gpu.log      (on an MI355X)
    python -m pytest tests/test_pi4_truth_cpu.py -q -s > cpu.log      (anywhere)
    python tools/pi4_truth_report.py gpu.log cpu.log [parent_far.log] > body.md

Prints the tables only (every case with its path, measured error, bound and ratio; the largest
ratio per path; the CPU defects and the cases that detect them; the definitions' distance to
the truth per path); the prose around them is written by hand. The third log, optional, is a
listing of the far / degenerate cases on another build (`FAR <case> ... ok|FAIL` lines).
"""
from __future__ import annotations

import collections
import re
import sys

ROW = re.compile(r"PI4TRUTH (\S+) (\S+) (\S+) err=(\S+) bound=(\S+) ratio=(\S+)")
DEFN = re.compile(r"PI4TRUTH defn (\S+) (\S+) err=(\S+) bound=(\S+)")
DEFECT = re.compile(r"PI4TRUTH defect (.*?): detected by (\d+) of (\d+) cases, largest err/bound (\S+) at (\S+)")


def lines(path):
    with open(path) as f:
        # pytest -q -s glues its progress dots to the line a test prints
        return [ln[ln.index("PI4TRUTH"):].rstrip() for ln in f if "PI4TRUTH" in ln]


def main(argv):
    gpu, cpu = lines(argv[1]), lines(argv[2])
    rows = [m.groups() for m in map(ROW.match, gpu) if m]
    worst = collections.defaultdict(lambda: (-1.0, None))
    for kind, cid, path, err, bound, ratio in rows:
        if kind == "tile-model":
            continue
        key = path.replace("-narrow", "").replace("-wide", "")
        worst[key] = max(worst[key], (float(ratio), f"{kind} `{cid}`"))
    print("## Largest error / bound per path\n\n| path | ratio | case |\n|---|---|---|")
    for path in sorted(worst):
        print(f"| {path} | {worst[path][0]:.4f} | {worst[path][1]} |")
    print("\n## CPU defects (test_pi4_truth_cpu.py)\n\n| defect | detected by | largest err / bound | at |\n|---|---|---|---|")
    for m in filter(None, map(DEFECT.match, cpu)):
        name, hit, tried, ratio, cid = m.groups()
        print(f"| {name} | {hit} of {tried} cases | {ratio} | `{cid}` |")
    dd = collections.defaultdict(lambda: (-1.0, 0.0, None))
    for m in filter(None, map(DEFN.match, cpu)):
        cid, path, err, bound = m.groups()
        r = float(err) / float(bound) if float(bound) > 0 else 0.0
        dd[path] = max(dd[path], (float(err), r, cid))
    print("\n## Definition against truth, largest relative distance per path (CPU)\n\n"
          "| path | measured | ratio to its bound | case |\n|---|---|---|---|")
    for path in sorted(dd):
        print(f"| {path} | {dd[path][0]:.3e} | {dd[path][1]:.3f} | `{dd[path][2]}` |")
    if len(argv) > 3:
        print("\n## The far and degenerate cases on the parent commit's build\n\n```")
        with open(argv[3]) as f:
            for ln in f:
                if ln.startswith("FAR ") or ln.startswith("failing"):
                    print(ln.rstrip())
        print("```")
    print(f"\n## Every case ({len(rows)} rows)\n\n| kind | case | path | measured | bound | ratio |\n|---|---|---|---|---|---|")
    for kind, cid, path, err, bound, ratio in rows:
        print(f"| {kind} | `{cid}` | {path} | {err} | {bound} | {ratio} |")


if __name__ == "__main__":
    main(sys.argv)
