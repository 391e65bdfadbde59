#!/usr/bin/env python3
"""Choose the Korobov multipliers of the lattice rule's built-in table (lattice_generator in
csrc/runtime/expr_lattice.cpp). CPU only, numpy, seeded: the same a every time.

For each m the candidates are CANDIDATES draws congruent to 3 or 5 mod 8 below n = 2^m (such
an a has multiplicative order 2^(m-2), so z_j = a^j mod n are distinct for j < 16 once
m >= 6), from numpy's default generator seeded with (SEED, m). The winner minimises

    e^2(a) = -1 + (1/n) sum_i prod_{j<16} (1 + gamma_j 2 pi^2 B2({i z_j / n})),
    B2(t) = t^2 - t + 1/6, gamma_j = 1 / (j + 1)^2

(utils/lattice_rule.py: criterion). 64 candidates at m = 16 take about half a second, m = 24
about two minutes.

    python tools/lattice_search.py --m 10 24          # prints the table's rows
    python tools/lattice_search.py --m 12 12 --json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from cuda_v_mpi_amd.utils.lattice_rule import search  # noqa: E402

CANDIDATES = 64
SEED = 2024


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--m", type=int, nargs=2, default=[10, 24], metavar=("LO", "HI"),
                    help="the range of m to search (inclusive)")
    ap.add_argument("--json", action="store_true", help="one JSON record per m")
    a = ap.parse_args(argv)
    for m in range(a.m[0], a.m[1] + 1):
        t0 = time.perf_counter()
        best, e2 = search(m, CANDIDATES, SEED)
        secs = time.perf_counter() - t0
        if a.json:
            print(json.dumps({"m": m, "a": best, "e2": e2, "candidates": CANDIDATES,
                              "seed": SEED, "seconds": secs}), flush=True)
        else:
            print(f"  {best}u,  // m = {m}: e2 = {e2:.6e} ({secs:.1f} s)", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
