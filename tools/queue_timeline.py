#!/usr/bin/env python3
"""One timeline of the static and of the queue form of the multi-step launch, same process,
same shape (needs a GPU): where a launch's time goes under each schedule.

    python tools/queue_timeline.py [--n 1e9] [--steps 48] [--per-cu 7,6] [--out DIR]

Per form: an untimed warm-up, one diagnostic batch (the plain launch between two events: the
denominator of the instrument's cost), one timeline batch; the record goes to
DIR/<form>.json.gz (the files tools/timeline_report.py reads) and the residency report to
stdout as markdown. --per-cu lists the queue's physical workgroups per CU to try.
"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def record(it, t: dict, plain_us: float) -> dict:
    r = dict(integrand=it.spec.name, n=it.n, slice_of=None, dtype=it.dtype, div=it.div,
             steps=t["steps"], grid=t["grid"], block=t["block"], clock_khz=t["clock_khz"],
             device_us=t["device_us"], plain_device_us=plain_us, values=list(t["values"]),
             work=t["work"], shader_clock=t["shader_clock"].tolist(), hw=t["hw"].tolist())
    if t["work"] == "queue":
        r.update(workgroups=t["workgroups"], wg_stamps=t["wg_stamps"].tolist(),
                 item_stamp=t["item_stamp"].tolist(), item_owner=t["item_owner"].tolist())
    else:
        r["stamps"] = t["stamps"].tolist()
    return r


def main(argv=None) -> int:
    import timeline_report as tr
    from cuda_v_mpi_amd import Integrator

    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--per-cu", default="0", help="queue workgroups per CU, comma-separated")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    forms = [("static", dict(work="static"))]
    for p in a.per_cu.split(","):
        forms.append((f"queue_{p}" if int(p) else "queue", dict(work="queue",
                                                               queue_wg_per_cu=int(p))))
    values = None
    for name, kw in forms:
        it = Integrator("pi4", n=int(a.n), slots=a.steps, **kw)
        it.run_steps(20 * a.steps, pipeline=False, graphs=False)  # clocks settle
        plain = it.plan.diagnose_batch(a.steps)["device_us"]
        t = it.timeline(a.steps)
        bits = [float(v).hex() for v in t["values"]]
        assert values is None or bits == values, "the forms disagree"
        values = bits
        r = record(it, t, plain)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with gzip.open(os.path.join(a.out, name + ".json.gz"), "wt") as f:
                json.dump(r, f)
        print(f"## {name}: work = {it.plan.work}, {it.plan.queue_workgroups or it.plan.grid} "
              f"physical workgroups\n")
        print(f"Plain batch {plain:.1f} us, instrumented {t['device_us']:.1f} us "
              f"(x{t['device_us'] / plain:.4f}).\n")
        if t["work"] == "queue":
            print(tr.queue_markdown(name, tr.analyse_queue(r)))
        else:
            print(tr.residency_markdown(tr.residency(r)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
