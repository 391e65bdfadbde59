#!/usr/bin/env python3
"""Read per-workgroup timelines of the persistent multi-step launch (needs no GPU).

Input: the JSON files `miint bench --timeline FILE` writes (RiemannPlan::timeline_batch; from
Python, Integrator.timeline(steps) holds the same arrays). Per workgroup w of the launch:

    stamps[w][0]            the device clock at kernel entry
    stamps[w][1 .. steps]   after step 1 .. steps' block sum (before the partial's store)
    stamps[w][steps + 1]    at exit
    shader_clock[w][0..1]   the workgroup's shader clock at entry and at exit
    hw[w][0..1]             raw XCC_ID and HW_ID register words (XCC id = hw[w][0] & 0xF)

The device clock is one constant-rate counter for the whole device (`clock_khz` ticks per
millisecond), so stamps of different workgroups and XCDs compare.

    python tools/timeline_report.py run.json [more.json.gz ...] [--ideal-us X] [--json]

Per file, a markdown section (or with --json one record per line) of

    span   max exit - min entry          ramp  max entry - min entry
    tail   max exit - min exit
    d[w][s], the step durations (differences of successive stamps; step 1's holds the
    kernel's set-up too): min / median / max over workgroups per step, and the skew of each
    step's stamp over workgroups (max - min);
    per XCC id: workgroups, median step duration (without step 1 when there are more steps:
    it holds the set-up), median shader clock (d memtime / d realtime x clock_khz);
    late entries: workgroups whose entry stamp is later than the earliest exit stamp, i.e. a
    second round of workgroups (the occupancy query the plan's residency check uses can say
    more than the device holds), and grid - late, the workgroups resident together;
    the critical path, i.e. the last workgroup to exit: its start delay (entry - min entry),
    its step durations summed, its exit segment (exit - last step stamp). The three add up to
    span exactly. And how much its step total exceeds the median workgroup's.

--ideal-us X attributes the gap span - X to four terms that add up to it by construction:

    start delay        the last workgroup's entry - min entry
    imbalance          its step total - the median workgroup's step total
    tail               its exit segment
    steps slower       the median workgroup's step total - X

A queue launch's record (`"work": "queue"`, RiemannConfig::work) is per physical workgroup
and per item instead: wg_stamps[w] = entry, exit; item_stamp[s][b] the device clock after
item (step s, virtual block b)'s block sum and item_owner[s][b] the workgroup that ran it. Its
report is the residency table: the share of CU-time with 0, 1, 2, ... workgroups resident
on a CU, a CU's idle time after its last exit, first to last exit, and the items each XCC ran
next to its shader clock. --residency adds the same table to a static record's report.

The launch measured is the timeline build's: stamps, their waits and their stores cost time
the plain launch does not spend. Read the shares, not the lengths (`device_us` over
`plain_device_us`, where the file has both, is the instrument's own cost).
"""
from __future__ import annotations

import argparse
import gzip
import json
import statistics
import sys

UNSET_STAMP = 0
UNSET_ID = 0xFFFFFFFF


class TimelineError(ValueError):
    pass


def validate(t: dict) -> None:
    """Raise TimelineError for a file no launch can have written: a wrong shape, a cell left
    at its sentinel, a workgroup whose stamps go backwards."""
    for k in ("steps", "grid", "clock_khz", "stamps", "shader_clock", "hw"):
        if k not in t:
            raise TimelineError(f"missing field {k!r}")
    steps, grid = int(t["steps"]), int(t["grid"])
    if steps < 1 or grid < 1 or int(t["clock_khz"]) <= 0:
        raise TimelineError("steps, grid and clock_khz must be positive")
    for name, cols in (("stamps", steps + 2), ("shader_clock", 2), ("hw", 2)):
        rows = t[name]
        if len(rows) != grid:
            raise TimelineError(f"{name}: {len(rows)} rows for a grid of {grid}")
        for w, row in enumerate(rows):
            if len(row) != cols:
                raise TimelineError(f"{name}: workgroup {w} has {len(row)} cells, not {cols}")
    for w in range(grid):
        if any(int(x) == UNSET_STAMP for x in t["stamps"][w]):
            raise TimelineError(f"stamps: workgroup {w} has an unwritten cell (sentinel 0)")
        if any(int(x) == UNSET_STAMP for x in t["shader_clock"][w]):
            raise TimelineError(f"shader_clock: workgroup {w} has an unwritten cell (sentinel 0)")
        if any(int(x) == UNSET_ID for x in t["hw"][w]):
            raise TimelineError(f"hw: workgroup {w} has an unwritten cell (sentinel all-ones)")
        row = t["stamps"][w]
        for i in range(1, len(row)):
            if int(row[i]) < int(row[i - 1]):
                raise TimelineError(f"stamps: workgroup {w} goes backwards at cell {i} "
                                    f"({row[i - 1]} -> {row[i]})")
        if int(t["shader_clock"][w][1]) < int(t["shader_clock"][w][0]):
            raise TimelineError(f"shader_clock: workgroup {w} goes backwards")


def is_queue(t: dict) -> bool:
    """The record of a queue launch (`"work": "queue"`; files from before the queue have no
    such field and are static records)."""
    return t.get("work") == "queue"


def validate_queue(t: dict) -> None:
    """The queue launch's record: per physical workgroup entry / exit, per item (step, virtual
    block) the stamp after its block sum and the workgroup that ran it."""
    for k in ("steps", "grid", "workgroups", "clock_khz", "wg_stamps", "item_stamp", "item_owner",
              "shader_clock", "hw"):
        if k not in t:
            raise TimelineError(f"missing field {k!r}")
    steps, grid, wgs = int(t["steps"]), int(t["grid"]), int(t["workgroups"])
    if steps < 1 or grid < 1 or wgs < 1 or int(t["clock_khz"]) <= 0:
        raise TimelineError("steps, grid, workgroups and clock_khz must be positive")
    for name, n, cols in (("wg_stamps", wgs, 2), ("shader_clock", wgs, 2), ("hw", wgs, 2),
                          ("item_stamp", steps, grid), ("item_owner", steps, grid)):
        rows = t[name]
        if len(rows) != n or any(len(r) != cols for r in rows):
            raise TimelineError(f"{name}: not {n} rows of {cols} cells")
    for w in range(wgs):
        if any(int(x) == UNSET_STAMP for x in t["wg_stamps"][w] + t["shader_clock"][w]):
            raise TimelineError(f"workgroup {w} has an unwritten stamp (sentinel 0)")
        if any(int(x) == UNSET_ID for x in t["hw"][w]):
            raise TimelineError(f"hw: workgroup {w} has an unwritten cell (sentinel all-ones)")
        if int(t["wg_stamps"][w][1]) < int(t["wg_stamps"][w][0]):
            raise TimelineError(f"wg_stamps: workgroup {w} exits before it enters")
    for s in range(steps):
        for b in range(grid):
            if int(t["item_stamp"][s][b]) == UNSET_STAMP:
                raise TimelineError(f"item ({s}, {b}) was never stamped (sentinel 0)")
            if not 0 <= int(t["item_owner"][s][b]) < wgs:
                raise TimelineError(f"item ({s}, {b}): owner {t['item_owner'][s][b]} is no "
                                    f"workgroup of the launch's {wgs}")


def load(path: str) -> dict:
    """A timeline file, plain or gzip-compressed (`.gz`: a 20-step G = 1 timeline is 0.7 MB
    of digits, 10 x less compressed)."""
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        t = json.load(f)
    if not isinstance(t, dict):
        raise TimelineError("not a JSON object")
    if is_queue(t):
        validate_queue(t)
    else:
        validate(t)
    return t


def residency(t: dict) -> dict:
    """Either record form, by CU (the XCC id and the SE / SH / CU fields of HW_ID, bits 8-15):
    the share of CU-time (CUs x the span from the first entry to the last exit) spent with
    0, 1, 2, ... workgroups resident, a CU's idle time between its last exit and the launch's
    end, the first-to-last exit, and the items (step, block) each XCC ran with its shader clock."""
    khz = int(t["clock_khz"])
    queue = is_queue(t)
    rows = t["wg_stamps"] if queue else t["stamps"]
    entry = [int(r[0]) for r in rows]
    exit_ = [int(r[-1]) for r in rows]
    xcc_of = [int(r[0]) & 0xF for r in t["hw"]]
    cu_of = [(xcc_of[w], (int(t["hw"][w][1]) >> 8) & 0xFF) for w in range(len(rows))]
    t0, t1 = min(entry), max(exit_)
    span = t1 - t0
    by_cu: dict = {}
    for w, cu in enumerate(cu_of):
        by_cu.setdefault(cu, []).append(w)
    time_at: dict = {}
    end_idle = []
    for ws in by_cu.values():
        ev = sorted([(entry[w], 1) for w in ws] + [(exit_[w], -1) for w in ws])
        now, n = t0, 0
        for at, dn in ev:
            time_at[n] = time_at.get(n, 0) + (at - now)
            now, n = at, n + dn
        time_at[0] = time_at.get(0, 0) + (t1 - now)
        end_idle.append(t1 - max(exit_[w] for w in ws))
    total = span * len(by_cu)
    shares = {n: v / total for n, v in sorted(time_at.items())} if total else {}
    if queue:
        items = [0] * len(rows)
        for row in t["item_owner"]:
            for o in row:
                items[int(o)] += 1
    else:
        items = [int(t["steps"])] * len(rows)
    per_xcc = []
    for x in sorted(set(xcc_of)):
        ws = [w for w in range(len(rows)) if xcc_of[w] == x]
        clocks = [(int(t["shader_clock"][w][1]) - int(t["shader_clock"][w][0])) /
                  (exit_[w] - entry[w]) * khz for w in ws if exit_[w] > entry[w] and items[w]]
        per_xcc.append(dict(xcc=x, workgroups=len(ws), items=sum(items[w] for w in ws),
                            median_shader_khz=statistics.median(clocks) if clocks else None))
    us = lambda ticks: ticks * 1e3 / khz  # noqa: E731
    return dict(cus=len(by_cu), span_us=us(span), first_to_last_exit_us=us(t1 - min(exit_)),
                first_to_last_working_exit_us=us(t1 - min(exit_[w] for w in range(len(rows))
                                                       if items[w])),
                resident_share=shares,
                share_le2=shares.get(1, 0.0) + shares.get(2, 0.0), share_1=shares.get(1, 0.0),
                share_0=shares.get(0, 0.0),
                end_idle_mean_us=us(statistics.mean(end_idle)), end_idle_max_us=us(max(end_idle)),
                end_idle_share=statistics.mean(end_idle) / span if span else 0.0,
                idle_workgroups=sum(1 for n in items if n == 0), per_xcc=per_xcc)


def residency_markdown(r: dict) -> str:
    o = [f"{r['cus']} CUs; span {r['span_us']:.1f} us; first to last exit "
         f"{r['first_to_last_exit_us']:.1f} us (among workgroups that ran an item "
         f"{r['first_to_last_working_exit_us']:.1f} us; {r['idle_workgroups']} ran none).",
         f"Two or fewer workgroups resident on a CU {100 * r['share_le2']:.1f} % of CU-time, one "
         f"{100 * r['share_1']:.1f} %, none {100 * r['share_0']:.1f} % (a CU idle after its last "
         f"exit: mean {r['end_idle_mean_us']:.1f} us = {100 * r['end_idle_share']:.2f} %, max "
         f"{r['end_idle_max_us']:.1f} us).", "",
         "| resident workgroups | " + " | ".join(str(n) for n in r["resident_share"]) + " |",
         "|---|" + "---|" * len(r["resident_share"]),
         "| share of CU-time % | " +
         " | ".join(f"{100 * v:.1f}" for v in r["resident_share"].values()) + " |", "",
         "| XCC | workgroups | items | median shader clock MHz |", "|---|---|---|---|"]
    for p in r["per_xcc"]:
        clk = "-" if p["median_shader_khz"] is None else f"{p['median_shader_khz'] / 1e3:.0f}"
        o.append(f"| {p['xcc']} | {p['workgroups']} | {p['items']} | {clk} |")
    return "\n".join(o) + "\n"


def analyse_queue(t: dict) -> dict:
    """The queue record's figures: the residency table, and per workgroup the time from one of
    its items' stamps to the next (an item's length as its workgroup saw it)."""
    validate_queue(t)
    khz = int(t["clock_khz"])
    mine: dict = {}
    for s, row in enumerate(t["item_owner"]):
        for b, o in enumerate(row):
            mine.setdefault(int(o), []).append(int(t["item_stamp"][s][b]))
    gaps = []
    for w, st in mine.items():
        st = [int(t["wg_stamps"][w][0])] + st  # claims only grow: already in order
        gaps += [b - a for a, b in zip(st[1:], st[2:])]  # without the first (set-up, ramp)
    us = lambda ticks: ticks * 1e3 / khz  # noqa: E731
    r = dict(work="queue", steps=int(t["steps"]), grid=int(t["grid"]),
             workgroups=int(t["workgroups"]), block=t.get("block"), clock_khz=khz,
             integrand=t.get("integrand"), n=t.get("n"), dtype=t.get("dtype"), div=t.get("div"),
             device_us=t.get("device_us"), plain_device_us=t.get("plain_device_us"),
             item_median_us=us(statistics.median(gaps)) if gaps else None,
             item_max_us=us(max(gaps)) if gaps else None,
             items_per_workgroup_min=min((len(v) for v in mine.values()), default=0),
             items_per_workgroup_max=max((len(v) for v in mine.values()), default=0),
             residency=residency(t))
    if r["device_us"] and r["plain_device_us"]:
        r["instrument_ratio"] = r["device_us"] / r["plain_device_us"]
    return r


def queue_markdown(name: str, r: dict) -> str:
    o = [f"### {name}", "",
         f"{r.get('integrand') or 'timeline'}, n = {r.get('n')}; queue launch: {r['steps']} steps "
         f"x virtual grid {r['grid']} = {r['steps'] * r['grid']} items pulled by "
         f"{r['workgroups']} workgroups of {r['block']} threads."]
    if r.get("device_us"):
        line = f"Event span of the instrumented batch {r['device_us']:.1f} us"
        if r.get("instrument_ratio"):
            line += (f", of the plain batch {r['plain_device_us']:.1f} us: instrument cost "
                     f"x{r['instrument_ratio']:.3f}")
        o.append(line + ".")
    if r["item_median_us"] is not None:
        o.append(f"A workgroup's item (stamp to stamp): median {r['item_median_us']:.2f} us, max "
                 f"{r['item_max_us']:.2f} us; {r['items_per_workgroup_min']} to "
                 f"{r['items_per_workgroup_max']} items per workgroup that ran any.")
    return "\n".join(o) + "\n\n" + residency_markdown(r["residency"])


def analyse(t: dict, ideal_us: float | None = None) -> dict:
    """Every figure of the report, in ticks of the device clock (`*_ticks`, exact) and in
    microseconds (`*_us`)."""
    validate(t)
    steps, grid, khz = int(t["steps"]), int(t["grid"]), int(t["clock_khz"])
    st = [[int(x) for x in row] for row in t["stamps"]]
    us = lambda ticks: ticks * 1e3 / khz  # noqa: E731
    entry = [r[0] for r in st]
    exit_ = [r[-1] for r in st]
    t0 = min(entry)
    span, ramp, tail = max(exit_) - t0, max(entry) - t0, max(exit_) - min(exit_)
    d = [[r[s + 1] - r[s] for s in range(steps)] for r in st]
    step_total = [r[steps] - r[0] for r in st]
    per_step = []
    for s in range(steps):
        col = [d[w][s] for w in range(grid)]
        at = [st[w][s + 1] for w in range(grid)]
        per_step.append(dict(step=s + 1, min_ticks=min(col), median_ticks=statistics.median(col),
                             max_ticks=max(col), skew_ticks=max(at) - min(at)))
    xcc_of = [int(r[0]) & 0xF for r in t["hw"]]
    per_xcc = []
    for x in sorted(set(xcc_of)):
        ws = [w for w in range(grid) if xcc_of[w] == x]
        clocks = []
        for w in ws:
            dr = exit_[w] - entry[w]
            if dr > 0:
                dm = int(t["shader_clock"][w][1]) - int(t["shader_clock"][w][0])
                clocks.append(dm / dr * khz)
        # step 1 holds the kernel's set-up (and, in a launch whose workgroups take turns,
        # the wait for them): with more than one step it is left out of the XCC's median
        per_xcc.append(dict(xcc=x, workgroups=len(ws),
                            median_step_ticks=statistics.median(
                                d[w][s] for w in ws for s in range(1 if steps > 1 else 0, steps)),
                            median_shader_khz=statistics.median(clocks) if clocks else None))
    last = max(range(grid), key=lambda w: (exit_[w], -w))  # the lowest index among the last
    start_delay = entry[last] - t0
    exit_seg = exit_[last] - st[last][steps]
    med_total = statistics.median(step_total)
    # a workgroup that enters after another has left was not resident with it: a second round
    late = sum(1 for w in range(grid) if entry[w] > min(exit_))
    r = dict(steps=steps, grid=grid, block=t.get("block"), clock_khz=khz,
             integrand=t.get("integrand"), n=t.get("n"), slice_of=t.get("slice_of"),
             dtype=t.get("dtype"), div=t.get("div"),
             device_us=t.get("device_us"), plain_device_us=t.get("plain_device_us"),
             span_ticks=span, ramp_ticks=ramp, tail_ticks=tail,
             span_us=us(span), ramp_us=us(ramp), tail_us=us(tail),
             late_entries=late, resident_at_first_exit=grid - late,
             per_step=per_step, per_xcc=per_xcc,
             last_workgroup=last, last_xcc=xcc_of[last],
             start_delay_ticks=start_delay, last_steps_ticks=step_total[last],
             exit_segment_ticks=exit_seg,
             median_steps_ticks=med_total, excess_ticks=step_total[last] - med_total,
             start_delay_us=us(start_delay), last_steps_us=us(step_total[last]),
             exit_segment_us=us(exit_seg), median_steps_us=us(med_total),
             excess_us=us(step_total[last] - med_total))
    if r["device_us"] and r["plain_device_us"]:
        r["instrument_ratio"] = r["device_us"] / r["plain_device_us"]
    for p in per_step:
        for k in ("min", "median", "max", "skew"):
            p[k + "_us"] = us(p[k + "_ticks"])
    for p in per_xcc:
        p["median_step_us"] = us(p["median_step_ticks"])
    if ideal_us is not None:
        ideal_ticks = ideal_us * khz / 1e3
        r.update(ideal_us=ideal_us, gap_ticks=span - ideal_ticks,
                 gap_start_delay_ticks=start_delay,
                 gap_imbalance_ticks=step_total[last] - med_total,
                 gap_tail_ticks=exit_seg,
                 gap_steps_slower_ticks=med_total - ideal_ticks)
        for k in ("gap", "gap_start_delay", "gap_imbalance", "gap_tail", "gap_steps_slower"):
            r[k + "_us"] = us(r[k + "_ticks"])
    return r


def markdown(name: str, r: dict) -> str:
    o = [f"### {name}", ""]
    what = f"{r['integrand']}, n = {r['n']}" if r.get("integrand") else "timeline"
    if r.get("slice_of"):
        what += f", share {r['slice_of'][0]} of {r['slice_of'][1]}"
    if r.get("dtype"):
        what += f", {r['dtype']}, div {r['div']}"
    o.append(f"{what}; {r['steps']} step{'s' if r['steps'] > 1 else ''}, grid {r['grid']} x {r['block']} threads, device clock "
             f"{r['clock_khz'] / 1e3:g} MHz.")
    if r.get("device_us"):
        line = f"Event span of the instrumented batch {r['device_us']:.1f} us"
        if r.get("instrument_ratio"):
            line += (f", of the plain batch {r['plain_device_us']:.1f} us: instrument cost "
                     f"x{r['instrument_ratio']:.3f}")
        o.append(line + ".")
    if r["late_entries"]:
        o += ["", f"**Not one round of workgroups:** {r['late_entries']} of {r['grid']} workgroups "
              f"enter after the first exit; {r['resident_at_first_exit']} were resident together. "
              "ramp, tail and the gap's terms below describe the rounds, not one resident launch."]
    o += ["", "| span us | ramp us | tail us |", "|---|---|---|",
          f"| {r['span_us']:.2f} | {r['ramp_us']:.2f} | {r['tail_us']:.2f} |", "",
          "| step | min us | median us | max us | skew at the block sum us |", "|---|---|---|---|---|"]
    for p in r["per_step"]:
        o.append(f"| {p['step']} | {p['min_us']:.2f} | {p['median_us']:.2f} | {p['max_us']:.2f} "
                 f"| {p['skew_us']:.2f} |")
    steady = "median step us (steps 2..)" if r["steps"] > 1 else "median step us"
    o += ["", f"| XCC | workgroups | {steady} | median shader clock MHz |", "|---|---|---|---|"]
    for p in r["per_xcc"]:
        clk = "-" if p["median_shader_khz"] is None else f"{p['median_shader_khz'] / 1e3:.0f}"
        o.append(f"| {p['xcc']} | {p['workgroups']} | {p['median_step_us']:.3f} | {clk} |")
    o += ["", f"Critical path: workgroup {r['last_workgroup']} (XCC {r['last_xcc']}) exits last: "
          f"start delay {r['start_delay_us']:.2f} + steps {r['last_steps_us']:.2f} + exit segment "
          f"{r['exit_segment_us']:.2f} = span {r['span_us']:.2f} us. Its steps take "
          f"{r['excess_us']:+.2f} us against the median workgroup's {r['median_steps_us']:.2f} us."]
    if "gap_us" in r:
        o += ["", f"Gap to the ideal {r['ideal_us']:.2f} us: {r['gap_us']:.2f} us = start delay "
              f"{r['gap_start_delay_us']:.2f} + imbalance {r['gap_imbalance_us']:.2f} + tail "
              f"{r['gap_tail_us']:.2f} + steps slower than ideal {r['gap_steps_slower_us']:.2f}."]
    return "\n".join(o) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+", help="timeline JSON files (miint bench --timeline)")
    ap.add_argument("--ideal-us", type=float, default=None,
                    help="the launch's ideal length: attribute span - ideal to four terms")
    ap.add_argument("--json", action="store_true", help="one JSON record per file, no markdown")
    ap.add_argument("--residency", action="store_true",
                    help="a static record: also the CU-time by resident workgroups, the end "
                         "idle and the items per XCC (a queue record's report always has them)")
    a = ap.parse_args(argv)
    for path in a.files:
        try:
            t = load(path)
            queue = is_queue(t)
            r = analyse_queue(t) if queue else analyse(t, a.ideal_us)
            if a.residency and not queue:
                r["residency"] = residency(t)
        except (TimelineError, OSError, EOFError, json.JSONDecodeError) as e:
            print(f"timeline_report: {path}: {e}", file=sys.stderr)
            return 1
        if a.json:
            print(json.dumps(dict(r, file=path)))
        elif queue:
            print(queue_markdown(path, r))
        else:
            print(markdown(path, r))
            if a.residency:
                print(residency_markdown(r["residency"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
