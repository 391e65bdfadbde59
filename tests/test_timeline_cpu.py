"""The timeline instrument without a GPU: tools/timeline_report.py on synthetic stamps whose
figures follow by hand from their construction, its refusal of files no launch can have
written, the timeline kernels' resources next to their plain twins' (compiled device-only to
gfx950 assembly), and the CLI's help."""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import isa_guard  # noqa: E402
import timeline_report  # noqa: E402

# The construction (ticks of a 100 MHz device clock: 100 ticks = 1 us):
#   16 workgroups, 4 steps, XCC id = w % 4 (with other bits of the register word set);
#   entry[w] = T0 + 10 w                       a linear start ramp: ramp = 150
#   a step takes 1000 ticks, on XCC 2 10 % more (1100)
#   workgroup 5 (XCC 1) is a straggler: its step 3 takes 1700
#   every exit segment (last block sum -> exit) takes 20
#   the shader clock runs 24 ticks per device tick (2400 MHz), on XCC 2 21 (2100 MHz)
T0, GRID, STEPS, KHZ = 5_000_000, 16, 4, 100_000


def synthetic():
    stamps, clk, hw = [], [], []
    for w in range(GRID):
        xcc = w % 4
        row = [T0 + 10 * w]
        for s in range(STEPS):
            d = 1100 if xcc == 2 else 1000
            if w == 5 and s == 2:
                d = 1700
            row.append(row[-1] + d)
        row.append(row[-1] + 20)
        stamps.append(row)
        rate = 21 if xcc == 2 else 24
        clk.append([7_000 + w, 7_000 + w + rate * (row[-1] - row[0])])
        hw.append([0x5A0 | xcc, 0x1000 + w])
    return dict(integrand="pi4", n=10**9, slice_of=[0, 8], dtype="fp64", div="series_exact",
                steps=STEPS, grid=GRID, block=256, clock_khz=KHZ, device_us=60.0,
                plain_device_us=50.0, values=[3.14] * STEPS, stamps=stamps, shader_clock=clk,
                hw=hw)


def test_span_ramp_tail():
    r = timeline_report.analyse(synthetic())
    # the straggler exits last: T0 + 50 + (3 x 1000 + 1700) + 20; first exit: workgroup 0
    assert r["span_ticks"] == 4770 and r["ramp_ticks"] == 150
    assert r["tail_ticks"] == 4770 - 4020
    assert r["span_us"] == pytest.approx(47.70, abs=1e-9)
    assert r["instrument_ratio"] == pytest.approx(1.2)


def test_step_durations_and_skew():
    r = timeline_report.analyse(synthetic())
    s1, s3 = r["per_step"][0], r["per_step"][2]
    assert (s1["min_ticks"], s1["median_ticks"], s1["max_ticks"]) == (1000, 1000, 1100)
    assert (s3["min_ticks"], s3["median_ticks"], s3["max_ticks"]) == (1000, 1000, 1700)
    # step 1's stamp: earliest workgroup 0 (1000), latest workgroup 14 on XCC 2 (140 + 1100)
    assert s1["skew_ticks"] == 240
    # step 3's: latest the straggler (50 + 3700), earliest workgroup 0 (3000)
    assert s3["skew_ticks"] == 750


def test_per_xcc_medians():
    r = timeline_report.analyse(synthetic())
    x = {p["xcc"]: p for p in r["per_xcc"]}
    assert sorted(x) == [0, 1, 2, 3] and all(p["workgroups"] == 4 for p in x.values())
    assert [x[i]["median_step_ticks"] for i in range(4)] == [1000, 1000, 1100, 1000]
    assert [x[i]["median_shader_khz"] for i in range(4)] == [24 * KHZ, 24 * KHZ, 21 * KHZ,
                                                             24 * KHZ]


def test_late_entries_are_counted():
    """A workgroup that enters after another has left is a second round: counted and said."""
    t = synthetic()
    assert timeline_report.analyse(t)["late_entries"] == 0
    first_exit = min(r[-1] for r in t["stamps"])
    for w in (9, 12):  # two workgroups start only after the first exit
        shift = first_exit + 5 - t["stamps"][w][0]
        t["stamps"][w] = [x + shift for x in t["stamps"][w]]
    r = timeline_report.analyse(t)
    assert r["late_entries"] == 2 and r["resident_at_first_exit"] == GRID - 2
    assert "2 of 16 workgroups enter after the first exit" in timeline_report.markdown("x", r)
    assert "enter after the first exit" not in timeline_report.markdown(
        "x", timeline_report.analyse(synthetic()))


def test_per_xcc_median_leaves_step_one_out():
    t = synthetic()
    for row in t["stamps"]:  # step 1 takes 5000 more everywhere (set-up): not an XCC's rate
        row[1:] = [x + 5000 for x in row[1:]]
    r = timeline_report.analyse(t)
    assert [p["median_step_ticks"] for p in r["per_xcc"]] == [1000, 1000, 1100, 1000]
    assert "median step us (steps 2..)" in timeline_report.markdown("x", r)
    one = dict(t, steps=1, stamps=[[row[0], row[1], row[1] + 20] for row in t["stamps"]])
    r1 = timeline_report.analyse(one)
    assert [p["median_step_ticks"] for p in r1["per_xcc"]] == [6000, 6000, 6100, 6000]
    assert "; 1 step, grid" in timeline_report.markdown("x", r1)


def test_critical_path_adds_up_to_span():
    r = timeline_report.analyse(synthetic())
    assert r["last_workgroup"] == 5 and r["last_xcc"] == 1
    assert (r["start_delay_ticks"], r["last_steps_ticks"], r["exit_segment_ticks"]) == (50, 4700, 20)
    assert r["start_delay_ticks"] + r["last_steps_ticks"] + r["exit_segment_ticks"] == r["span_ticks"]
    # step totals: 11 workgroups at 4000, 4 at 4400, the straggler at 4700: median 4000
    assert r["median_steps_ticks"] == 4000 and r["excess_ticks"] == 700


def test_ideal_gap_terms_sum_to_the_gap():
    r = timeline_report.analyse(synthetic(), ideal_us=39.0)  # 3900 ticks
    assert r["gap_ticks"] == pytest.approx(870, abs=1e-6)
    terms = [r["gap_start_delay_ticks"], r["gap_imbalance_ticks"], r["gap_tail_ticks"],
             r["gap_steps_slower_ticks"]]
    assert terms[:3] == [50, 700, 20] and terms[3] == pytest.approx(100, abs=1e-6)
    assert sum(terms) == pytest.approx(r["gap_ticks"], abs=1e-6)
    assert r["gap_us"] == pytest.approx(8.70, abs=1e-9)


def test_command_line_markdown_and_json(tmp_path):
    f = tmp_path / "synthetic.json"
    f.write_text(json.dumps(synthetic()))
    tool = os.path.join(REPO, "tools", "timeline_report.py")
    p = subprocess.run([sys.executable, tool, str(f), "--ideal-us", "39", "--json"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout)
    assert rec["span_ticks"] == 4770 and rec["file"] == str(f) and rec["gap_imbalance_ticks"] == 700
    p = subprocess.run([sys.executable, tool, str(f), "--ideal-us", "39"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert "| 47.70 | 1.50 | 7.50 |" in p.stdout and "workgroup 5 (XCC 1) exits last" in p.stdout
    assert "start delay 0.50 + imbalance 7.00 + tail 0.20 + steps slower than ideal 1.00" in p.stdout


@pytest.mark.parametrize("field,value,word", [("stamps", 0, "unwritten"),
                                              ("shader_clock", 0, "unwritten"),
                                              ("hw", 0xFFFFFFFF, "unwritten")])
def test_a_sentinel_cell_is_rejected(field, value, word):
    t = synthetic()
    t[field][7][1] = value
    with pytest.raises(timeline_report.TimelineError, match=rf"{field}: workgroup 7 .*{word}"):
        timeline_report.analyse(t)


def test_a_decreasing_row_is_rejected(tmp_path):
    t = synthetic()
    t["stamps"][3][2] = t["stamps"][3][1] - 1
    with pytest.raises(timeline_report.TimelineError, match="workgroup 3 goes backwards"):
        timeline_report.analyse(t)
    f = tmp_path / "bad.json"
    f.write_text(json.dumps(t))
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "timeline_report.py"), str(f)],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "workgroup 3" in p.stderr


def test_a_wrong_shape_is_rejected():
    t = synthetic()
    t["stamps"][2].pop()
    with pytest.raises(timeline_report.TimelineError, match="workgroup 2 has 5 cells, not 6"):
        timeline_report.analyse(t)


# ------------------------------------------------------------------ the first readings
# tests/golden/timeline_*.json.gz: the three timelines profiles/r7/timeline.md reads (one
# MI355X; gzip -n9 of what `miint bench --timeline` wrote). (file, ideal us) -> the figures
# the document quotes: span, last workgroup and its XCC, start delay, imbalance, exit segment.
# ..., and the workgroups that entered after the first exit.
READINGS = {
    "timeline_g1_20.json.gz": (1413.64, 141431, 1717, 3, 29687, 31206, 20, 256),
    "timeline_share8_20.json.gz": (176.71, 18806, 155, 1, 10, 440, 20, 0),
    "timeline_g1_1.json.gz": (None, 7579, 1543, 5, 3051, 420, 20, 264),
}


@pytest.mark.parametrize("name", list(READINGS))
def test_the_committed_readings_give_the_documents_figures(name):
    ideal, span, last, xcc, delay, excess, exit_seg, late = READINGS[name]
    t = timeline_report.load(os.path.join(REPO, "tests", "golden", name))
    r = timeline_report.analyse(t, ideal)
    assert (r["span_ticks"], r["last_workgroup"], r["last_xcc"]) == (span, last, xcc)
    assert (r["start_delay_ticks"], r["excess_ticks"], r["exit_segment_ticks"]) == (delay, excess,
                                                                                  exit_seg)
    assert r["start_delay_ticks"] + r["last_steps_ticks"] + r["exit_segment_ticks"] == span
    assert r["span_us"] <= t["device_us"] and len(r["per_xcc"]) == 8
    assert r["late_entries"] == late and r["resident_at_first_exit"] == t["grid"] - late
    if ideal is not None:
        terms = sum(r[k] for k in ("gap_start_delay_ticks", "gap_imbalance_ticks",
                                   "gap_tail_ticks", "gap_steps_slower_ticks"))
        assert terms == pytest.approx(r["gap_ticks"], abs=1e-6)
    with open(os.path.join(REPO, "profiles", "r7", "timeline.md")) as f:
        assert f"= span {r['span_us']:.2f} us" in f.read()


# ------------------------------------------------------------------ the kernels' assembly
TL = r"riemann_timeline_kernel(?:_o8)?ILNS_7DivModeE"
PAIRS = {  # timeline kernel, the guard's pattern of its plain twin
    "pi4_series_exact": (TL + r"3ENS_3Pi4EEEv", isa_guard.GUARDED["ms_pi4_series_exact"][1]),
    "table_series": (TL + r"0ENS_5TableEEEv", isa_guard.GUARDED["ms_table_series"][1]),
}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(isa_guard.HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        return list(isa_guard.functions(isa_guard.compile_asm("riemann", d)))


@pytest.mark.parametrize("name", list(PAIRS))
def test_timeline_kernel_next_to_its_plain_twin(kernels, name):
    tl_pat, plain_pat = PAIRS[name]
    tl = [k for k in kernels if re.search(tl_pat, k[0])]
    plain = [k for k in kernels if re.search(plain_pat, k[0])]
    assert len(tl) == 1 and len(plain) == 1
    assert not re.search(isa_guard.MS, tl[0][0])  # the guard does not take it for a plan's kernel
    (_, tl_body, tl_info), (_, plain_body, plain_info) = tl[0], plain[0]
    assert isa_guard.field(tl_info, "ScratchSize") == 0
    # the same waves per SIMD: the same residency, so the plan's grid fits the timeline kernel
    assert isa_guard.field(tl_info, "Occupancy") == isa_guard.field(plain_info, "Occupancy")
    # one stamp at entry, one in the step loop, one at exit; none in the plans' kernel
    assert tl_body.count("s_memrealtime") == 3 and tl_body.count("s_memtime") == 2
    assert "s_memrealtime" not in plain_body and "s_memtime" not in plain_body
    assert "s_getreg_b32" not in plain_body


def test_every_plain_multistep_kernel_is_free_of_stamps(kernels):
    plain = [k for k in kernels if re.search(isa_guard.MS, k[0])]
    assert len(plain) >= 30
    for sym, body, _ in plain:
        assert "s_memrealtime" not in body and "s_memtime" not in body, sym
    tl = [k for k in kernels if re.search(TL, k[0])]
    assert tl and all(isa_guard.field(info, "ScratchSize") == 0 for _, _, info in tl)


@pytest.mark.parametrize("bad", ["3", "2/2", "-1/4", "a/b", "1/2x", "0/0"])
def test_a_malformed_slice_gets_a_message(bad):
    exe = os.path.join(REPO, "build", "bin", "miint")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    for cmd in ("bench", "table2d"):
        p = subprocess.run([exe, cmd, "--slice=" + bad], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--slice wants R/W with 0 <= R < W" in p.stderr, p.stderr


def test_help_lists_the_flag():
    exe = os.path.join(REPO, "build", "bin", "miint")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    p = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--timeline FILE" in p.stdout + p.stderr
