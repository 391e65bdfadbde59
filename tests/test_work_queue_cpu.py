"""The work queue of the multi-step launch on the CPU box: the queue kernels' resources and
tile counts (tools/isa_guard.py on the gfx950 assembly), where the claim's wait stands, and the
`work` setting's plumbing (RiemannConfig::work, MIINT_MS_WORK, the close = "launch" fallback)."""
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

QUEUE = ["q_pi4_series_exact", "q_pi4_series", "q_pi4f32_series", "q_sin_series",
         "q_table_series", "q_table_ieee", "qt_pi4_series_exact"]
STATIC_OF = {"q_pi4_series_exact": "ms_pi4_series_exact", "q_pi4_series": "ms_pi4_series",
             "q_pi4f32_series": "ms_pi4f32_series", "q_sin_series": "ms_sin_series",
             "q_table_series": "ms_table_series", "q_table_ieee": "ms_table_ieee"}


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(isa_guard.HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        return isa_guard.compile_asm("riemann", d)


@pytest.fixture(scope="module")
def measured(asm):
    fns = list(isa_guard.functions(asm))
    out = {}
    for key in QUEUE + list(STATIC_OF.values()):
        _, pat, tile = isa_guard.GUARDED[key]
        rx = re.compile(pat)
        name, body, info = next((n, b, i) for n, b, i in fns if rx.search(n))
        out[key] = dict(isa_guard.stats(body, info, tile), symbol=name, body=body)
    return out


def test_rows_exist():
    with open(isa_guard.BASELINE) as f:
        base = json.load(f)
    for k in QUEUE:
        assert k in isa_guard.GUARDED and k in base and "missing" not in base[k], k
        assert base[k]["scratch"] == 0 and base[k]["hot_loop_scratch_ops"] == 0, k


def test_no_regression_against_the_baseline(measured):
    with open(isa_guard.BASELINE) as f:
        base = json.load(f)
    now = {k: measured[k] for k in QUEUE}
    assert isa_guard.compare({k: base[k] for k in QUEUE}, now) == []


def test_headline_instantiation(measured):
    """<= 64 VGPRs, >= 7 waves per SIMD, no scratch; the tile's straight line keeps the
    multi-step kernel's counts (<= 430 VALU, >= 402 v_pk_fma_f32 per tile, two tile blocks:
    the round loop's and the exec-masked extra round's)."""
    q, ms = measured["q_pi4_series_exact"], measured["ms_pi4_series_exact"]
    assert q["vgpr"] <= 64 and q["occupancy"] >= 7 and q["scratch"] == 0 and q["agpr"] == 0
    assert q["max_block_valu"] == ms["max_block_valu"] <= 430
    assert q["body"].count("v_pk_fma_f32") == ms["body"].count("v_pk_fma_f32") >= 2 * 402
    tl = measured["qt_pi4_series_exact"]
    assert tl["occupancy"] == q["occupancy"] and tl["scratch"] == 0
    assert tl["max_block_valu"] == q["max_block_valu"]


@pytest.mark.parametrize("key", sorted(STATIC_OF))
def test_queue_twin_keeps_the_static_kernels_shape(measured, key):
    """Every queue kernel: the static kernel's occupancy, no new scratch, the same tile block,
    and an item loop that costs at most 32 VALU more per item than the static step loop. What
    the queue adds per item is three more thread-0 branches (the claim, the LDS word, each a
    compare and an exec save), the claim's operands (a zero offset, the 1, a 64-bit address
    add), the LDS word's write and read and a readfirstlane: about two dozen instructions in
    the loop's text, once per item, not all of them on every wave's path. 32 is 1.3 % of the
    headline's item (5.7 rounds of a 427-VALU tile at N = 1e9)."""
    q, ms = measured[key], measured[STATIC_OF[key]]
    assert q["occupancy"] >= ms["occupancy"] and q["scratch"] <= ms["scratch"]
    assert q["max_block_valu"] <= ms["max_block_valu"]
    assert q["hot_loop_valu"] <= ms["hot_loop_valu"] + 32, (q["hot_loop_valu"], ms["hot_loop_valu"])


def test_the_claims_wait_stands_after_the_tile_loop(measured):
    """In the item loop the claim (global_atomic_add with return) is issued before the tile
    block and nothing waits for vector memory until after the last tile block."""
    lines = [ln.split(";")[0].strip() for ln in measured["q_pi4_series_exact"]["body"].splitlines()]
    lines = [s for s in lines if s]
    claims = [i for i, s in enumerate(lines) if s.startswith("global_atomic_add") and "sc0" in s]
    assert len(claims) == 3  # the first claim, the item loop's, the exit count
    first, loop_claim, exit_count = claims
    fma = [i for i, s in enumerate(lines) if s.startswith("v_pk_fma_f32")]
    assert first < loop_claim < fma[0] and fma[-1] < exit_count
    waits = [i for i, s in enumerate(lines) if s.startswith("s_waitcnt") and "vmcnt" in s
             and loop_claim < i < exit_count]
    assert len(waits) == 1 and waits[0] > fma[-1]
    # the claimed index is handed on through LDS after that wait, before the barrier
    barrier = next(i for i, s in enumerate(lines) if s == "s_barrier" and i > waits[0])
    assert any(s.startswith("ds_write_b32") for s in lines[waits[0]:barrier])
    # no memory operation by inline assembly, no flat atomics
    assert not any(s.startswith("flat_") for s in lines)


# ------------------------------------------------------------------ plumbing (no GPU)
@pytest.fixture(scope="module")
def native():
    from cuda_v_mpi_amd import native as load

    return load(auto_build=False)


def test_resolve_work(native):
    r = native.resolve_work
    assert r("static") == "static" and r("queue") == "queue"
    assert r("auto", None, False) == "static" and r("auto", None, True) == "queue"
    assert r("auto", "", True) == "queue"  # an empty variable is unset
    # MIINT_MS_WORK overrides under auto only
    assert r("auto", "queue", False) == "queue" and r("auto", "static", True) == "static"
    assert r("static", "queue", True) == "static" and r("queue", "static", False) == "queue"
    # plans closed in the launch (and plans without multi-step batches) keep the static kernel
    for work in ("auto", "static", "queue"):
        assert r(work, "queue", True, True) == "static"
    with pytest.raises(RuntimeError, match="work must be auto, static or queue"):
        r("dynamic")
    with pytest.raises(RuntimeError, match="MIINT_MS_WORK must be static or queue"):
        r("auto", "dynamic")


def test_config_and_keyword(native):
    cfg = native.RiemannConfig()
    assert cfg.work == "auto" and cfg.queue_wg_per_cu == 0
    cfg.work = "queue"
    assert cfg.work == "queue"
    from cuda_v_mpi_amd import Integrator

    with pytest.raises(ValueError, match="work must be auto"):
        Integrator("pi4", n=1 << 20, backend="host", work="dynamic")
    assert Integrator("pi4", n=1 << 20, backend="host", work="queue")._cfg.work == "queue"


def test_auto_runs_the_queue_for_the_headline_only(native):
    """riemann_queue_pays: the instantiations whose own A/B showed the queue faster."""
    def pays(integrand, dtype, div, n=10**9):
        return native.riemann_queue_pays(integrand, 0.0, 1.0 / n, 0.0, 0, n, [], 0.0, 0.0,
                                         getattr(native.DType, dtype), getattr(native.DivMode, div))

    assert pays(0, "fp64", "series_exact")
    assert not pays(0, "fp64", "ieee")  # no multi-step kernel at all
    assert not pays(0, "fp64", "series") and not pays(0, "fp32", "series")
    assert not pays(1, "fp64", "series")


def test_cli_flag():
    exe = os.path.join(REPO, "build", "bin", "miint")
    if not os.path.exists(exe):
        pytest.skip("CLI not built")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--work auto|static|queue" in out.stdout + out.stderr
