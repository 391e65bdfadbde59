"""The series_exact tiles form and square each sample's residual in packed fp32
(integrands.hpp Pi4::tile_acc): one v_pk_fma_f32 forms the two residuals of a +-k pair from an
SGPR pair (k, -k), a second adds their two squares, so the pair loop costs 1.0 VALU per sample
instead of 2.0 fp64. Pinned through tools/isa_guard.py on the gfx950 assembly: 465 / 466 VALU
per 384-sample tile (1.211 / 1.214 per sample; 821 / 822 with fp64 squares), hence the 1.25
limit (the guard's 3 % margin). The series (g-fold) tiles stay fp64 — their g^2 carries the
linear term — and must not move."""
from __future__ import annotations

import json
import os
import re
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import isa_guard  # noqa: E402

NAMES = ("pi4_series_exact", "ms_pi4_series_exact", "pi4_series", "ms_pi4_series")


@pytest.fixture(scope="module")
def kernels():
    """name -> (stats, function body) from one device-only compile of riemann.hip."""
    if not os.path.exists(isa_guard.HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        fns = list(isa_guard.functions(isa_guard.compile_asm("riemann", d)))
    out = {}
    for name in NAMES:
        _, pat, tile = isa_guard.GUARDED[name]
        sym, body, info = next(f for f in fns if re.search(pat, f[0]))
        out[name] = (dict(isa_guard.stats(body, info, tile), symbol=sym), body)
    return out


def longest_block(body: str) -> list[str]:
    """Instructions of the straight-line block with the most VALU (one tile)."""
    blocks, _ = isa_guard.cfg(body)
    return max(blocks, key=lambda b: sum(1 for s in b if s.startswith("v_")))


def test_single_launch_tile_is_one_valu_per_sample_in_the_loop(kernels):
    assert kernels["pi4_series_exact"][0]["valu_per_sample"] <= 1.25


def test_multistep_tile_is_one_valu_per_sample_at_seven_waves(kernels):
    ms = kernels["ms_pi4_series_exact"][0]
    assert ms["max_block_valu"] / 384 <= 1.25
    assert ms["scratch"] == 0 and ms["vgpr"] <= 64 and ms["occupancy"] >= 7


@pytest.mark.parametrize("name", ["pi4_series_exact", "ms_pi4_series_exact"])
def test_tile_block_holds_a_packed_fma_per_sample(kernels, name):
    """192 pairs, each one packed FMA for its two residuals and one for their squares."""
    block = longest_block(kernels[name][1])
    packed = [s for s in block if s.split()[0] == "v_pk_fma_f32"]
    assert len(packed) >= 384, len(packed)
    # the residuals' (k, -k) comes straight from an SGPR pair: no move into VGPRs per pair
    assert sum(1 for s in packed if re.match(r"v_pk_fma_f32 v\[\d+:\d+\], s\[\d+:\d+\],", s)) >= 192
    assert sum(1 for s in block if s.split()[0] == "v_fma_f64") <= 60  # seed, centres, fold


def test_series_fold_kernels_are_untouched(kernels):
    with open(isa_guard.BASELINE) as f:
        base = json.load(f)
    for name in ("pi4_series", "ms_pi4_series"):
        assert kernels[name][0] == base[name], name
