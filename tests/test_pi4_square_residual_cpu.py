"""The series_exact tiles square a residual without the per-pair curvature term
(integrands.hpp Pi4::tile_acc): 4 fp64 VALU per +-k pair instead of 5. Pinned through
tools/isa_guard.py on the gfx950 assembly: 821 / 822 VALU per 384-sample tile (2.14 per
sample; 1013 / 1014 = 2.64 with the term), hence the 2.15 limit. The series (g-fold) tiles
keep the term — their g^2 = 1/4 + e + e^2 carries the linear part — and must not move."""
from __future__ import annotations

import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import isa_guard  # noqa: E402

NAMES = ("pi4_series_exact", "ms_pi4_series_exact", "pi4_series", "ms_pi4_series")


@pytest.fixture(scope="module")
def measured():
    if not os.path.exists(isa_guard.HIPCC):
        pytest.skip("hipcc not available")
    return isa_guard.measure(NAMES)


def test_single_launch_tile_is_two_valu_per_sample(measured):
    assert measured["pi4_series_exact"]["valu_per_sample"] <= 2.15


def test_multistep_tile_is_two_valu_per_sample_at_seven_waves(measured):
    ms = measured["ms_pi4_series_exact"]
    assert ms["max_block_valu"] / 384 <= 2.15
    assert ms["scratch"] == 0 and ms["vgpr"] <= 64 and ms["occupancy"] >= 7


def test_series_fold_kernels_are_untouched(measured):
    with open(isa_guard.BASELINE) as f:
        base = json.load(f)
    for name in ("pi4_series", "ms_pi4_series"):
        assert measured[name] == base[name], name
