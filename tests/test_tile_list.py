"""The per-tile body list on the CPU: lib/tile_list_check
(tools/tile_list_check.cpp) drives raytracing-clj_amd/csrc/tile_list.h -- the
text the kernel's workgroup prologue runs, built for the host -- over random
cameras (no defocus, a small aperture, an aperture as large as the focus
distance, a camera 1000 units from the origin) and scenes (bodies in view,
behind the camera, around it, tangent to a tile's extreme rays, far smaller and
far larger than a pixel), every tile of small frames (partial border tiles,
tile heights 1 and 8, rows two image rows apart).  The rays come from the
kernel's fp32 camera arithmetic at the jitter's and the lens's extremes, and
every body is run through the scan's fp32 body test.

Required: every candidate of a ray (disc >= 0 and not (h < 0 and c >= 0)) is in
its tile's list -- zero misses over at least 5 million candidate pairs -- and
the same run with R_f halved does report misses (the cases reach the bound).
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "raytracing-clj_amd" / "lib" / "tile_list_check"


@pytest.fixture(scope="module")
def report():
    assert EXE.exists(), f"{EXE} missing: run __graft_entry__.build()"
    p = subprocess.run([str(EXE), "5000000"], capture_output=True, text=True, timeout=120)
    assert p.returncode in (0, 1), p.stderr[-2000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    return rep, p.stderr


def test_no_candidate_is_missing_from_its_tiles_list(report):
    rep, err = report
    assert rep["candidates"] >= 5_000_000, rep
    assert rep["misses"] == 0, (rep, err[-2000:])


def test_negative_control_reports_misses(report):
    rep, _ = report
    assert rep["control_misses"] > 0, rep


def test_the_cases_are_met(report):
    rep, _ = report
    for key in ("no_defocus", "wide_aperture", "inside", "behind", "tangent", "tiny", "huge", "one_row_tiles",
                "partial_tiles"):
        assert rep[key] > 0, (key, rep)
    # the list culls: not every body of every tile is kept
    assert 0.05 < rep["kept_share"] < 0.9, rep


def test_c1_lists_fit(report):
    """C1's frame: all 12,750 tiles' lists, in bodies and in the 4-body tree's
    leaf records (what the kernel stores: at most 15 a tile)."""
    c1 = report[0]["c1"]
    assert c1["tiles"] == 12750 and c1["bodies"] == 484, c1
    assert c1["share_over_15_records"] == 0.0 and c1["max_records"] <= 15, c1
    assert c1["mean_bodies"] < 4.0, c1
