"""The feature pass's hit search on the CPU (no GPU needed):
lib/first_hit_check is csrc/first_hit.h -- the text feat_kernel runs -- built
for the host.  For every ray the stack walk over each of bvh_build's three
trees (2, 4 and 8 bodies per leaf) must return the linear scan's (body, t
bits); the counts below, taken on the scan's own results, keep the comparison
from being vacuous.  The same tool then takes the edge scenes' bodies
(tests/edge_scenes.py) and the oracle's camera rays for them from files."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edge_scenes as E
import feat_oracle as F

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "first_hit_check"


@pytest.fixture(scope="module")
def report():
    assert TOOL.exists(), "lib/first_hit_check is not built (make -C raytracing-clj_amd)"
    r = subprocess.run([str(TOOL), "42"], capture_output=True, text=True, timeout=300)
    assert r.stdout.strip(), (r.returncode, r.stderr)
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    rep["returncode"] = r.returncode
    return rep


def test_walk_equals_scan_for_every_leaf_size(report):
    assert report["mismatches"] == {"2": 0, "4": 0, "8": 0}
    assert report["returncode"] == 0


def test_the_rays_exercise_what_they_should(report):
    cam = report["camera_rays"]
    assert report["rays"] >= 200_000 and report["rays"] == 2 * cam
    assert report["camera_hits"] >= 0.1 * cam and report["camera_misses"] >= 0.1 * cam
    assert report["camera_hits"] + report["camera_misses"] == cam
    # equal t, the lower index wins: the duplicated scene
    assert report["tie_rays"] >= 1000
    # the big bodies' leaves, taken before the tree
    if report["cover_big_bodies"] > 0:
        assert report["big_hits"] >= 1000


def test_the_stack_bound_the_kernel_sizes_its_rows_by(report):
    """feat_kernel's LDS stack holds depth + 1 rows per lane; the walk never
    has more than depth - 1 entries pending."""
    assert report["stack_over_depth"] == 0
    assert 0 < report["stack_peak"] <= report["max_depth"] - 1


# ---- the edge scenes' bodies under the oracle's camera rays (--scene / --rays) --------------------
EDGE_CASES = (["nonfinite_few", "nonfinite_64", "nonfinite_65", "nonfinite_80", "neg_radius_field", "ties_big",
               "ties_big_glass", "origin_on_surface", "camera_inside_glass"] + [f"scale_2^{k}" for k in E.SCALES])
EDGE_SPP = 4


def dump_case(name, directory):
    """The case's bodies and the mirror's 64 x 36 x 4 camera rays as the tool
    reads them -> (scene file, rays file, the mirror's features)."""
    sc, cam, meta = E.case(name)
    m = F.edge_mirror(name, spp=EDGE_SPP, detail=True)
    scene, rays = directory / "scene.f32", directory / "rays.f32"
    sc.sphere.astype("<f4").tofile(scene)
    m["rays"].astype("<f4").tofile(rays)
    return scene, rays, m


@pytest.mark.parametrize("name", EDGE_CASES)
def test_walk_equals_scan_on_edge_scenes(name, tmp_path):
    """Non-finite bodies on either side of 64, negative radii, twins across
    the big-body list, origins on a surface and inside a body, and scenes
    scaled until |d|^2 underflows or overflows (scale_2^63: u = inf * 0): the
    walk ends, stays within its stack and returns the scan's answer, and the
    scan's hits are those the oracle's mirror found for the same rays."""
    assert TOOL.exists(), "lib/first_hit_check is not built (make -C raytracing-clj_amd)"
    scene, rays, m = dump_case(name, tmp_path)
    r = subprocess.run([str(TOOL), "--scene", str(scene), "--rays", str(rays)], capture_output=True, text=True,
                       timeout=120)
    assert r.stdout.strip(), (r.returncode, r.stderr)
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(name, rep)
    assert r.returncode == 0 and rep["mismatches"] == {"2": 0, "4": 0, "8": 0}
    assert rep["stack_over_depth"] == 0 and rep["stack_peak"] <= max(rep["max_depth"] - 1, 0)
    sc = E.case(name)[0]
    assert rep["bodies"] == len(sc) and rep["rays"] == E.W * E.H * EDGE_SPP
    # the scan (first_hit.h) and the oracle's own text agree on what is hit
    assert rep["hits"] == int((m["body"] >= 0).sum())
    if name == "scale_2^63":
        assert rep["hits"] == 0 and rep["odd_rays"] == rep["rays"]
    else:
        assert rep["hits"] > 0 and rep["odd_rays"] == 0
    if name.startswith("nonfinite_"):
        assert not np.isfinite(sc.sphere).all()
    if name.startswith("ties_big"):
        assert rep["big_bodies"] == 8
