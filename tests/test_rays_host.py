"""Ray queries on the host (include/rt.h: rt_rays_host, rt_occluded_host; no GPU
needed): the pinhole rays give rt_ids_host's integers and the feature mirror's
depths; caller-made rays agree with a float64 reading of hittable.clj:7-31 and
raytracing.clj:33-43 wherever that reading is not itself a close call; every
inactive class gives the "none" record; the self-hit guard; occlusion equals
"a body was found" on all of it; first_hit.h's walks give the scan's bits on
query rays (lib/rays_check, which also runs the host passes under the
sanitizers); the binding matches the header.
"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edge_scenes as E
import feat_oracle as FO
import ray_sets as RS

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "rays_check"
F = np.float32
RAY_FUNCS = ("rt_launch_rays", "rt_launch_occluded", "rt_rays_host", "rt_occluded_host", "rt_rays_occupancy")
# the edge scenes rt_launch_ids is held to (tests/test_gpu_motion.py)
EDGE_NAMES = ("ties", "ties_big", "nonfinite_few", "nonfinite_64", "nonfinite_65", "nonfinite_80",
              "bubble_negative_radius", "neg_radius_field", "camera_inside_glass")


def R():
    from rtclj import raytracing
    return raytracing


def camera_of(name, w, h):
    from rtclj import scenes
    return R().camera(w, h, **R().REFERENCE_CAMERA) if name == "reference" else scenes.cover_camera(w, h)


# ---- pinhole agreement -----------------------------------------------------------------
@pytest.mark.parametrize("name", ("reference", "cover"))
def test_pinhole_rays_give_the_id_pass(name):
    """pinhole_rays through rt_rays_host: rt_ids_host's integers on a 64 x 40
    frame, a row band included; the records are whole (t = dist / |d|, unit
    normals against d, reserved 0)."""
    w, h = 64, 40
    sc, cam = RS.scene(name), camera_of(name, w, h)
    rays = R().pinhole_rays(cam, w, h)
    assert rays.shape == (h, w) and (rays["t_min"] == F(1e-3)).all() and np.isinf(rays["t_max"]).all()
    hits = R().rays_host(sc, rays)
    want = R().ids_host(sc, cam, w, h)
    assert np.array_equal(hits["body"], want)
    assert len(np.unique(want)) >= (4 if name == "reference" else 15) and (name == "reference" or (want == -1).any())
    band = R().rays_host(sc, R().pinhole_rays(cam, w, 9, row0=17))
    assert np.array_equal(RS.words(band), RS.words(hits[17:26]))
    hit = hits["body"] >= 0
    assert np.array_equal(RS.words(hits[~hit]), RS.words(RS.none_records(int((~hit).sum()))))
    n = hits["normal"][hit].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    assert ((rays["d"][hit].astype(np.float64) * n).sum(axis=1) < 0).all()
    assert (hits["reserved"] == 0).all() and np.isin(hits["front_face"], (0, 1)).all()
    assert np.array_equal(R().occluded_host(sc, rays), hit)


@pytest.mark.parametrize("name", ("reference", "cover"))
def test_dist_is_the_feature_samples_depth(name):
    """The feature mirror's own camera rays (jitter, defocus disk) through
    rt_rays_host: its body and its depth, bit for bit."""
    w, h = 64, 40
    sc, cam = RS.scene(name), camera_of(name, w, h)
    m = FO.mirror(sc, cam, w, h, 1, 5, want_body=True, want_t=True, want_rays=True)
    q = m["rays"].reshape(-1, 6)
    rays = RS.make_rays(q[:, :3], np.full(len(q), 1e-3), q[:, 3:], np.full(len(q), np.inf))
    hits = R().rays_host(sc, rays)
    assert np.array_equal(hits["body"], m["body"].reshape(-1))
    assert np.array_equal(hits["dist"], m["t"].reshape(-1).astype(F))
    assert (hits["body"] >= 0).sum() > 200


# ---- the float64 reading -----------------------------------------------------------------
@pytest.mark.parametrize("name", ("reference", "cover"))
def test_query_rays_against_float64(name):
    """4096 caller-made rays per scene (RS.query_rays) against RS.ref64.

    A ray is left out only where the float64 answer is a close call
    (RS.ref64's `marginal`, a subset of what such a test may leave out), at most
    2 % of them: none of 4096 on the reference scene, 56 on the cover scene.
    On the rest: the same body;
    |dist - t64 |d|| <= 6e-4 (|oc| + |r|), the position error bvh_pad.h records
    for the fp32 test; t within 4 ulp of dist / |d|; the same front_face.  The
    normal has a test of its own below."""
    sc, rays = RS.scene(name), RS.query_rays(name)
    ref = RS.ref64(sc.sphere, rays)
    hits = R().rays_host(sc, rays)
    keep = ~ref["marginal"]
    print(name, "left out:", int((~keep).sum()), "of", len(rays), "hits:", int((ref["body"] >= 0).sum()))
    assert (~keep).sum() <= 0.02 * len(rays)
    assert (ref["body"][keep] >= 0).sum() > 0.3 * len(rays) and (ref["body"][keep] < 0).sum() > 0.1 * len(rays)
    assert np.isfinite(rays["t_max"]).sum() > 0.4 * len(rays)
    assert np.array_equal(hits["body"][keep], ref["body"][keep])
    k = keep & (ref["body"] >= 0)
    dist, t = hits["dist"][k].astype(np.float64), hits["t"][k].astype(np.float64)
    assert (np.abs(dist - ref["t"][k] * ref["len"][k]) <= 6e-4 * ref["reach"][k]).all()
    q = dist / ref["len"][k]
    assert (np.abs(t - q) <= 4 * np.spacing(q.astype(F)).astype(np.float64)).all()
    assert np.array_equal(hits["front_face"][k] == 1, ref["front"][k])
    assert (hits["front_face"][k] == 0).any() and (hits["front_face"][k] == 1).any()
    assert np.array_equal(R().occluded_host(sc, rays), hits["body"] >= 0)
    # a miss is the "none" record
    miss = hits["body"] < 0
    assert np.array_equal(RS.words(hits[miss]), RS.words(RS.none_records(int(miss.sum()))))


@pytest.mark.parametrize("name", ("reference", "cover"))
def test_query_normals_against_float64(name):
    """The same rays, the same 2 % at most left out: every component of the
    record's normal within 1e-3 of the float64 reading's.

    Largest difference 5.6e-6 on the reference scene, 8.3e-5 on the cover
    scene.  The normal of P = o + dist u would miss the bound there (7.6e-3 on a
    body of r = 0.2 met 27 units away: the fp32 root's error over r), which is
    why the record's normal is rebuilt around the ray's closest point to the
    centre (csrc/ray_query.h, rq_record)."""
    sc, rays = RS.scene(name), RS.query_rays(name)
    ref = RS.ref64(sc.sphere, rays)
    hits = R().rays_host(sc, rays)
    assert ref["marginal"].sum() <= 0.02 * len(rays)
    k = ~ref["marginal"] & (ref["body"] >= 0) & (hits["body"] == ref["body"])
    err = np.abs(hits["normal"][k].astype(np.float64) - ref["normal"][k])
    print(name, "largest normal difference:", err.max(), "above 1e-3:", int((err.max(axis=1) > 1e-3).sum()), "of", int(k.sum()))
    assert err.max() <= 1e-3


# ---- inactive rays, the guard ------------------------------------------------------------
def test_inactive_rays_give_the_none_record():
    names, rays = RS.inactive_rays()
    sc = RS.scene("reference")
    # the active ray every class is a corruption of: the centre body, from (0, 0, 1) along -z
    ok = R().rays_host(sc, RS.make_rays([(0, 0, 1)], [0], [(0, 0, -1)], [np.inf]))[0]
    assert ok["body"] == 1 and ok["front_face"] == 1 and abs(float(ok["dist"]) - 1.7) < 1e-6
    hits = R().rays_host(sc, rays)
    occ = R().occluded_host(sc, rays)
    none = RS.words(RS.none_records(1))[0]
    for i, nm in enumerate(names):
        assert np.array_equal(RS.words(hits[i:i + 1])[0], none), (nm, hits[i])
        assert not occ[i], nm
    # t_max is a strict bound, in units of |d|
    d2 = RS.make_rays([(0, 0, 1)] * 3, [0] * 3, [(0, 0, -2)] * 3, [0.85, np.nextafter(F(0.85), F(1)), 0.5])
    h2 = R().rays_host(sc, d2)
    assert h2["t"][1] == F(0.85) and h2["dist"][1] == ok["dist"], h2
    assert list(h2["body"]) == [-1, 1, -1]
    assert list(R().occluded_host(sc, d2)) == [False, True, False]


def test_last_guards_a_ray_from_a_surface():
    rays, last = RS.guarded_rays()
    sc = RS.scene("reference")
    plain = R().rays_host(sc, rays)
    guarded = R().rays_host(sc, rays, last)
    inward = np.arange(len(rays)) % 2 == 0
    # without the guard an inward ray meets its own body: at about 0, or at the chord's end
    assert (plain["body"][inward] == 1).all()
    assert (plain["dist"][inward] < 1e-5).sum() > 5
    # with it, at the chord's end 2 h (a back face), never near 0; an outward ray never meets it
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    two_h = 2.0 * ((sc.sphere[1, :3].astype(np.float64) - o) * u).sum(axis=1)
    assert (guarded["body"][inward] == 1).all() and (guarded["front_face"][inward] == 0).all()
    assert np.abs(guarded["dist"][inward] - two_h[inward]).max() < 1e-5 and guarded["dist"][inward].min() > 0.5
    assert (guarded["body"][~inward] != 1).all()
    assert np.array_equal(R().occluded_host(sc, rays, last), guarded["body"] >= 0)
    assert np.array_equal(R().occluded_host(sc, rays), plain["body"] >= 0)
    # last < 0 is no guard; last >= n names no body
    for inert in (np.full(len(rays), -1, np.int32), np.full(len(rays), -7, np.int32),
                  np.full(len(rays), len(sc), np.int32), np.full(len(rays), 2**31 - 1, np.int32)):
        assert np.array_equal(RS.words(R().rays_host(sc, rays, inert)), RS.words(plain))
        assert np.array_equal(R().occluded_host(sc, rays, inert), plain["body"] >= 0)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_scenes(name):
    """The edge scenes' pinhole rays: rt_ids_host's integers, occlusion equal
    to them, no NaN in a record."""
    sc, cam, _ = E.case(name)
    rays = R().pinhole_rays(cam, E.W, E.H)
    hits = R().rays_host(sc, rays)
    assert np.array_equal(hits["body"], R().ids_host(sc, cam, E.W, E.H))
    assert np.array_equal(R().occluded_host(sc, rays), hits["body"] >= 0)
    assert not np.isnan(hits["normal"]).any() and not np.isnan(hits["t"]).any()


# ---- walk against scan, the sanitizers ---------------------------------------------------
def run_tool(*args):
    assert TOOL.exists(), "lib/rays_check is not built (make -C raytracing-clj_amd)"
    r = subprocess.run([str(TOOL), *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    return rep


def test_walk_equals_scan_on_query_rays():
    """first_hit.h's fh_walk and fh_walk_any against the scan over bvh_build's
    three trees, on query rays (far and inside origins, surfaces, t_min = 0,
    finite t_max, |d| 2^-6 .. 2^6, guards): 34,000 rays on each of the
    reference scene, the 484-body and the 1025-body cover scene."""
    rep = run_tool("walk", 34000, 11)
    assert rep["bodies"] == [5, 484, 1025] and rep["rays"] == 102000
    assert rep["mismatch_walk"] == [0, 0, 0] and rep["mismatch_any"] == [0, 0, 0] and rep["stack_over"] == 0
    assert rep["active"] > 0.9 * rep["rays"] and rep["hits"] > 0.4 * rep["rays"]
    assert rep["guarded_hits"] > 2000 and rep["finite_tmax"] > 0.3 * rep["rays"] and rep["tmin0"] > 0.3 * rep["rays"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_walk_equals_scan_on_edge_scenes(name, tmp_path):
    sc = E.case(name)[0]
    path = tmp_path / "scene.f32"
    sc.sphere.astype("<f4").tofile(path)
    rep = run_tool("walk", 4000, 3, "--scene", path)
    assert rep["bodies"] == [len(sc)] and rep["rays"] == 4000 and rep["hits"] > 400
    assert rep["mismatch_walk"] == [0, 0, 0] and rep["mismatch_any"] == [0, 0, 0] and rep["stack_over"] == 0


def test_host_passes_under_the_sanitizers():
    """lib/rays_check: csrc/ray_query.h (the bodies of rt_rays_host and
    rt_occluded_host, the text the kernels run) under
    -fsanitize=address,undefined with hostile inputs, a program of its own."""
    rep = run_tool()
    assert rep["bad"] == 0 and rep["hits"] > 1000 and rep["inactive"] >= 17 and rep["guarded"] > 0
    mk = (ROOT / "raytracing-clj_amd" / "Makefile").read_text()
    rule = mk[mk.index("$(OUT)/rays_check:"):]
    assert "-fsanitize=address,undefined,float-cast-overflow" in rule[:700] and "-fno-sanitize-recover=all" in rule[:700]
    assert "-static-libasan" in rule[:700] and "$(OUT)/rays_check" in mk[mk.index("all:"):mk.index("all:") + 600]
    assert "csrc/ray_query.h" in mk[mk.index("HDRS"):mk.index("all:")]


# ---- arguments, the binding ----------------------------------------------------------------
def test_argument_errors_and_n_zero():
    from rtclj._lib import lib, rt_ray, rt_ray_hit, rt_scene, u8ptr
    sc = RS.scene("reference")
    rays = RS.make_rays([(0, 0, 1)], [0], [(0, 0, -1)], [np.inf])
    rp = rays.ctypes.data_as(C.POINTER(rt_ray))
    out = RS.none_records(1)
    out["body"] = 77
    op = out.ctypes.data_as(C.POINTER(rt_ray_hit))
    occ = np.full(1, 9, np.uint8)
    for args in ((None, rp, None, 1, op), (C.byref(sc.c), None, None, 1, op), (C.byref(sc.c), rp, None, 1, None)):
        assert lib.rt_rays_host(*args) == -1 and b"NULL" in lib.rt_last_error()
    for args in ((None, rp, None, 1, u8ptr(occ)), (C.byref(sc.c), None, None, 1, u8ptr(occ)),
                 (C.byref(sc.c), rp, None, 1, None)):
        assert lib.rt_occluded_host(*args) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_rays_host(C.byref(sc.c), rp, None, 1 << 31, op) == -1 and b"2^31" in lib.rt_last_error()
    assert lib.rt_occluded_host(C.byref(sc.c), rp, None, 1 << 31, u8ptr(occ)) == -1 and b"2^31" in lib.rt_last_error()
    bad = rt_scene(-1, None, None, None)
    assert lib.rt_rays_host(C.byref(bad), rp, None, 1, op) == -1 and b"scene" in lib.rt_last_error()
    # n = 0: fine, with or without arrays, nothing written
    assert lib.rt_rays_host(C.byref(sc.c), None, None, 0, None) == 0
    assert lib.rt_rays_host(C.byref(sc.c), rp, None, 0, op) == 0
    assert lib.rt_occluded_host(C.byref(sc.c), None, None, 0, None) == 0
    assert lib.rt_occluded_host(C.byref(sc.c), rp, None, 0, u8ptr(occ)) == 0
    assert out["body"][0] == 77 and occ[0] == 9
    assert R().rays_host(sc, rays[:0]).shape == (0,) and R().occluded_host(sc, rays[:0]).shape == (0,)
    # an empty scene: every ray misses
    empty = R().Scene(np.zeros((0, 4), F), np.zeros(0, np.int32), np.zeros((0, 4), F))
    assert R().rays_host(empty, rays)["body"][0] == -1 and not R().occluded_host(empty, rays)[0]
    # the device entries without a scene: an error, no device call
    assert lib.rt_launch_rays(None, None, None, 1, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_launch_occluded(None, None, None, 1, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_rays_occupancy(None, None) == -1 and b"NULL" in lib.rt_last_error()
    with pytest.raises(ValueError):
        R().rays_host(sc, rays, last=np.zeros(2, np.int32))


def test_binding_matches_the_header():
    from rtclj import _lib
    hdr = (ROOT / "include" / "rt.h").read_text()
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    assert re.search(r"typedef struct rt_ray \{[^}]*float o\[3\];\s*float t_min;[^}]*float d\[3\];\s*float t_max;", hdr)
    assert re.search(r"typedef struct rt_ray_hit \{[^}]*int32_t body;[^}]*int32_t front_face;[^}]*float t;[^}]*"
                     r"float dist;[^}]*float normal\[3\];[^}]*float reserved;", hdr)
    assert C.sizeof(_lib.rt_ray) == 32 and C.sizeof(_lib.rt_ray_hit) == 32
    assert np.dtype(_lib.RAY_DTYPE).itemsize == 32 and np.dtype(_lib.RAY_HIT_DTYPE).itemsize == 32
    assert _lib.rt_ray.t_min.offset == 12 and _lib.rt_ray.d.offset == 16 and _lib.rt_ray.t_max.offset == 28
    assert _lib.rt_ray_hit.t.offset == 8 and _lib.rt_ray_hit.normal.offset == 16 and _lib.rt_ray_hit.reserved.offset == 28
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    n = {f: len(re.search(rf"\b{f}\s*\(([^)]*)\)", body).group(1).split(",")) for f in RAY_FUNCS}
    assert n == {"rt_launch_rays": 6, "rt_launch_occluded": 6, "rt_rays_host": 5, "rt_occluded_host": 5,
                 "rt_rays_occupancy": 2}
    for f in RAY_FUNCS:
        assert len(_lib.SIGNATURES[f][1]) == n[f] and f in _lib.ADDITIVE and hasattr(_lib.lib, f)
        assert hasattr(_lib.diag_lib(), f)
