"""The camera prelude of variant 22 against the walk:
variant 30 is 22 without the tile list, every segment through the walk.  The
body test, the acceptance and the draws are the walk's, and the gate on the
prelude's trips (kPreMin) only moves a camera segment to a later trip, so every
case renders both variants and compares the frames and both counters
(segments, samples) bit for bit, with the loop-free samplers and with
RT_FLAG_REJECTION_SAMPLERS, at depth 8.

The cluster scenes put 15, 16 and 17 bodies into one tile's list: the counts
are lib/tile_list_check's (`count`: csrc/tile_list.h built for the host),
checked here on the CPU.  They were the boundary cases of round 21's dense tile
records -- copies of up to 16 listed bodies in four records of the leaf layout,
which rendered these same bits and were taken out again for their LDS (DESIGN.md
§8.2) -- and stay as lists of several leaf records in one tile; cover(3)'s own
centre tiles hold 19 and 20 bodies.  The 3-spp case is the gate's drain case: a
pool spent from the start, whose waves' last unstarted samples must still get
their trip.  The last test runs tools/simt_sim.cpp, the CPU model, without and
with the gate (PREK): the same samples and segments, so the policy only
reorders work.
"""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "raytracing-clj_amd" / "lib"
CHECK = LIB / "tile_list_check"

WALK, LIST = 30, 22
W, H, SPP, DEPTH = 40, 24, 8, 8
TILE = (2, 0)   # the cluster's tile: columns 16..23, rows 0..7 (cover(3) alone: 7 bodies)
FLAGS = ["direct", "rejection"]


def _flags(name):
    from rtclj import _lib
    return 0 if name == "direct" else _lib.RT_FLAG_REJECTION_SAMPLERS


def _variant(v):
    from rtclj._lib import lib
    old = lib.rt_set_variant(v)
    assert old >= 0, f"rt_set_variant({v}) refused"
    return old


def _both(render):
    """render() under the walk and under the list: (frame, counters) each."""
    from rtclj._lib import lib
    got = {}
    old = _variant(WALK)
    try:
        for v in (WALK, LIST):
            _variant(v)
            got[v] = render()
    finally:
        lib.rt_set_variant(old)
    return got[WALK], got[LIST]


def _render(sc, cam, w, h, spp, flags=0, seed=3):
    from rtclj import raytracing as R

    def go():
        st = {}
        out = R.render(sc, cam, w, h, spp=spp, max_depth=DEPTH, seed=seed, n_devices=1, stats=st, flags=flags)
        return out, (st.get("segments"), st.get("samples"))
    return go


def _same(a, b, what=""):
    (fa, ca), (fb, cb) = a, b
    assert fa.shape == fb.shape and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), \
        f"{what}: {float((fa == fb).all(axis=-1).mean()):.4%} pixels bit-exact"
    assert ca == cb, (what, ca, cb)


def _kept(sc, cam, tile, tmp):
    """lib/tile_list_check's list length of the 8 x 8 tile (tx, ty)."""
    assert CHECK.exists(), f"{CHECK} missing: run __graft_entry__.build()"
    x0, y0 = 8 * tile[0], 8 * tile[1]
    lines = [" ".join(repr(float(np.float32(v))) for v in cam.as_list()) + f" {int(cam.defocus)}",
             f"{x0} {x0 + 7} {y0} {y0 + 7}"]
    lines += [" ".join(repr(float(v)) for v in b) for b in np.asarray(sc.sphere, np.float32)]
    path = Path(tmp) / "tile.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([str(CHECK), "count", str(path)], capture_output=True, text=True, timeout=30)
    assert p.returncode == 0, p.stderr[-500:]
    m = re.search(r'"bodies": (\d+), "kept": (\d+)', p.stdout)
    assert m and int(m.group(1)) == len(sc.sphere), p.stdout
    return int(m.group(2))


def _cluster(n, tmp):
    """cover(3) plus small spheres inside tile TILE's view, in front of the
    scene, until the tile's list holds exactly n bodies."""
    from rtclj import raytracing as R
    from rtclj import scenes
    base = scenes.cover(3)
    cam = scenes.cover_camera(W, H)
    have = _kept(base, cam, TILE, tmp)
    assert have < 15, f"cover(3) alone puts {have} bodies into tile {TILE}"
    c, p00, du, dv = (np.array(v[:], np.float64) for v in (cam.center, cam.p00, cam.du, cam.dv))
    sph, kind, mat = [base.sphere], [base.kind], [base.mat]
    for i in range(n - have):
        # a point of the ray through the tile, a third of the way to the focus
        # plane, the bodies a pixel and a half apart and one behind the other
        fx, fy = 8 * TILE[0] + 1.25 + 1.5 * (i % 4), 8 * TILE[1] + 1.25 + 1.5 * ((i // 4) % 4)
        s = 0.30 + 0.008 * i
        pt = c + s * (p00 + fx * du + fy * dv - c)
        sph.append(np.array([[pt[0], pt[1], pt[2], 0.02]], np.float32))
        k = (R.RT_LAMBERTIAN, R.RT_METAL, R.RT_DIELECTRIC)[i % 3]
        kind.append(np.array([k], np.int32))
        mat.append(np.array([(0.8, 0.3, 0.3, 0.0) if i % 3 == 0 else (0.7, 0.7, 0.9, 0.1) if i % 3 == 1
                             else (0.0, 0.0, 0.0, 1.5)], np.float32))
    sc = R.Scene(np.vstack(sph), np.concatenate(kind), np.vstack(mat))
    return sc, cam


@pytest.mark.parametrize("n", [15, 16, 17])
def test_cluster_scenes_put_n_bodies_into_the_tiles_list(n, tmp_path):
    """On the CPU: the scenes the GPU cases below render are the boundary tiles."""
    sc, cam = _cluster(n, tmp_path)
    assert _kept(sc, cam, TILE, tmp_path) == n


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_cover3(gpu_lib, flags):
    from rtclj import scenes
    _same(*_both(_render(scenes.cover(3), scenes.cover_camera(W, H), W, H, SPP, _flags(flags))), "cover(3)")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [15, 16, 17])
def test_cluster_in_one_tile(gpu_lib, tmp_path, n, flags):
    sc, cam = _cluster(n, tmp_path)
    _same(*_both(_render(sc, cam, W, H, SPP, _flags(flags))), f"cluster of {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_empty_scene(gpu_lib, flags):
    from rtclj import raytracing as R
    from rtclj import scenes
    sc = R.Scene(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, 4), np.float32))
    _same(*_both(_render(sc, scenes.cover_camera(W, H), W, H, SPP, _flags(flags))), "empty scene")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_big_bodies_only(gpu_lib, flags):
    """The ground and the three r = 1 bodies: no tree to speak of, every tile's list from the big bodies' leaf."""
    from rtclj import scenes
    sc = scenes.cover(3, max_bodies=4)
    _same(*_both(_render(sc, scenes.cover_camera(W, H), W, H, SPP, _flags(flags))), "big bodies only")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_partial_edge_tiles(gpu_lib, flags):
    from rtclj import scenes
    w, h = 37, 21
    _same(*_both(_render(scenes.cover(3), scenes.cover_camera(w, h), w, h, SPP, _flags(flags))), "37 x 21")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_sharded_launch(gpu_lib, flags):
    """row_tile = 8, tile_first = 1, tile_step = 2: the odd 8-row bands of the frame."""
    import torch
    from rtclj import scenes
    from rtclj._lib import check, lib, rt_params
    sc, cam = scenes.cover(3), scenes.cover_camera(W, H)
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    try:
        p = rt_params(width=W, height=H, row_begin=0, row_end=H, spp=SPP, max_depth=DEPTH, seed=7, row_tile=8,
                      tile_first=1, tile_step=2, flags=_flags(flags))
        rows = lib.rt_rows_out(C.byref(p))
        assert rows == 8

        def go():
            out = torch.full((rows * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()), None))
            torch.cuda.synchronize()
            return out.cpu().numpy().reshape(rows, W, 3), tuple(cnt.cpu().tolist())
        _same(*_both(go), "sharded launch")
    finally:
        lib.rt_scene_free(ds)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_fewer_samples_than_lanes(gpu_lib, flags):
    """3 spp on 16 x 8: 192 samples a tile for a workgroup's 256 lanes -- the
    pool is spent at the start, the waves' last fresh lanes must still get their trip."""
    from rtclj import scenes
    w, h = 16, 8
    _same(*_both(_render(scenes.cover(3), scenes.cover_camera(w, h), w, h, 3, _flags(flags))), "3 spp on 16 x 8")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_realm(gpu_lib, flags):
    from rtclj import _lib, scenes
    _same(*_both(_render(scenes.cover(3), scenes.cover_camera(W, H), W, H, SPP, _lib.RT_FLAG_REALM | _flags(flags))),
          "RT_FLAG_REALM")


@pytest.mark.gpu
def test_statistics_build_counts_the_prelude(gpu_lib):
    """Variant 31 (22 with counters, the diagnostic library) renders 30's bits,
    and rt_debug_stats 27-31 add up on the scene of the four big bodies (one or
    two leaf records: every tile has a list): every sample starts in a trip, a
    trip holds at most 64 lanes, the trips' leaf and exact passes are among all
    of them, a walk segment after a trip is a walk segment."""
    from rtclj import raytracing as R
    from rtclj import scenes
    from rtclj._lib import check, diag_lib
    d = diag_lib()
    sc, cam = scenes.cover(3, max_bodies=4), scenes.cover_camera(W, H)
    got = {}
    old = d.rt_set_variant(WALK)
    assert old >= 0
    try:
        for v in (WALK, 31):
            assert d.rt_set_variant(v) >= 0, v
            check(d.rt_debug_stats((C.c_uint64 * 32)()))   # clear
            st = {}
            out = R.render(sc, cam, W, H, spp=SPP, max_depth=DEPTH, seed=3, n_devices=1, stats=st, library=d)
            dbg = (C.c_uint64 * 32)()
            check(d.rt_debug_stats(dbg))
            got[v] = (out, (st["segments"], st["samples"])), [int(x) for x in dbg]
    finally:
        d.rt_set_variant(old)
    _same(got[WALK][0], got[31][0], "variant 31")
    s = got[31][1]
    calls, trips, lanes, leafs, exacts, after = s[0], s[27], s[28], s[29], s[30], s[31]
    samples = got[31][0][1][1]
    print(dict(calls=calls, trips=trips, lanes=lanes, leafs=leafs, exacts=exacts, after=after, samples=samples))
    assert 0 < trips < calls and trips <= lanes <= 64 * trips
    assert lanes <= samples == W * H * SPP
    assert 0 < leafs <= s[12] and exacts <= s[13] and after <= calls - trips
    assert lanes == samples   # (under the gate no lane of a listed tile walks its camera segment)


def test_the_models_gate_only_reorders_work(tmp_path):
    """tools/simt_sim.cpp on 20 tiles of C1 with the prelude, without and with
    the gate (PREK=16): the same samples, the same segments."""
    exe = tmp_path / "simt_sim"
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(ROOT / "include"), str(ROOT / "tools" / "simt_sim.cpp"),
                        str(ROOT / "raytracing-clj_amd" / "csrc" / "bvh.cpp"), f"-L{LIB}", "-lrtclj",
                        f"-Wl,-rpath,{LIB}", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    counts, lanes = {}, {}
    for prek in ("0", "16"):
        env = dict(os.environ, PADT="1", PRE="2", INFL="2", NV="1", PREK=prek)
        r = subprocess.run([str(exe), "20", "100"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        m = re.search(r"counts: samples (\d+) segments (\d+)", r.stdout)
        t = re.search(r"prelude: ([0-9.]+) trips per wave-iter, ([0-9.]+) lanes a trip", r.stdout)
        assert m and t, r.stdout[-2000:]
        counts[prek], lanes[prek] = (int(m.group(1)), int(m.group(2))), float(t.group(2))
        print(prek, counts[prek], t.groups())
    assert counts["0"] == counts["16"] and counts["0"][0] == 20 * 64 * 100, counts
    assert lanes["16"] > lanes["0"], lanes   # (the gate is on: fuller trips)
