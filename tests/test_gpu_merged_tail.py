"""The merged tail of variant 22's wave iteration: the walk's
hits and the prelude trip's camera rays are shaded in one pass, the walk's
misses leave early (the miss exit).  Per path the operations and the draws are
those of variant 30, the same kernel without the prelude, and the colour sums
are integers, so every case renders variant 30, variant 22 and the default
choice (0) and compares the frames as uint32 and both counters (segments,
samples) bit for bit; one case also against the oracle's fp32 mirror.

The cases are the branches the rotated loop adds: trips whose lanes all end in
the tail with no walk at all (camera rays into the sky), a camera segment that
is the path's last (max_depth 1, 2: rem == 0 inside the tail), paths absorbed
in the tail (metal with fuzz 1), the dielectric block with trip and walk lanes
together (glass only), pools smaller than a wave and gates that never fill
(spp 1, 3, 17 on one tile; 100 for the refills), tiles without a list beside
listed ones (the plain flow and the rotated one in one launch), partial edge
tiles, a sharded launch, the rejection samplers and RT_FLAG_REALM.  Frames are
at most 32 x 24.  The CPU test runs tools/simt_sim.cpp's TAIL switch: the same
samples and segments, fewer VALU instructions per sample.
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

WALK, LIST, AUTO = 30, 22, 0
W, H, SPP, DEPTH = 32, 24, 8, 8
TILE = (1, 1)   # the clusters' tile: columns 8..15, rows 8..15


def _render_all(render):
    """render() under the walk, the list and the default choice: (frame, counters) each."""
    from rtclj._lib import lib
    got = {}
    old = lib.rt_set_variant(WALK)
    assert old >= 0, "rt_set_variant(30) refused"
    try:
        for v in (WALK, LIST, AUTO):
            assert lib.rt_set_variant(v) >= 0, f"rt_set_variant({v}) refused"
            got[v] = render()
    finally:
        lib.rt_set_variant(old)
    return got


def _render(sc, cam, w, h, spp, depth=DEPTH, flags=0, seed=5):
    from rtclj import raytracing as R

    def go():
        st = {}
        out = R.render(sc, cam, w, h, spp=spp, max_depth=depth, seed=seed, n_devices=1, stats=st, flags=flags)
        return out, (st.get("segments"), st.get("samples"))
    return go


def _same(got, what):
    fa, ca = got[WALK]
    for v in (LIST, AUTO):
        fb, cb = got[v]
        assert fa.shape == fb.shape and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), \
            f"{what}, variant {v}: {float((fa == fb).all(axis=-1).mean()):.4%} pixels bit-exact"
        assert ca == cb, (what, v, ca, cb)
    return fa, ca


def _check(sc, cam, w, h, spp, what, **kw):
    out, (segs, samples) = _same(_render_all(_render(sc, cam, w, h, spp, **kw)), what)
    assert samples == w * h * spp, (what, samples)
    return out, segs


def _sky_camera(w, h):
    """Above the cover scene, looking up: every camera ray ends in the sky."""
    from rtclj import raytracing as R
    return R.camera(w, h, vfov=20.0, look_from=(0.0, 5.0, 0.0), look_at=(0.0, 15.0, 2.0), vup=(0.0, 1.0, 0.0),
                    defocus_angle=0.6, focus_dist=10.0)


def _cluster(kind, mat, n=8):
    """The ground and n small bodies of one material in tile TILE's view, a
    pixel and a half apart and one behind the other."""
    from rtclj import raytracing as R
    from rtclj import scenes
    base = scenes.cover(3, max_bodies=4)
    cam = scenes.cover_camera(W, H)
    c, p00, du, dv = (np.array(v[:], np.float64) for v in (cam.center, cam.p00, cam.du, cam.dv))
    sph, kinds, mats = [base.sphere[:1]], [base.kind[:1]], [base.mat[:1]]
    for i in range(n):
        fx, fy = 8 * TILE[0] + 1.25 + 1.5 * (i % 4), 8 * TILE[1] + 1.25 + 1.5 * ((i // 4) % 4)
        s = 0.30 + 0.008 * i
        pt = c + s * (p00 + fx * du + fy * dv - c)
        sph.append(np.array([[pt[0], pt[1], pt[2], 0.05]], np.float32))
        kinds.append(np.array([kind], np.int32))
        mats.append(np.array([mat], np.float32))
    return R.Scene(np.vstack(sph), np.concatenate(kinds), np.vstack(mats)), cam


@pytest.mark.gpu
def test_cover3_and_the_oracle(gpu_lib):
    """cover(3) under the three variants, and against MODE_MIRROR32 | DIRECT."""
    import oracle
    from rtclj import scenes
    sc, cam = scenes.cover(3), scenes.cover_camera(W, H)
    out, segs = _check(sc, cam, W, H, SPP, "cover(3)")
    m32, _, osegs, osamples = oracle.render(oracle.MODE_MIRROR32 | oracle.DIRECT, sc.sphere.astype(np.float64), sc.kind,
                                            sc.mat.astype(np.float64), cam.as_list(), cam.defocus, W, H, SPP, DEPTH,
                                            seed=5)
    assert np.array_equal(out.view(np.uint32), m32.view(np.uint32)), \
        f"GPU vs fp32 mirror: {float((out == m32).all(axis=-1).mean()):.4%} pixels bit-exact"
    assert (segs, W * H * SPP) == (osegs, osamples)


@pytest.mark.gpu
def test_empty_scene(gpu_lib):
    """No body: every trip's lanes end in the tail, no walk ever runs."""
    from rtclj import raytracing as R
    from rtclj import scenes
    sc = R.Scene(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, 4), np.float32))
    _, segs = _check(sc, scenes.cover_camera(W, H), W, H, SPP, "empty scene")
    assert segs == W * H * SPP


@pytest.mark.gpu
def test_camera_turned_to_the_sky(gpu_lib):
    from rtclj import scenes
    _, segs = _check(scenes.cover(3), _sky_camera(W, H), W, H, SPP, "cover(3), camera to the sky")
    assert segs == W * H * SPP   # (one segment a sample: none hit anything)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
def test_camera_segment_is_the_last(gpu_lib, depth):
    """max_depth 1, 2: rem == 0 inside the merged tail, for trip lanes (1) and walk lanes (2)."""
    from rtclj import scenes
    _, segs = _check(scenes.cover(3), scenes.cover_camera(W, H), W, H, SPP, f"max_depth {depth}", depth=depth)
    assert W * H * SPP <= segs <= depth * W * H * SPP


@pytest.mark.gpu
def test_metal_cluster_with_fuzz_1(gpu_lib):
    """Metal with fuzz 1: many scattered rays point into the body and are absorbed, in the tail."""
    from rtclj import raytracing as R
    sc, cam = _cluster(R.RT_METAL, (0.7, 0.7, 0.9, 1.0))
    _check(sc, cam, W, H, 16, "metal cluster, fuzz 1")


@pytest.mark.gpu
def test_glass_cluster(gpu_lib):
    """Glass only (on the ground): the dielectric block serves trip lanes and walk lanes together."""
    from rtclj import raytracing as R
    sc, cam = _cluster(R.RT_DIELECTRIC, (0.0, 0.0, 0.0, 1.5))
    _check(sc, cam, W, H, 16, "glass cluster")


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 3, 17, 100])
def test_one_tile(gpu_lib, spp):
    """8 x 8: 64, 192 samples for 256 lanes (batches spent from the start), 1088 (a gate that seldom fills), 6400."""
    from rtclj import scenes
    _check(scenes.cover(3), scenes.cover_camera(8, 8), 8, 8, spp, f"8 x 8, {spp} spp")


@pytest.mark.gpu
def test_tiles_without_a_list_beside_listed_ones(gpu_lib):
    """cover(11) on 32 x 24: a tile spans so much of the field that its list
    passes the limit (the plain flow), while the tiles of sky and ground have
    one (the rotated flow).  The statistics build (variant 31) shows both: trips
    ran, and camera samples started outside them."""
    from rtclj import raytracing as R
    from rtclj import scenes
    from rtclj._lib import check, diag_lib
    sc, cam = scenes.cover(11), scenes.cover_camera(W, H)
    ref, _ = _check(sc, cam, W, H, SPP, "cover(11)")
    d = diag_lib()
    old = d.rt_set_variant(31)
    assert old >= 0
    try:
        check(d.rt_debug_stats((C.c_uint64 * 32)()))   # clear
        out = R.render(sc, cam, W, H, spp=SPP, max_depth=DEPTH, seed=5, n_devices=1, library=d)
        dbg = (C.c_uint64 * 32)()
        check(d.rt_debug_stats(dbg))
    finally:
        d.rt_set_variant(old)
    s = [int(x) for x in dbg]
    print(dict(calls=s[0], fresh_lanes=s[17], trips=s[27], trip_lanes=s[28]))
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), "variant 31"
    assert s[17] == W * H * SPP and s[27] > 0 and 0 < s[28] < s[17]


@pytest.mark.gpu
def test_partial_edge_tiles(gpu_lib):
    from rtclj import scenes
    _check(scenes.cover(3), scenes.cover_camera(20, 12), 20, 12, SPP, "20 x 12")


@pytest.mark.gpu
def test_sharded_launch(gpu_lib):
    """row_tile = 8, tile_first = 1, tile_step = 2: the odd 8-row bands of the frame."""
    import torch
    from rtclj import scenes
    from rtclj._lib import check, lib, rt_params
    sc, cam = scenes.cover(3), scenes.cover_camera(W, H)
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    try:
        p = rt_params(width=W, height=H, row_begin=0, row_end=H, spp=SPP, max_depth=DEPTH, seed=7, row_tile=8,
                      tile_first=1, tile_step=2)
        rows = lib.rt_rows_out(C.byref(p))
        assert rows == 8

        def go():
            out = torch.full((rows * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()), None))
            torch.cuda.synchronize()
            return out.cpu().numpy().reshape(rows, W, 3), tuple(cnt.cpu().tolist())
        _same(_render_all(go), "sharded launch")
    finally:
        lib.rt_scene_free(ds)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["RT_FLAG_REJECTION_SAMPLERS", "RT_FLAG_REALM"])
def test_flags(gpu_lib, flag):
    from rtclj import _lib, scenes
    _check(scenes.cover(3), scenes.cover_camera(W, H), W, H, SPP, flag, flags=getattr(_lib, flag))


def test_the_models_merged_tail_only_moves_the_shading(tmp_path):
    """tools/simt_sim.cpp on 20 tiles of C1 with the gated prelude, without and
    with TAIL=1: the same samples and segments, a lower cost per sample."""
    exe = tmp_path / "simt_sim"
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(ROOT / "include"), str(ROOT / "tools" / "simt_sim.cpp"),
                        str(ROOT / "raytracing-clj_amd" / "csrc" / "bvh.cpp"), f"-L{LIB}", "-lrtclj",
                        f"-Wl,-rpath,{LIB}", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    counts, cost = {}, {}
    for tail in ("0", "1"):
        env = dict(os.environ, PADT="1", PRE="2", INFL="2", NV="1", PREK="16", TAIL=tail)
        r = subprocess.run([str(exe), "20", "100"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        m = re.search(r"counts: samples (\d+) segments (\d+)", r.stdout)
        c = re.search(r"cost/sample\s+([0-9.]+)", r.stdout)
        assert m and c, r.stdout[-2000:]
        counts[tail], cost[tail] = (int(m.group(1)), int(m.group(2))), float(c.group(1))
        print(tail, counts[tail], cost[tail])
    assert counts["0"] == counts["1"] and counts["0"][0] == 20 * 64 * 100, counts
    assert cost["1"] < cost["0"], cost
