"""The per-tile body list (raytracing-clj_amd/csrc/tile_list.h):
variant 22 resolves every camera segment against the tile's list in a prelude
of the wave iteration instead of the big bodies' leaves and the tree walk;
variant 30 is 22 without the list, every segment through the walk.  The body test, the acceptance, the draws and their
order per path are the walk's, so a frame and both counters (segments,
samples) must be equal bit for bit between 22 and 30 in one process -- over the
launch shapes and flags the list has to work with, on tiles whose list
overflows (they keep the walk) and tiles with an empty one (the sky: their
paths never enter the walk).  One case is also held to the oracle's fp32
mirror (MODE_MIRROR32 | DIRECT).
"""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

WALK, LIST = 30, 22


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


def _render(sc, cam, w, h, spp, depth, seed=3, **kw):
    from rtclj import raytracing as R

    def go():
        st = {}
        out = R.render(sc, cam, w, h, spp=spp, max_depth=depth, seed=seed, n_devices=1, stats=st, **kw)
        return out, (st.get("segments"), st.get("samples"))
    return go


def _same(a, b, what=""):
    (fa, ca), (fb, cb) = a, b
    assert fa.shape == fb.shape and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), \
        f"{what}: {float((fa == fb).all(axis=-1).mean()):.4%} pixels bit-exact"
    assert ca == cb, (what, ca, cb)


@pytest.fixture(scope="module")
def cover(gpu_lib):
    from rtclj import scenes
    return scenes.cover(11)


def test_the_launch_runs_the_list_variant(gpu_lib, cover):
    """Either is launched where asked for; the list costs no register and no workgroup per CU."""
    from rtclj._lib import check, lib, rt_params
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(cover.c), C.byref(ds)))
    try:
        p = rt_params(width=160, height=90, row_begin=0, row_end=90, spp=8, max_depth=50, seed=1)
        occ = {}
        old = _variant(WALK)
        try:
            for v in (WALK, LIST):
                _variant(v)
                out4 = (C.c_int * 4)()
                check(lib.rt_launch_occupancy(ds, C.byref(p), out4))
                occ[v] = list(out4)
        finally:
            lib.rt_set_variant(old)
        print(occ)
        assert occ[WALK][3] == WALK and occ[LIST][3] == LIST, occ
        assert occ[WALK][0] == 7, occ              # seven workgroups per CU
        assert occ[LIST][0] == occ[WALK][0] and occ[LIST][1] <= occ[WALK][1], occ
    finally:
        lib.rt_scene_free(ds)


def test_cover_frame_and_the_mirror(gpu_lib, cover):
    from rtclj import scenes
    w, h, spp, depth = 160, 90, 8, 50
    cam = scenes.cover_camera(w, h)
    walk, lst = _both(_render(cover, cam, w, h, spp, depth, seed=5))
    _same(walk, lst, "cover(11)")
    want, _, segs, _ = oracle.render(oracle.MODE_MIRROR32 | oracle.DIRECT, cover.sphere.astype(np.float64), cover.kind,
                                     cover.mat.astype(np.float64), cam.as_list(), cam.defocus, w, h, spp, depth, seed=5)
    assert np.array_equal(lst[0], want) and lst[1][0] == segs, "the list path against the fp32 mirror"


def test_reference_scene(gpu_lib):
    """Five bodies: no big-body leaf, a tree of a few leaves."""
    from rtclj import raytracing as R
    sc = R.Scene.from_bodies(R.hittables)
    w, h = 160, 90
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    _same(*_both(_render(sc, cam, w, h, 8, 50)), "reference scene")


def _cluster_scene():
    """A ground, 64 bodies of r = 0.02 in a cube 0.2 wide at the look-at point
    (under four pixels across at 160 x 90: the four tiles around the image's
    centre see all 64, more than a list holds -- they keep the walk), and a
    ring of larger bodies elsewhere (tiles with short lists, and the sky's empty ones)."""
    from rtclj import raytracing as R
    sph, kind, mat = [(0.0, -1000.0, 0.0, 1000.0)], [R.RT_LAMBERTIAN], [(0.5, 0.5, 0.5, 0.0)]
    for i in range(64):
        x, y, z = i % 4, (i // 4) % 4, i // 16
        sph.append((-0.075 + 0.05 * x, 0.425 + 0.05 * y, -0.075 + 0.05 * z, 0.02))
        kind.append((R.RT_LAMBERTIAN, R.RT_METAL, R.RT_DIELECTRIC)[i % 3])
        mat.append((0.8, 0.3, 0.3, 0.0) if i % 3 == 0 else (0.7, 0.7, 0.9, 0.1) if i % 3 == 1 else (0.0, 0.0, 0.0, 1.5))
    for i in range(12):
        a = 2.0 * np.pi * i / 12
        sph.append((2.5 * np.cos(a), 0.3, 2.5 * np.sin(a), 0.3))
        kind.append(R.RT_METAL if i % 2 else R.RT_LAMBERTIAN)
        mat.append((0.6, 0.8, 0.4, 0.05))
    return R.Scene(np.array(sph, np.float32), np.array(kind, np.int32), np.array(mat, np.float32))


def test_cluster_overflows_some_lists(gpu_lib):
    from rtclj import raytracing as R
    sc = _cluster_scene()
    w, h = 160, 90
    cam = R.camera(w, h, 20.0, (13.0, 2.0, 3.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 0.6, 13.4)
    _same(*_both(_render(sc, cam, w, h, 8, 50)), "cluster of 64")


def test_camera_inside_a_glass_sphere(gpu_lib):
    from rtclj import raytracing as R
    base = R.Scene.from_bodies(R.hittables)
    sph = np.vstack([base.sphere, np.array([[-2.0, 2.0, 1.0, 0.75]], np.float32)])
    kind = np.concatenate([base.kind, np.array([R.RT_DIELECTRIC], np.int32)])
    mat = np.vstack([base.mat, np.array([[0.0, 0.0, 0.0, 1.5]], np.float32)])
    sc = R.Scene(sph, kind, mat)
    w, h = 96, 54
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    _same(*_both(_render(sc, cam, w, h, 8, 50)), "camera inside glass")


@pytest.mark.parametrize("angle", [0.0, 30.0])
def test_defocus(gpu_lib, cover, angle):
    from rtclj import raytracing as R
    w, h = 64, 36
    cam = R.camera(w, h, 20.0, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), angle, 10.0)
    _same(*_both(_render(cover, cam, w, h, 6, 50)), f"defocus {angle}")


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_shallow_depths(gpu_lib, cover, depth):
    from rtclj import scenes
    w, h = 64, 36
    _same(*_both(_render(cover, scenes.cover_camera(w, h), w, h, 6, depth)), f"depth {depth}")


def test_one_row_tiles_interleaved(gpu_lib, cover):
    """row_tile = 1, tile_step = 2: a pool's eight rows lie two image rows apart."""
    import torch
    from rtclj import scenes
    from rtclj._lib import check, lib, rt_params
    w, h = 72, 40
    cam = scenes.cover_camera(w, h)
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(cover.c), C.byref(ds)))
    try:
        p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=6, max_depth=50, seed=7, row_tile=1, tile_first=1,
                      tile_step=2)
        rows = lib.rt_rows_out(C.byref(p))
        assert rows == h // 2

        def go():
            out = torch.full((rows * w * 3,), float("nan"), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()), None))
            torch.cuda.synchronize()
            return out.cpu().numpy().reshape(rows, w, 3), tuple(cnt.cpu().tolist())
        _same(*_both(go), "interleaved 1-row tiles")
    finally:
        lib.rt_scene_free(ds)


def test_sample_split(gpu_lib, cover):
    """A launch of six tiles: every tile's samples split over several workgroups."""
    from rtclj import scenes
    w, h = 24, 16
    _same(*_both(_render(cover, scenes.cover_camera(w, h), w, h, 96, 50)), "sample split")


def test_whole_tiles_many_claims(gpu_lib, cover):
    """5,400 whole tiles of 1,536 samples: every wave claims batch after batch,
    from its workgroup's counter and -- the launch's last tiles, shared with
    helper workgroups -- from the tile's word, in the prelude's refill and in
    the walk's by turns."""
    from rtclj import scenes
    w, h = 800, 432
    _same(*_both(_render(cover, scenes.cover_camera(w, h), w, h, 24, 50)), "whole tiles")


def test_accumulated_passes(gpu_lib, cover):
    """rt_launch_accum passes and the resolve (Progressive)."""
    from rtclj import raytracing as R
    from rtclj import scenes
    w, h = 64, 36
    cam = scenes.cover_camera(w, h)

    def go():
        return R.render(cover, cam, w, h, spp=7, max_depth=50, seed=3, n_devices=1, passes=2), None
    walk, lst = _both(go)
    _same(walk, lst, "accumulated passes")
    _same(lst, _render(cover, cam, w, h, 7, 50)()[:1] + (None,), "passes against one launch")


def test_adaptive_steps(gpu_lib, cover):
    from rtclj import raytracing as R
    from rtclj import scenes
    w, h = 64, 36
    cam = scenes.cover_camera(w, h)

    def go():
        st = {}
        out = R.render(cover, cam, w, h, max_depth=50, seed=3, n_devices=1, stats=st,
                       adaptive=dict(tol_q16=2048, step=2, min_spp=4, max_spp=16))
        return out, (st["samples"], st["tile_spp"].tobytes())
    _same(*_both(go), "adaptive steps")


@pytest.mark.parametrize("flag", ["RT_FLAG_REALM", "RT_FLAG_REJECTION_SAMPLERS"])
def test_flags(gpu_lib, cover, flag):
    from rtclj import _lib, scenes
    w, h = 64, 36
    _same(*_both(_render(cover, scenes.cover_camera(w, h), w, h, 6, 50, flags=getattr(_lib, flag))), flag)
