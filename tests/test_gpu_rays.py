"""Ray queries on the device (include/rt.h: rt_launch_rays, rt_launch_occluded):
every word of every record and every occlusion byte is the host's
(rt_rays_host, rt_occluded_host) -- for the float64 test's rays, the pinhole
rays, the inactive and the guarded sets, on the reference scene, the 484-body
cover scene, a 1025-body scene whose tree leaves LDS and the edge scenes
rt_launch_ids is held to, under the default selector, the scan (5) and the tree
in global memory (12); for ray counts around a wave, a workgroup and the
grid-stride loop's partial last block; after rt_scene_update; in stream order.
Every output buffer is pre-filled and ends in canaries that must stay.
"""
import ctypes as C

import numpy as np
import pytest

import edge_scenes as E
import ray_sets as RS
from test_rays_host import EDGE_NAMES, camera_of

pytestmark = pytest.mark.gpu

CANARY_WORD = 0x5a5a5a5a
CANARY_BYTE = 0xa5
PAD = 64                      # records / bytes behind each output
VARIANTS = (0, 5, 12)


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    e = Env()
    e.torch, e.R, e.lib = torch, R, gpu_lib.lib
    return e


def to_device(env, a):
    t = env.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    env.torch.cuda.synchronize()
    return t


def out_buffers(env, n):
    torch = env.torch
    hits = torch.full(((n + PAD) * 8,), CANARY_WORD, dtype=torch.int32, device="cuda")
    occ = torch.full((n + PAD,), CANARY_BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return hits, occ


def read_outputs(env, hits, occ, n):
    """-> (records (n,), bytes (n,)); the canaries behind them checked."""
    from rtclj._lib import RAY_HIT_DTYPE
    h = hits.cpu().numpy().view(np.uint32)
    o = occ.cpu().numpy()
    assert (h[8 * n:] == CANARY_WORD).all() and (o[n:] == CANARY_BYTE).all(), "written behind the output"
    return h[:8 * n].view(np.dtype(RAY_HIT_DTYPE)), o[:n]


def device_query(env, ds, rays, last=None, stream=None):
    """Both launches for `rays` on scene ds (a DeviceScene) -> (records, bytes)."""
    rays = np.ascontiguousarray(rays).reshape(-1)
    n = len(rays)
    d_rays = to_device(env, rays)
    d_last = to_device(env, np.ascontiguousarray(last, np.int32)) if last is not None else None
    hits, occ = out_buffers(env, n)
    lp = d_last.data_ptr() if d_last is not None else None
    st = stream.cuda_stream if stream is not None else None
    ds.intersect_into(d_rays.data_ptr(), n, hits.data_ptr(), lp, st)
    ds.occluded_into(d_rays.data_ptr(), n, occ.data_ptr(), lp, st)
    env.torch.cuda.synchronize()
    return read_outputs(env, hits, occ, n)


def check_equals_host(env, ds, sc, rays, last=None, what=""):
    rays = np.ascontiguousarray(rays).reshape(-1)
    want = env.R.rays_host(sc, rays, last)
    want_occ = env.R.occluded_host(sc, rays, last)
    assert np.array_equal(want_occ, want["body"] >= 0)
    for variant in VARIANTS:
        old = env.lib.rt_set_variant(variant)
        try:
            got, occ = device_query(env, ds, rays, last)
        finally:
            env.lib.rt_set_variant(old)
        diff = (RS.words(got) != RS.words(want)).any(axis=1)
        assert not diff.any(), (what, variant, int(diff.sum()), got[diff][:2], want[diff][:2])
        assert np.array_equal(occ, want_occ.astype(np.uint8)), (what, variant, int((occ != want_occ).sum()))
    return want


# ---- 1. device == host, every word ------------------------------------------------------------
@pytest.mark.parametrize("name", ("reference", "cover", "large"))
def test_records_equal_host(env, name):
    R = env.R
    sc = RS.scene(name)
    out4 = (C.c_int * 4)()
    with R.DeviceScene(sc) as ds:
        assert env.lib.rt_rays_occupancy(ds.handle, out4) == 0
        assert out4[3] == (1 if name == "large" else 0) and out4[0] >= 1 and out4[1] > 0   # large: the tree leaves LDS
        q = RS.query_rays(name)
        want = check_equals_host(env, ds, sc, q, what="query")
        assert (want["body"] >= 0).sum() > 1000 and (want["body"] < 0).sum() > 400
        # the same rays, every fifth guarded by the body it hits (the ray starts again from outside it)
        last = np.where(np.arange(len(q)) % 5 == 0, want["body"], -1).astype(np.int32)
        check_equals_host(env, ds, sc, q, last, what="query, guarded")
        cam = camera_of("reference" if name == "reference" else "cover", 64, 40)
        check_equals_host(env, ds, sc, R.pinhole_rays(cam, 64, 40), what="pinhole")
        names, inactive = RS.inactive_rays()
        got = check_equals_host(env, ds, sc, inactive, what="inactive")
        assert np.array_equal(RS.words(got), RS.words(RS.none_records(len(names))))
        rays, glast = RS.guarded_rays()
        check_equals_host(env, ds, sc, rays, glast, what="guarded")
        check_equals_host(env, ds, sc, rays, np.full(len(rays), len(sc) + 3, np.int32), what="last >= n")
        for variant in VARIANTS:     # the occupancy entry follows the selector
            old = env.lib.rt_set_variant(variant)
            try:
                assert env.lib.rt_rays_occupancy(ds.handle, out4) == 0
            finally:
                env.lib.rt_set_variant(old)
            assert out4[3] == {5: 2, 12: 1}.get(variant, out4[3])


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_records_of_edge_scenes(env, name):
    sc, cam, _ = E.case(name)
    rays = env.R.pinhole_rays(cam, E.W, E.H).reshape(-1)
    with env.R.DeviceScene(sc) as ds:
        want = check_equals_host(env, ds, sc, rays, what=name)
        # every ray guarded by some body of the scene, the never-hit ones among them
        last = (np.arange(len(rays)) % (len(sc) + 1) - 1).astype(np.int32)
        check_equals_host(env, ds, sc, rays, last, what=name + ", guarded")
    assert np.array_equal(want["body"].reshape(E.H, E.W), env.R.ids_host(sc, cam, E.W, E.H))


# ---- 2. ray counts ----------------------------------------------------------------------------
def test_ray_counts(env):
    """1, 63, 64, 65, 257 rays, and more than 256 x the grid's workgroups with a
    partial last block: the grid-stride loop's second trip."""
    R, torch = env.R, env.torch
    sc = RS.scene("reference")
    base = RS.query_rays("reference")
    out4 = (C.c_int * 4)()
    with R.DeviceScene(sc) as ds:
        assert env.lib.rt_rays_occupancy(ds.handle, out4) == 0 and out4[3] == 0
        grid = out4[0] * torch.cuda.get_device_properties(0).multi_processor_count
        big = 256 * grid + 256 + 77
        assert big % 256 != 0 and big > 256 * grid
        for n in (1, 63, 64, 65, 257, big):
            rays = np.resize(base, n)
            want = R.rays_host(sc, rays)
            got, occ = device_query(env, ds, rays)
            assert np.array_equal(RS.words(got), RS.words(want)), n
            assert np.array_equal(occ, (want["body"] >= 0).astype(np.uint8)), n
        old = env.lib.rt_set_variant(12)      # the tree in global memory: the same loop
        try:
            got, occ = device_query(env, ds, rays)
        finally:
            env.lib.rt_set_variant(old)
        assert np.array_equal(RS.words(got), RS.words(want)) and np.array_equal(occ, want["body"] >= 0)


# ---- 3. the pinhole ids ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("reference", "cover"))
def test_pinhole_bodies_equal_the_id_pass(env, name):
    R, torch = env.R, env.torch
    w, h = 160, 90
    sc, cam = RS.scene(name), camera_of(name, w, h)
    with R.DeviceScene(sc) as ds:
        ids = torch.full((w * h,), 0x7fffffff, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert env.lib.rt_launch_ids(ds.handle, C.byref(cam), w, h, 0, C.c_void_p(ids.data_ptr()), None) == 0
        got, occ = device_query(env, ds, R.pinhole_rays(cam, w, h))
        assert np.array_equal(got["body"], ids.cpu().numpy())
        assert np.array_equal(occ, got["body"] >= 0)


# ---- 4. after a refit ---------------------------------------------------------------------------
def test_queries_follow_rt_scene_update(env):
    R = env.R
    sc = RS.scene("cover")
    rays = RS.query_rays("cover")
    rng = np.random.default_rng(5)
    sph = sc.sphere.copy()
    sph[1:, :3] += rng.uniform(-0.15, 0.15, (len(sc) - 1, 3)).astype(np.float32)
    moved = R.Scene(sph, sc.kind, sc.mat)
    stale = R.rays_host(sc, rays)
    with R.DeviceScene(sc) as ds:
        check_equals_host(env, ds, sc, rays, what="before")
        ds.update(moved)
        want = check_equals_host(env, ds, moved, rays, what="after")
    assert (RS.words(want) != RS.words(stale)).any(axis=1).sum() > 100
    assert (want["body"] != stale["body"]).any()


# ---- 5. stream order ------------------------------------------------------------------------------
def test_stream_order(env):
    """Upload, two launches and the copies back on one non-default stream, no
    host synchronisation in between."""
    R, torch = env.R, env.torch
    from rtclj._lib import RAY_HIT_DTYPE
    sc = RS.scene("cover")
    rays = np.ascontiguousarray(RS.query_rays("cover"))
    n = len(rays)
    want = R.rays_host(sc, rays)
    host_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).pin_memory()
    host_hits = torch.zeros(n * 32, dtype=torch.uint8).pin_memory()
    host_occ = torch.full((n,), 7, dtype=torch.uint8).pin_memory()
    with R.DeviceScene(sc) as ds:
        d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        hits, occ = out_buffers(env, n)
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_rays.copy_(host_rays, non_blocking=True)
            ds.intersect_into(d_rays.data_ptr(), n, hits.data_ptr(), None, stream.cuda_stream)
            ds.occluded_into(d_rays.data_ptr(), n, occ.data_ptr(), None, stream.cuda_stream)
            host_hits.copy_(hits[:n * 8].view(torch.uint8), non_blocking=True)
            host_occ.copy_(occ[:n], non_blocking=True)
        stream.synchronize()
        got = host_hits.numpy().view(np.dtype(RAY_HIT_DTYPE))
        assert np.array_equal(RS.words(got), RS.words(want))
        assert np.array_equal(host_occ.numpy(), (want["body"] >= 0).astype(np.uint8))
        torch.cuda.synchronize()
        read_outputs(env, hits, occ, n)


# ---- 6. errors -----------------------------------------------------------------------------------
def test_argument_errors_write_nothing(env):
    lib, R = env.lib, env.R
    sc = RS.scene("reference")
    rays = np.ascontiguousarray(RS.query_rays("reference")[:16])
    d_rays = to_device(env, rays)
    hits, occ = out_buffers(env, 16)
    rp, hp, op = C.c_void_p(d_rays.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(occ.data_ptr())
    with R.DeviceScene(sc) as ds:
        h = ds.handle
        for fn, out in ((lib.rt_launch_rays, hp), (lib.rt_launch_occluded, op)):
            for args, word in (((None, rp, None, 16, out, None), b"NULL"), ((h, None, None, 16, out, None), b"NULL"),
                               ((h, rp, None, 16, None, None), b"NULL"), ((h, rp, None, 1 << 31, out, None), b"2^31"),
                               ((h, C.c_void_p(d_rays.data_ptr() + 4), None, 4, out, None), b"aligned")):
                assert fn(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
            assert fn(h, rp, None, 0, out, None) == 0          # n = 0: fine, nothing enqueued
            assert fn(h, None, None, 0, None, None) == 0       # ... and needs no arrays
            assert fn(None, rp, None, 0, out, None) == -1      # ... but a scene
        assert lib.rt_launch_rays(h, rp, None, 4, C.c_void_p(hits.data_ptr() + 8), None) == -1
        assert lib.rt_rays_occupancy(h, None) == -1 and lib.rt_rays_occupancy(None, (C.c_int * 4)()) == -1
        env.torch.cuda.synchronize()
        assert (hits.cpu().numpy().view(np.uint32) == CANARY_WORD).all() and (occ.cpu().numpy() == CANARY_BYTE).all()
