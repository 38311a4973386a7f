"""Specular-chain features on the device (include/rt.h: rt_launch_feat_chain):
rt_feat_read after a chain pass equals rt_feat_chain_host's records summed, bit
for bit, for every shape, selector, sampler, stream and scene below; with no
bounce, and on rough bodies with any, it is rt_launch_feat; on smooth bodies it
is the path rt_launch traces under RT_FLAG_REALM; the counters; the closed
mirror; the kinds an rt_feat remembers; the Python hosts and rt_main --chain;
and tests/test_chain_host.py's quality check on the device's own frames.  All
inputs are valid and every frame is small: nothing here can fault.
"""
import ctypes as C
import functools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edge_scenes as E
import feat_oracle as FO
import test_chain_host as T
from test_denoise_host import bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_MAIN = ROOT / "raytracing-clj_amd" / "lib" / "rt_main"
REJECTION = 8          # RT_FLAG_REJECTION_SAMPLERS
REALM = 2              # RT_FLAG_REALM
VARIANTS = (0, 12, 5)  # the default, the tree in global memory, the linear scan
SHARD = dict(row_tile=8, tile_first=1, tile_step=2)


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    from rtclj import scenes
    from rtclj._lib import lib
    e = Env()
    e.torch, e.R, e.lib, e.scenes = torch, R, lib, scenes
    return e


def _params(w, h, spp, begin=0, seed=9, flags=0, **kw):
    from rtclj._lib import rt_params
    return rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=1, seed=seed, sample_begin=begin,
                     flags=flags, **kw)


def _opts(o):
    from rtclj._lib import rt_feat_chain_opts
    return None if o is None else rt_feat_chain_opts(max_bounces=o.get("max_bounces", 8), fuzz_max=o.get("fuzz_max", 0.0))


class Dev:
    """An uploaded scene, an rt_feat of p's shape and two counters."""

    def __init__(self, env, sc, p):
        from rtclj._lib import check
        self.env, self.lib = env, env.lib
        self.ds, self.h = C.c_void_p(), C.c_void_p()
        check(self.lib.rt_scene_upload(0, C.byref(sc.c), C.byref(self.ds)))
        check(self.lib.rt_feat_create(self.ds, C.byref(p), C.byref(self.h)))
        self.rows, self.w = self.lib.rt_rows_out(C.byref(p)), p.width
        self.cnt = env.torch.zeros(2, dtype=env.torch.int64, device="cuda")
        env.torch.cuda.synchronize()

    def _stream(self, stream):
        return C.c_void_p(stream.cuda_stream) if stream is not None else None

    def chain(self, cam, p, opts, stream=None, counters=True):
        o = _opts(opts)
        return self.lib.rt_launch_feat_chain(self.ds, C.byref(cam), C.byref(p), None if o is None else C.byref(o), self.h,
                                             C.c_void_p(self.cnt.data_ptr()) if counters else None, self._stream(stream))

    def first_hit(self, cam, p, stream=None):
        return self.lib.rt_launch_feat(self.ds, C.byref(cam), C.byref(p), self.h, None, self._stream(stream))

    def clear(self):
        assert self.lib.rt_feat_clear(self.h, None) == 0
        self.cnt.zero_()
        self.env.torch.cuda.synchronize()

    def read(self):
        from rtclj._lib import check, fptr, i64ptr, u32ptr
        self.env.torch.cuda.synchronize()
        sums = np.full((self.rows, self.w, 6), -1, np.int64)
        hits = np.full((self.rows, self.w), 0xffffffff, np.uint32)
        depth = np.full((self.rows, self.w), np.nan, np.float32)
        check(self.lib.rt_feat_read(self.h, i64ptr(sums), u32ptr(hits), fptr(depth), None))
        assert not np.isnan(depth).any()
        return dict(sums=sums, hits=hits, depth=depth)

    def counters(self):
        self.env.torch.cuda.synchronize()
        return self.cnt.cpu().numpy().tolist()

    def free(self):
        self.lib.rt_feat_free(self.h)
        self.lib.rt_scene_free(self.ds)


def _with_variant(lib, v, fn):
    old = lib.rt_set_variant(v)
    assert old >= 0
    try:
        return fn()
    finally:
        lib.rt_set_variant(old)


def shard_rows(h, row_tile, first, step):
    return [r for t in range(first, -(-h // row_tile), step) for r in range(t * row_tile, min(h, (t + 1) * row_tile))]


def expected(sc, rays, opts):
    """The host's records of `rays` (rows, width, spp, 6) summed, and the segments they took."""
    rec = T.host(sc, rays, **(opts or {}))
    return T.records_sum(rec), int((rec["bounces"].astype(np.int64) + 1).sum()), rec


def check_scene(env, sc, cam, w, h, spp, seed, opts, begin=0, flags=0, variants=VARIANTS, shard=None, rays=None):
    """One chain pass under each selector == the host's sums and counters; the
    same with max_bounces = 0 == rt_launch_feat's read-back."""
    if rays is None:
        rays = FO.mirror(sc, cam, w, h, spp, seed, begin, rejection=bool(flags & REJECTION), want_rays=True)["rays"]
    if shard:
        rays = rays[shard_rows(h, shard["row_tile"], shard["tile_first"], shard["tile_step"])]
    want, segs, rec = expected(sc, rays, opts)
    p = _params(w, h, spp, begin, seed, flags, **(shard or {}))
    d = Dev(env, sc, p)
    try:
        assert (d.rows, d.w) == rays.shape[:2]
        for v in variants:
            def one():
                d.clear()
                assert d.chain(cam, p, opts) == 0, env.lib.rt_last_error()
                got = d.read()
                assert T.same_raw(got, want), (v, int((got["sums"] != want["sums"]).any(axis=-1).sum()),
                                               int((got["hits"] != want["hits"]).sum()))
                assert d.counters() == [segs, rays.shape[0] * rays.shape[1] * spp], v
                d.clear()
                assert d.chain(cam, p, dict(opts or {}, max_bounces=0)) == 0
                zero = d.read()
                d.clear()
                assert d.first_hit(cam, p) == 0
                assert T.same_raw(zero, d.read()), v
            _with_variant(env.lib, v, one)
    finally:
        d.free()
    return rec


# ---- 1, 2, 4: the device equals the host; no bounce equals rt_launch_feat; the counters ---------
MIXED_OPTS = dict(max_bounces=8, fuzz_max=0.5)


@pytest.mark.parametrize("w,h,spp,shard", ((1, 1, 1, None), (9, 7, 5, None), (33, 40, 4, SHARD)))
@pytest.mark.parametrize("rejection", (False, True))
@pytest.mark.parametrize("defocus", (True, False))
def test_mixed_scene(env, w, h, spp, shard, rejection, defocus):
    R = env.R
    cam = R.camera(w, h, **dict(R.REFERENCE_CAMERA, vfov=40.0, defocus_angle=10.0 if defocus else 0.0))
    rec = check_scene(env, T.mixed_scene(), cam, w, h, spp, 9, MIXED_OPTS, flags=REJECTION if rejection else 0, shard=shard)
    if w > 1:
        assert rec["bounces"].max() >= 2 and (rec["body"] < 0).any() and (rec["body"] >= 0).any()


def test_fuzz_max_decides_what_is_smooth(env):
    """The fuzz-0.3 metal is followed at fuzz_max 0.5 and ends the chain at 0."""
    R = env.R
    sc, cam = T.mixed_scene(), R.camera(33, 40, **dict(R.REFERENCE_CAMERA, vfov=40.0))
    rays = FO.mirror(sc, cam, 33, 40, 2, 9, want_rays=True)["rays"]
    a, b = T.host(sc, rays, fuzz_max=0.5), T.host(sc, rays, fuzz_max=0.0)
    assert ((b["body"] == 4) & (b["bounces"] == 0)).any() and not ((a["body"] == 4) & (a["bounces"] == 0)).any()
    check_scene(env, sc, cam, 33, 40, 2, 9, dict(fuzz_max=0.0), variants=(0,), rays=rays)
    check_scene(env, sc, cam, 33, 40, 2, 9, None, variants=(0,), rays=rays)      # NULL options: {8, 0}


@pytest.mark.parametrize("name", T.EDGE_NAMES)
def test_edge_scenes(env, name):
    sc, cam, m, spp, seed, begin = T.detail(name)
    check_scene(env, sc, cam, E.W, E.H, spp, seed, None, begin=begin, rays=m["rays"])


def test_above_1024_bodies(env):
    sc, cam = env.scenes.cover(17), env.scenes.cover_camera(24, 16)
    assert len(sc) > 1024
    rec = check_scene(env, sc, cam, 24, 16, 2, 3, None)
    assert rec["bounces"].max() >= 1


def test_rough_bodies_only(env):
    """Lambertian bodies only: any max_bounces is rt_launch_feat."""
    R = env.R
    s = T.mixed_scene()
    sc = R.Scene(s.sphere, np.zeros(len(s), np.int32), s.mat)
    cam = R.camera(33, 40, **dict(R.REFERENCE_CAMERA, vfov=40.0))
    p = _params(33, 40, 4)
    d = Dev(env, sc, p)
    try:
        assert d.first_hit(cam, p) == 0
        want = d.read()
        for mb in (1, 8, 64):
            d.clear()
            assert d.chain(cam, p, dict(max_bounces=mb, fuzz_max=3.0)) == 0
            assert T.same_raw(d.read(), want), mb
            assert d.counters() == [33 * 40 * 4] * 2
    finally:
        d.free()


def test_streams_and_passes(env):
    """On the NULL stream and a created one; two passes over consecutive sample
    ranges against one; two passes issued from two streams."""
    R, torch = env.R, env.torch
    sc, w, h = T.mixed_scene(), 33, 40
    cam = R.camera(w, h, **dict(R.REFERENCE_CAMERA, vfov=40.0))
    rays = FO.mirror(sc, cam, w, h, 6, 9, want_rays=True)["rays"]
    want, segs, _ = expected(sc, rays, MIXED_OPTS)
    whole, a, b = _params(w, h, 6), _params(w, h, 4), _params(w, h, 2, begin=4)
    d = Dev(env, sc, whole)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        for plan in (((whole, None),), ((whole, s1),), ((a, None), (b, None)), ((a, s1), (b, s2)), ((b, s2), (a, s1))):
            d.clear()
            for p, st in plan:
                assert d.chain(cam, p, MIXED_OPTS, stream=st) == 0
            assert env.lib.rt_feat_samples(d.h) == 6
            assert T.same_raw(d.read(), want), [id(st) for _, st in plan]
            assert d.counters() == [segs, w * h * 6]
    finally:
        d.free()


# ---- 3. property 2 on the device ---------------------------------------------------------------
def test_smooth_bodies_give_the_realm_path(env):
    sc, cam, rec, sky = T.property2()
    assert sky.mean() >= 0.5
    p = _params(T.P2_W, T.P2_H, 1, seed=T.P2_SEED, flags=REALM)
    p.max_depth = T.P2_BOUNCES + 2
    d = Dev(env, sc, p)
    torch = env.torch
    try:
        out = torch.full((T.P2_H * T.P2_W * 3,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert env.lib.rt_launch(d.ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), None, None) == 0
        assert d.chain(cam, p, dict(max_bounces=T.P2_BOUNCES)) == 0
        raw = d.read()
        img = out.cpu().numpy().reshape(T.P2_H, T.P2_W, 3)
    finally:
        d.free()
    assert T.same_raw(raw, T.records_sum(rec))
    got = FO.resolve_np(raw["sums"], raw["hits"], raw["depth"], 1)[..., 0:3]
    assert not np.isnan(img).any()
    assert np.array_equal(bits(got[sky]), bits(img[sky])), int((got[sky] != img[sky]).any(axis=-1).sum())


# ---- 5. the closed mirror ------------------------------------------------------------------------
def test_closed_mirror(env):
    sc, cam = T.closed_mirror()
    p = _params(8, 8, 4, seed=1)
    d = Dev(env, sc, p)
    try:
        for v in VARIANTS:
            def one():
                d.clear()
                assert d.chain(cam, p, dict(max_bounces=64)) == 0
                raw = d.read()
                assert (raw["hits"] == 4).all() and np.isfinite(raw["depth"]).all()
                assert d.counters() == [65 * 8 * 8 * 4, 8 * 8 * 4]
                return raw
            raw = _with_variant(env.lib, v, one)
            rays = FO.mirror(sc, cam, 8, 8, 4, 1, want_rays=True)["rays"]
            assert T.same_raw(raw, expected(sc, rays, dict(max_bounces=64))[0]), v
    finally:
        d.free()


# ---- 6. kinds, options, clear; the argument errors -----------------------------------------------
def test_kind_mixing_and_clear(env):
    from rtclj._lib import fptr, i64ptr, u32ptr
    R, lib = env.R, env.lib
    sc, w, h = T.mixed_scene(), 9, 7
    cam = R.camera(w, h, **dict(R.REFERENCE_CAMERA, vfov=40.0))
    p = _params(w, h, 2)
    d = Dev(env, sc, p)

    def refused(rc, word):
        return rc == -1 and word in lib.rt_last_error()

    try:
        assert d.chain(cam, p, dict(max_bounces=4)) == 0
        held = d.read()
        assert refused(d.first_hit(cam, p), b"hold chain passes")
        assert refused(d.chain(cam, p, dict(max_bounces=5)), b"other options")
        assert refused(d.chain(cam, p, dict(max_bounces=4, fuzz_max=0.1)), b"other options")
        assert refused(d.chain(cam, p, None), b"other options")      # NULL: {8, 0}
        for bad in (dict(max_bounces=-1), dict(max_bounces=65), dict(fuzz_max=-1.0), dict(fuzz_max=float("nan"))):
            assert refused(d.chain(cam, p, bad), b"rt_launch_feat_chain: ")
        for q in (_params(w + 1, h, 2), _params(w, h, -1), _params(w, h, 2, flags=64)):
            assert refused(d.chain(cam, q, dict(max_bounces=4)), b"rt_launch_feat_chain: ")
        assert refused(lib.rt_launch_feat_chain(None, C.byref(cam), C.byref(p), None, d.h, None, None), b"NULL")
        assert lib.rt_feat_samples(d.h) == 2 and T.same_raw(d.read(), held)
        # rt_feat_add keeps the kind
        assert lib.rt_feat_add(d.h, i64ptr(held["sums"]), u32ptr(held["hits"]), fptr(held["depth"]), 2, None) == 0
        assert refused(d.first_hit(cam, p), b"hold chain passes")
        assert d.chain(cam, _params(w, h, 2, begin=4), dict(max_bounces=4)) == 0 and lib.rt_feat_samples(d.h) == 6
        # a pass of no samples checks and changes nothing; REALM and STREAMED are inert
        assert d.chain(cam, _params(w, h, 0), dict(max_bounces=4)) == 0 and lib.rt_feat_samples(d.h) == 6
        d.clear()
        assert d.first_hit(cam, p) == 0
        first = d.read()
        assert refused(d.chain(cam, p, dict(max_bounces=4)), b"hold first-hit passes")
        assert T.same_raw(d.read(), first)
        d.clear()
        assert d.chain(cam, _params(w, h, 2, flags=REALM | 4), dict(max_bounces=4)) == 0
        assert T.same_raw(d.read(), held)
        out4 = (C.c_int * 4)()
        assert lib.rt_feat_chain_occupancy(d.ds, out4) == 0 and out4[0] >= 1 and out4[3] in (0, 1, 2)
    finally:
        d.free()


# ---- 7. render_denoised and render_upscaled ---------------------------------------------------------
PW, PH = 160, 90


def test_render_denoised_and_upscaled(env):
    R = env.R
    sc, cam = T.reference_scene(), T.ref_camera(PW, PH)
    den, mean, feat = R.render_denoised(sc, cam, PW, PH, spp=8, seed=3, chain=8)
    with R.Progressive(sc, cam, PW, PH, seed=3) as a0, R.Progressive(sc, cam, PW, PH, seed=3, sample_begin=4) as a1, \
            R.Features(sc, cam, PW, PH, seed=3, chain=8) as ft, R.Features(sc, cam, PW, PH, seed=3) as f1:
        a0.add(4), a1.add(4), ft.add(8), f1.add(8)
        h0, h1, chained, first = a0.frame(), a1.frame(), ft.frame(), f1.frame()
    assert np.array_equal(bits(feat), bits(chained)) and not np.array_equal(bits(chained), bits(first))
    rays = FO.mirror(sc, cam, PW, PH, 8, 3, want_rays=True)["rays"]
    raw = T.records_sum(T.host(sc, rays))
    assert np.array_equal(bits(feat), bits(FO.resolve_np(raw["sums"], raw["hits"], raw["depth"], 8)))
    assert np.array_equal(bits(mean), bits(np.float32(0.5) * (h0 + h1)))
    assert np.array_equal(bits(den), bits(R.denoise_host(h0, h1, chained)))
    plain = R.render_denoised(sc, cam, PW, PH, spp=8, seed=3)
    assert np.array_equal(bits(plain[2]), bits(first)) and not np.array_equal(bits(plain[0]), bits(den))
    # the render scale: both feature frames are chain frames
    cw, ch = R.coarse_size(PW, PH, 2)
    ccam = R.camera_coarsen(cam, 2)
    st = R.render_upscaled(sc, cam, PW, PH, spp=8, scale=2, seed=3, chain=8, stages=True)
    with R.Features(sc, ccam, cw, ch, seed=3, chain=8) as fc:
        fc.add(8)
        coarse = fc.frame()
    uden, up0, up1, ufeat, c0, c1, cfeat = st
    assert np.array_equal(bits(ufeat), bits(chained)) and np.array_equal(bits(cfeat), bits(coarse))
    w0, w1 = R.upsample_host(c0, c1, coarse, chained, scale=2)
    assert np.array_equal(bits(up0), bits(w0)) and np.array_equal(bits(up1), bits(w1))
    assert np.array_equal(bits(uden), bits(R.denoise_host(w0, w1, chained)))


# ---- 8. render_animation ---------------------------------------------------------------------------
def test_render_animation(env):
    """Three frames: the temporal stages are a run without `chain`, bit for bit;
    the denoised frames are rt_denoise_host over the run's own chain features."""
    from test_motion_host import rising
    R = env.R
    cams = []
    for f in range(3):
        ang = np.radians(0.4) * f
        lf = (-2.0 * np.cos(ang) + 1.0 * np.sin(ang), 2.0, 2.0 * np.sin(ang) + 1.0 * np.cos(ang))
        cams.append(R.camera(PW, PH, **{**R.REFERENCE_CAMERA, "look_from": lf}))
    scs = [R.Scene.from_bodies(rising(f, 3)) for f in range(3)]
    plain = list(R.render_animation(scs, cams, PW, PH, spp=4, seed=5, stages=True))
    chained = list(R.render_animation(scs, cams, PW, PH, spp=4, seed=5, stages=True, chain=8))
    assert len(plain) == len(chained) == 3
    differ = 0
    for f, (a, b) in enumerate(zip(plain, chained)):
        assert len(a) == 7 and len(b) == 8
        for x, y in zip(a[1:], b[1:7]):
            assert np.array_equal(bits(x), bits(y)), f      # halves, first-hit features, history, ids
        cf = b[7]
        with R.Features(scs[f], cams[f], PW, PH, seed=5, sample_begin=4 * f, chain=8) as ft:
            ft.add(4)
            assert np.array_equal(bits(cf), bits(ft.frame())), f
        assert np.array_equal(bits(b[0]), bits(R.denoise_host(b[4], b[5], cf))), f
        differ += int((bits(a[0]) != bits(b[0])).any(axis=-1).sum())
    assert differ > 100
    # with a render scale: the upsampler is guided by chain features too
    for f, st in enumerate(R.render_animation(scs[:2], cams[:2], PW, PH, spp=4, seed=5, stages=True, chain=8, scale=2)):
        den, h0, h1, feat, acc0, acc1, ids, c0, c1, fc, cf = st
        u0, u1 = R.upsample_host(c0, c1, fc, cf, scale=2)
        assert np.array_equal(bits(h0), bits(u0)) and np.array_equal(bits(h1), bits(u1)), f
        assert np.array_equal(bits(den), bits(R.denoise_host(acc0, acc1, cf))), f
        assert np.array_equal(bits(feat), bits(plain[f][3])), f


# ---- 10. quality on the device's own frames -----------------------------------------------------------
class DeviceFrames:
    """test_chain_host's frame source on the device: rt_launch_accum,
    rt_launch_feat and rt_launch_feat_chain."""

    def __init__(self, env):
        self.R = env.R

    def render(self, sc, cam, spp, seed, begin=0):
        with self.R.Progressive(sc, cam, T.QW, T.QH, seed=seed, sample_begin=begin) as a:
            a.add(spp)
            return a.frame()

    def features(self, sc, cam, spp, seed, chain):
        with self.R.Features(sc, cam, T.QW, T.QH, seed=seed, chain=8 if chain else None) as ft:
            ft.add(spp)
            return ft.frame()


@pytest.mark.parametrize("which", ("cover_3", "reference"))
def test_quality_on_the_device(env, which):
    """tests/test_chain_host.py's test 7 with the device's frames, under the same thresholds."""
    T.check_quality(which, T.quality_table(which, DeviceFrames(env)))


# ---- 9. rt_main --chain ------------------------------------------------------------------------------
def test_rt_main_chain(env, tmp_path):
    R = env.R
    assert RT_MAIN.exists(), "lib/rt_main is not built (make -C raytracing-clj_amd)"
    env.torch.cuda.synchronize()
    child = dict(os.environ)
    child.pop("RTCLJ_LIBRARY", None)
    r = subprocess.run([str(RT_MAIN), "8", "50", "--width", str(PW), "--gpus", "1", "--no-png", "--seed", "3",
                        "--denoise", "ch", "--chain", "8"], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                       env=child)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    den, _, _ = R.render_denoised(T.reference_scene(), T.ref_camera(PW, PH), PW, PH, spp=8, seed=3, chain=8)
    assert np.array_equal(R.read_ppm(tmp_path / "ch.denoised.ppm"), R.write_color(den))
    for bad in (["--chain", "8"], ["--denoise", "bad", "--chain", "65"]):
        r = subprocess.run([str(RT_MAIN), "8", "50", "--width", str(PW), "--gpus", "1", "--no-png", *bad], cwd=tmp_path,
                           capture_output=True, text=True, timeout=120, env=child)
        assert r.returncode == 2 and "--chain" in r.stderr, (bad, r.returncode, r.stderr)
    assert not (tmp_path / "bad.denoised.ppm").exists()
