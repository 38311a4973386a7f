"""Progressive rendering on the device (include/rt.h, rt_accum): passes of a
frame added into an accumulator are, bit for bit, the frame one rt_launch of
the total spp gives -- for any pass sizes, launch shapes, kernel variants,
flags, order and streams -- and the accumulator's entries leave rt_launch as
it was.  rt_launch's own output is the bit-exact reference; the oracle's fp32
mirror (MODE_MIRROR32 | DIRECT) the independent one.  Every frame is resolved
into a NaN-filled buffer: an element the resolve skipped would stay NaN.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_MAIN = ROOT / "raytracing-clj_amd" / "lib" / "rt_main"
OCC_SHAPES = (("ref", 400, 225, 100), ("cover", 1200, 675, 100))


class Env:
    pass


def _occupancy(ds, w, h, spp):
    from rtclj._lib import check, lib, rt_params
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=50, seed=1)
    out4 = (C.c_int * 4)()
    check(lib.rt_launch_occupancy(ds, C.byref(p), out4))
    return tuple(out4)


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    from rtclj import scenes
    from rtclj._lib import check, lib
    e = Env()
    e.torch = torch
    e.sc = R.Scene.from_bodies(R.hittables)
    e.cover = scenes.cover(11)
    e.ds, e.ds_cover = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(e.sc.c), C.byref(e.ds)))
    check(lib.rt_scene_upload(0, C.byref(e.cover.c), C.byref(e.ds_cover)))
    # before any accumulating pass has run in this module
    e.occ_before = {name: _occupancy(e.ds if name == "ref" else e.ds_cover, w, h, spp)
                    for name, w, h, spp in OCC_SHAPES}
    yield e
    lib.rt_scene_free(e.ds)
    lib.rt_scene_free(e.ds_cover)


def _cam(w, h):
    from rtclj import raytracing as R
    return R.camera(w, h, **R.REFERENCE_CAMERA)


def _params(w, h, spp, begin=0, seed=9, flags=0, depth=50, **kw):
    from rtclj._lib import rt_params
    return rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=depth, seed=seed,
                     sample_begin=begin, flags=flags, **kw)


def _sptr(env, stream):
    s = stream or env.torch.cuda.current_stream()
    return s, C.c_void_p(s.cuda_stream)


def _shape(p):
    from rtclj._lib import lib
    return (lib.rt_rows_out(C.byref(p)), p.width, 3)


def _launch(env, cam, p, ds=None, counters=False):
    """rt_launch of p -> frame (and [segments, samples])."""
    from rtclj._lib import lib
    torch = env.torch
    shape = _shape(p)
    out = torch.full((int(np.prod(shape)),), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s, sp = _sptr(env, None)
    rc = lib.rt_launch(ds or env.ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()),
                       C.c_void_p(cnt.data_ptr()) if counters else None, sp)
    assert rc == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    frame = out.cpu().numpy().reshape(shape)
    assert not np.isnan(frame).any()
    return (frame, cnt.cpu().numpy().tolist()) if counters else frame


class Acc:
    """An rt_accum and the device buffers its resolves write."""

    def __init__(self, env, p, ds=None):
        from rtclj._lib import check, lib
        self.env, self.ds, self.shape = env, ds or env.ds, _shape(p)
        self.n = int(np.prod(self.shape))
        self.h = C.c_void_p()
        check(lib.rt_accum_create(self.ds, C.byref(p), C.byref(self.h)))
        self.cnt = env.torch.zeros(2, dtype=env.torch.int64, device="cuda")
        env.torch.cuda.synchronize()

    def add(self, cam, p, stream=None, counters=True):
        from rtclj._lib import lib
        rc = lib.rt_launch_accum(self.ds, C.byref(cam), C.byref(p), self.h,
                                 C.c_void_p(self.cnt.data_ptr()) if counters else None, _sptr(self.env, stream)[1])
        assert rc == 0, lib.rt_last_error()

    def passes(self, cam, p, sizes):
        """p's frame in passes of `sizes` samples, from p.sample_begin on."""
        from rtclj._lib import rt_params
        assert sum(sizes) == p.spp, (sizes, p.spp)
        q = rt_params.from_buffer_copy(p)
        for n in sizes:
            q.spp = n
            self.add(cam, q)
            q.sample_begin += n
        return self

    @property
    def samples(self):
        from rtclj._lib import lib
        return lib.rt_accum_samples(self.h)

    def counters(self):
        self.env.torch.cuda.synchronize()
        return self.cnt.cpu().numpy().tolist()

    def frame(self, flags=0):
        from rtclj._lib import lib
        torch = self.env.torch
        torch.cuda.synchronize()   # (passes on other streams have finished)
        out = torch.full((self.n,), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.rt_accum_resolve(self.h, flags, C.c_void_p(out.data_ptr()), _sptr(self.env, None)[1])
        assert rc == 0, lib.rt_last_error()
        torch.cuda.synchronize()
        f = out.cpu().numpy().reshape(self.shape)
        assert not np.isnan(f).any()
        return f

    def frame_u8(self, flags=0):
        from rtclj._lib import lib
        torch = self.env.torch
        torch.cuda.synchronize()
        out = torch.full((self.n + 5,), 0xa5, dtype=torch.uint8, device="cuda")   # 5 guard bytes behind
        rc = lib.rt_accum_resolve_u8(self.h, flags, C.c_void_p(out.data_ptr()), _sptr(self.env, None)[1])
        assert rc == 0, lib.rt_last_error()
        torch.cuda.synchronize()
        b = out.cpu().numpy()
        assert (b[self.n:] == 0xa5).all()
        return b[:self.n].reshape(self.shape)

    def read(self):
        from rtclj._lib import check, lib, u64ptr
        out = np.full(self.shape, 0xffffffffffffffff, np.uint64)
        check(lib.rt_accum_read(self.h, u64ptr(out), _sptr(self.env, None)[1]))
        return out

    def free(self):
        from rtclj._lib import lib
        lib.rt_accum_free(self.h)
        self.h = C.c_void_p()


def _mirror(env, w, h, spp, seed=9, realm=False, rejection=False):
    mode = (oracle.MODE_REALM32 if realm else oracle.MODE_MIRROR32) | (0 if rejection else oracle.DIRECT)
    cam = _cam(w, h)
    out, _, segs, smp = oracle.render(mode, env.sc.sphere.astype(np.float64), env.sc.kind,
                                      env.sc.mat.astype(np.float64), cam.as_list(), cam.defocus, w, h, spp, 50,
                                      seed=seed, nthreads=min(16, os.cpu_count() or 1))
    return out, [segs, smp]


# ---- 1: passes equal one launch ------------------------------------------------
@pytest.fixture(scope="module")
def small(env):
    """21 x 13 (ragged in both axes; 819 sums: the resolve's odd tail), seed
    9, depth 50, 8 spp: rt_launch's frame and counters, the mirror's."""
    from rtclj import raytracing as R
    w, h = 21, 13
    cam = _cam(w, h)
    p = _params(w, h, 8)
    frame, cnt = _launch(env, cam, p, counters=True)
    m, mcnt = _mirror(env, w, h, 8)
    assert np.array_equal(frame, m) and cnt == mcnt
    return dict(w=w, h=h, cam=cam, p=p, frame=frame, cnt=cnt, u8=R.write_color(frame))


@pytest.mark.parametrize("sizes", [(1, 2, 5), (4, 4), (8,)])
def test_passes_equal_one_launch(env, small, sizes):
    acc = Acc(env, small["p"])
    try:
        assert acc.samples == 0
        acc.passes(small["cam"], small["p"], sizes)
        assert acc.samples == 8
        assert np.array_equal(acc.frame(), small["frame"])
        assert np.array_equal(acc.frame_u8(), small["u8"])
        assert acc.counters() == small["cnt"]
    finally:
        acc.free()


# ---- 2: the compact image's wrap counting across passes ---------------------------
def test_compact_wraps_across_passes(env):
    w, h = 16, 8
    cam = _cam(w, h)
    assert _occupancy(env.ds, w, h, 300)[3] == 22 and _occupancy(env.ds, w, h, 255)[3] == 22
    # (a launch of at most 255 spp adds its u32 sums without counting wraps,
    # one of more counts them.  255 + 1 is 256 samples, not 300: it is held
    # against the 256-spp launch, and 255 + 1 + 44 against the 300-spp one.)
    for total, cases in ((300, ((200, 100), (255, 1, 44), (256, 44))), (256, ((255, 1),))):
        p = _params(w, h, total)
        want = _launch(env, cam, p)
        for sizes in cases:
            acc = Acc(env, p)
            try:
                assert np.array_equal(acc.passes(cam, p, sizes).frame(), want), sizes
            finally:
                acc.free()


# ---- 3: past the compact image's per-launch limit -----------------------------------
def test_passes_stay_on_the_compact_image_past_its_launch_limit(env):
    w, h = 8, 8
    cam = _cam(w, h)
    p = _params(w, h, 80000)
    assert _occupancy(env.ds, w, h, 40000)[3] == 22
    assert _occupancy(env.ds, w, h, 80000)[3] == 16
    want = _launch(env, cam, p)
    acc = Acc(env, p)
    try:
        got = acc.passes(cam, p, (40000, 40000)).frame()
        assert acc.samples == 80000
        assert np.array_equal(got, want)
    finally:
        acc.free()


# ---- 4: every shipped variant ------------------------------------------------------
@pytest.mark.parametrize("v", [0, 16, 18, 22, 24, 26, 12, 5])
def test_every_shipped_variant(env, v):
    from rtclj._lib import lib
    w, h = 24, 16
    cam = _cam(w, h)
    p = _params(w, h, 8)
    old = lib.rt_set_variant(v)
    assert old >= 0
    acc = None
    try:
        want = _launch(env, cam, p)
        acc = Acc(env, p)
        assert np.array_equal(acc.passes(cam, p, (3, 5)).frame(), want)
    finally:
        lib.rt_set_variant(old)
        if acc:
            acc.free()


# ---- 5: launch shapes --------------------------------------------------------------
@pytest.mark.parametrize("split", [None, 1, 4])
def test_sample_splits(env, monkeypatch, split):
    w, h = 40, 24
    cam = _cam(w, h)
    p = _params(w, h, 12)
    monkeypatch.delenv("RTCLJ_SPLIT", raising=False)
    want = _launch(env, cam, p)
    if split is not None:
        monkeypatch.setenv("RTCLJ_SPLIT", str(split))
    acc = Acc(env, p)
    try:
        assert np.array_equal(acc.passes(cam, p, (6, 6)).frame(), want)
    finally:
        acc.free()
        monkeypatch.delenv("RTCLJ_SPLIT", raising=False)
    assert np.array_equal(_launch(env, cam, p), want)


def test_interleaved_shard(env):
    w, h = 40, 24
    cam = _cam(w, h)
    p = _params(w, h, 12, row_tile=8, tile_first=1, tile_step=3)
    want = _launch(env, cam, p)
    assert want.shape == (8, w, 3)
    full = _launch(env, cam, _params(w, h, 12))
    assert np.array_equal(want, full[8:16])
    acc = Acc(env, p)
    try:
        assert np.array_equal(acc.passes(cam, p, (6, 6)).frame(), want)
    finally:
        acc.free()


def test_frame_of_whole_tiles_on_fresh_scenes(env):
    """768 x 448 (5,376 tiles: more than three rounds of workgroups, so
    rt_launch runs whole tiles and, as a fresh scene's first launch, shares
    their tails): passes 5 + 4 as a fresh scene's first launches equal it,
    and so does an rt_launch behind them on their scene and stream."""
    from rtclj._lib import check, lib
    w, h = 768, 448
    cam = _cam(w, h)
    p = _params(w, h, 9)
    fresh = [C.c_void_p(), C.c_void_p()]
    for d in fresh:
        check(lib.rt_scene_upload(0, C.byref(env.sc.c), C.byref(d)))
    acc = None
    try:
        want = _launch(env, cam, p, ds=fresh[0])
        acc = Acc(env, p, ds=fresh[1])
        assert np.array_equal(acc.passes(cam, p, (5, 4)).frame(), want)
        assert np.array_equal(_launch(env, cam, p, ds=fresh[1]), want)
    finally:
        if acc:
            acc.free()
        for d in fresh:
            lib.rt_scene_free(d)


# ---- 6: flags ----------------------------------------------------------------------
def test_realm_passes(env):
    from rtclj._lib import RT_FLAG_REALM
    w, h = 21, 13
    cam = _cam(w, h)
    p = _params(w, h, 7, flags=RT_FLAG_REALM)
    want = _launch(env, cam, p)
    assert np.array_equal(want, _mirror(env, w, h, 7, realm=True)[0])
    acc = Acc(env, p)
    try:
        acc.passes(cam, p, (3, 4))
        assert np.array_equal(acc.frame(RT_FLAG_REALM), want)
        # 7 is no power of two: the quotient is another frame
        assert not np.array_equal(acc.frame(0), want)
    finally:
        acc.free()


def test_rejection_sampler_passes(env):
    from rtclj._lib import RT_FLAG_REJECTION_SAMPLERS
    w, h = 21, 13
    cam = _cam(w, h)
    p = _params(w, h, 8, flags=RT_FLAG_REJECTION_SAMPLERS)
    want = _launch(env, cam, p)
    assert np.array_equal(want, _mirror(env, w, h, 8, rejection=True)[0])
    acc = Acc(env, p)
    try:
        acc.passes(cam, p, (4, 4))
        assert np.array_equal(acc.frame(0), want)
        assert np.array_equal(acc.frame(RT_FLAG_REJECTION_SAMPLERS), want)   # (the resolve reads realm only)
    finally:
        acc.free()


# ---- 7: streams and order ----------------------------------------------------------
def test_streams_and_order(env, small):
    torch = env.torch
    cam, w, h = small["cam"], small["w"], small["h"]
    lo, hi = _params(w, h, 4, begin=0), _params(w, h, 4, begin=4)
    acc = Acc(env, small["p"])
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        acc.add(cam, lo, stream=s1)
        acc.add(cam, hi, stream=s2)     # (both enqueued before either is waited for)
        assert np.array_equal(acc.frame(), small["frame"])
        assert acc.counters() == small["cnt"]
    finally:
        acc.free()
    acc = Acc(env, small["p"])
    try:
        acc.add(cam, hi)
        acc.add(cam, lo)
        assert np.array_equal(acc.frame(), small["frame"])
    finally:
        acc.free()


# ---- 8: resolve is non-destructive, clear works ---------------------------------------
def test_resolve_keeps_the_sums_and_clear_empties_them(env, small):
    from rtclj._lib import check, lib
    cam, w, h = small["cam"], small["w"], small["h"]
    acc = Acc(env, small["p"])
    try:
        acc.add(cam, _params(w, h, 3, begin=0))
        first = acc.frame()
        assert np.array_equal(first, _launch(env, cam, _params(w, h, 3)))
        assert np.array_equal(acc.frame(), first)
        assert np.array_equal(acc.frame_u8(), acc.frame_u8())
        acc.add(cam, _params(w, h, 5, begin=3))
        assert np.array_equal(acc.frame(), small["frame"])
        check(lib.rt_accum_clear(acc.h, _sptr(env, None)[1]))
        assert acc.samples == 0
        assert not acc.read().any()
        assert not acc.frame().any() and not acc.frame_u8().any()
        acc.passes(cam, small["p"], (8,))
        assert acc.samples == 8 and np.array_equal(acc.frame(), small["frame"])
    finally:
        acc.free()


# ---- 9: round trip through the host --------------------------------------------------
def test_sums_round_trip(env, small):
    from rtclj._lib import check, fptr, lib, u64ptr
    from rtclj.shard import combine_exact
    cam, w, h = small["cam"], small["w"], small["h"]
    a, b, c = (Acc(env, small["p"]) for _ in range(3))
    try:
        a.add(cam, _params(w, h, 3, begin=0))
        b.add(cam, _params(w, h, 5, begin=3))
        sa, sb = a.read(), b.read()
        assert sa.max() < 3 << 24 and sb.max() <= 5 << 24 and sa.any()
        for s, n in ((sa, 3), (sb, 5)):
            check(lib.rt_accum_add(c.h, u64ptr(s), n, _sptr(env, None)[1]))
        assert c.samples == 8
        dev = c.frame()
        assert np.array_equal(dev, small["frame"])
        assert np.array_equal(c.read(), sa + sb)
        host = np.full(dev.shape, np.nan, np.float32)
        tot = sa + sb
        check(lib.rt_resolve_sums(u64ptr(tot), tot.size, 8, 0, fptr(host)))
        assert np.array_equal(host, dev)
        assert np.array_equal(combine_exact([sa, sb], 8), dev)
    finally:
        for x in (a, b, c):
            x.free()


# ---- 10: errors ----------------------------------------------------------------------
def test_errors_leave_the_accumulator_usable(env, small):
    from rtclj._lib import lib, rt_params, u64ptr
    cam, w, h, p = small["cam"], small["w"], small["h"], small["p"]
    acc = Acc(env, p)
    sp = _sptr(env, None)[1]
    f = env.torch.zeros(acc.n, dtype=env.torch.float32, device="cuda")
    fp = C.c_void_p(f.data_ptr())
    zeros = np.zeros(acc.shape, np.uint64)

    def refused(rc):
        return rc == -1 and lib.rt_last_error() != b""
    try:
        # shapes
        for q in (_params(w + 1, h, 2), _params(w, h + 1, 2),
                  _params(w, h, 2, row_tile=4, tile_first=0, tile_step=2),
                  rt_params(width=w, height=h, row_begin=1, row_end=h, spp=2, max_depth=50, seed=9)):
            assert refused(lib.rt_launch_accum(env.ds, C.byref(cam), C.byref(q), acc.h, None, sp))
        bad = C.c_void_p()
        assert refused(lib.rt_accum_create(env.ds, C.byref(_params(0, h, 1)), C.byref(bad))) and not bad.value
        assert refused(lib.rt_accum_create(env.ds, C.byref(rt_params(width=4, height=4, row_begin=3, row_end=2)),
                                           C.byref(bad)))
        # another device's scene
        if lib.rt_device_count() > 1:
            other = C.c_void_p()
            assert lib.rt_scene_upload(1, C.byref(env.sc.c), C.byref(other)) == 0
            assert refused(lib.rt_launch_accum(other, C.byref(cam), C.byref(p), acc.h, None, None))
            assert b"device" in lib.rt_last_error()
            lib.rt_scene_free(other)
        # NULLs
        assert refused(lib.rt_launch_accum(None, C.byref(cam), C.byref(p), acc.h, None, sp))
        assert refused(lib.rt_launch_accum(env.ds, None, C.byref(p), acc.h, None, sp))
        assert refused(lib.rt_launch_accum(env.ds, C.byref(cam), None, acc.h, None, sp))
        assert refused(lib.rt_launch_accum(env.ds, C.byref(cam), C.byref(p), None, None, sp))
        assert refused(lib.rt_accum_create(None, C.byref(p), C.byref(bad)))
        assert refused(lib.rt_accum_create(env.ds, None, C.byref(bad)))
        assert refused(lib.rt_accum_create(env.ds, C.byref(p), None))
        assert refused(lib.rt_accum_resolve(acc.h, 0, None, sp)) and refused(lib.rt_accum_resolve(None, 0, fp, sp))
        assert refused(lib.rt_accum_resolve_u8(acc.h, 0, None, sp)) and refused(lib.rt_accum_resolve(acc.h, 64, fp, sp))
        assert refused(lib.rt_accum_read(acc.h, None, sp)) and refused(lib.rt_accum_read(None, u64ptr(zeros), sp))
        assert refused(lib.rt_accum_add(acc.h, None, 1, sp)) and refused(lib.rt_accum_add(None, u64ptr(zeros), 1, sp))
        assert refused(lib.rt_accum_add(acc.h, u64ptr(zeros), -1, sp))
        assert refused(lib.rt_accum_clear(None, sp))
        assert refused(lib.rt_launch_accum(env.ds, C.byref(cam), C.byref(_params(w, h, 2, flags=64)), acc.h, None, sp))
        assert lib.rt_last_error().startswith(b"rt_launch_accum: ")
        assert acc.samples == 0
        # the count's limit, 2^32 - 1, with no rendering
        assert lib.rt_accum_add(acc.h, u64ptr(zeros), 2 ** 32 - 3, sp) == 0
        assert acc.samples == 2 ** 32 - 3
        assert refused(lib.rt_launch_accum(env.ds, C.byref(cam), C.byref(_params(w, h, 3)), acc.h, None, sp))
        assert b"2^32" in lib.rt_last_error()
        assert refused(lib.rt_accum_add(acc.h, u64ptr(zeros), 3, sp))
        assert acc.samples == 2 ** 32 - 3 and not acc.read().any()
        assert lib.rt_accum_add(acc.h, u64ptr(zeros), 2, sp) == 0 and acc.samples == 2 ** 32 - 1
        assert not acc.frame().any()
        # ... and still usable
        assert lib.rt_accum_clear(acc.h, sp) == 0
        assert np.array_equal(acc.passes(cam, p, (2, 6)).frame(), small["frame"])
    finally:
        acc.free()


# ---- the Python host ---------------------------------------------------------------
def test_progressive_and_render_passes(env, small):
    from rtclj import raytracing as R
    torch = env.torch
    w, h = small["w"], small["h"]
    with R.Progressive(env.sc, small["cam"], w, h, seed=9) as pr:
        assert pr.samples == 0 and pr.shape == (h, w, 3)
        assert pr.add(3) == 3
        first = pr.frame()
        assert np.array_equal(first, _launch(env, small["cam"], _params(w, h, 3)))
        assert pr.add(5) == 8
        assert np.array_equal(pr.frame(), small["frame"])
        assert np.array_equal(pr.frame_u8(), small["u8"])
        d = torch.full((h * w * 3,), float("nan"), dtype=torch.float32, device="cuda")
        d8 = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pr.resolve_into(d.data_ptr())
        pr.resolve_into(d8.data_ptr(), u8=True)
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy().reshape(h, w, 3), small["frame"])
        assert np.array_equal(d8.cpu().numpy().reshape(h, w, 3), small["u8"])
        sums = pr.sums()
        pr.clear()
        assert pr.samples == 0 and not pr.frame().any()
        assert pr.add_sums(sums, 8) == 8 and np.array_equal(pr.frame(), small["frame"])
        pr.clear()
        pr.add(8)
        assert np.array_equal(pr.frame(), small["frame"])
    for k in (1, 3, 20):
        assert np.array_equal(R.render(env.sc, small["cam"], w, h, spp=8, seed=9, passes=k), small["frame"]), k
    assert np.array_equal(R.render(env.sc, small["cam"], w, h, spp=8, seed=9, passes=3, u8=True), small["u8"])
    assert np.array_equal(R.render(env.sc, small["cam"], w, h, spp=8, seed=9), small["frame"])


# ---- 12: rt_main --passes --------------------------------------------------------------
def test_rt_main_passes_writes_the_same_ppm(gpu_lib, tmp_path):
    assert RT_MAIN.exists(), "lib/rt_main is not built (make -C raytracing-clj_amd)"
    child = dict(os.environ)
    child.pop("RTCLJ_LIBRARY", None)
    base = ["16", "50", "--width", "64", "--gpus", "1", "--no-png"]
    for name, extra in (("plain.ppm", []), ("passes.ppm", ["--passes", "4"])):
        r = subprocess.run([str(RT_MAIN), *base, "--out", name, *extra], cwd=tmp_path, capture_output=True,
                           text=True, timeout=120, env=child)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    plain = (tmp_path / "plain.ppm").read_bytes()
    assert plain.startswith(b"P3\n64 36\n255\n")
    assert (tmp_path / "passes.ppm").read_bytes() == plain


# ---- 11: existing launches are untouched (after the tests above) -----------------------
def test_rt_launch_is_untouched_by_the_passes(env, small):
    """A split pass and an unsplit one on the scene and stream, then plain
    rt_launch es there: the mirror's frames (the stream's own split sums were
    not left dirty), and the occupancy the launches had before any pass."""
    cam, w, h = small["cam"], small["w"], small["h"]
    acc = Acc(env, small["p"])
    try:
        acc.passes(cam, small["p"], (7, 1))
        frame, cnt = _launch(env, cam, small["p"], counters=True)
        m, mcnt = _mirror(env, w, h, 8)
        assert np.array_equal(frame, m) and cnt == mcnt
        assert np.array_equal(_launch(env, cam, small["p"]), m)
        assert np.array_equal(acc.frame(), m)
    finally:
        acc.free()
    for name, ww, hh, spp in OCC_SHAPES:
        assert _occupancy(env.ds if name == "ref" else env.ds_cover, ww, hh, spp) == env.occ_before[name], name
    assert env.occ_before["ref"][3] == 22
