"""Adaptive sampling on the device (include/rt.h, rt_adapt): tiles whose two
sample halves agree stop being traced, and because the halves are exact
integer sums the per-tile sample counts and the frame are a pure function of
scene, camera, seed, flags and options -- held here bit for bit.

The expected counts come from the oracle alone: 64 one-sample frames of its
fp32 mirror (each exactly an integer sum: a 1-spp frame is
RN(float(sum)) * 2^-24 / 1 with sum <= 2^24) pushed through the rule restated
in Python ints (tests/test_adapt_host.py's adapt_rule).  The frame's reference
is rt_launch at spp = the tile's count.  Every frame is resolved into a
NaN-filled buffer.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from test_adapt_host import adapt_rule

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_MAIN = ROOT / "raytracing-clj_amd" / "lib" / "rt_main"
W, H = 60, 36                      # ragged right (4 px) and bottom (4 rows) tiles; 8 x 5 tiles
OPTS = dict(step_spp=8, min_spp=16, max_spp=64, tol_q16=4096)
OCC_SHAPES = (("ref", 400, 225, 100),)


class Env:
    pass


def _cam(w, h):
    from rtclj import raytracing as R
    return R.camera(w, h, **R.REFERENCE_CAMERA)


def _params(w, h, spp=0, begin=0, seed=9, flags=0, depth=50, **kw):
    from rtclj._lib import rt_params
    return rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=depth, seed=seed,
                     sample_begin=begin, flags=flags, **kw)


def _shape(p):
    from rtclj._lib import lib
    return (lib.rt_rows_out(C.byref(p)), p.width, 3)


def _occupancy(ds, w, h, spp):
    from rtclj._lib import check, lib, rt_params
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=50, seed=1)
    out4 = (C.c_int * 4)()
    check(lib.rt_launch_occupancy(ds, C.byref(p), out4))
    return tuple(out4)


def _sptr(env, stream):
    s = stream or env.torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _launch(env, cam, p, ds=None):
    from rtclj._lib import lib
    torch = env.torch
    shape = _shape(p)
    out = torch.full((int(np.prod(shape)),), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.rt_launch(ds or env.ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), None, _sptr(env, None))
    assert rc == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    frame = out.cpu().numpy().reshape(shape)
    assert not np.isnan(frame).any()
    return frame


def _one_spp_sums(sc, cam, w, h, n, seed=9, realm=False, rejection=False):
    """n one-sample mirror frames as integers (uint64 (h, w, 3) each)."""
    mode = (oracle.MODE_REALM32 if realm else oracle.MODE_MIRROR32) | (0 if rejection else oracle.DIRECT)
    ones = []
    for k in range(n):
        f = oracle.render(mode, sc.sphere.astype(np.float64), sc.kind, sc.mat.astype(np.float64), cam.as_list(),
                          cam.defocus, w, h, 1, 50, seed=seed, sample_begin=k,
                          nthreads=min(16, os.cpu_count() or 1))[0].astype(np.float64) * 2.0 ** 24
        assert np.array_equal(f, np.floor(f)) and f.min() >= 0 and f.max() <= 2 ** 24   # exact integers
        ones.append(f.astype(np.uint64))
    return ones


def simulate(ones, step_spp, min_spp, max_spp, tol_q16):
    """The sampler in Python ints over per-sample integer frames: (counts
    (gy, gx), H0, H1)."""
    rows, width = ones[0].shape[:2]
    gy, gx = (rows + 7) // 8, (width + 7) // 8
    h = [np.zeros_like(ones[0]), np.zeros_like(ones[0])]
    counts = np.zeros((gy, gx), np.uint32)
    active = np.ones((gy, gx), bool)
    k = 0
    while active.any():
        px = np.repeat(np.repeat(active, 8, 0), 8, 1)[:rows, :width]
        add = sum(ones[k * step_spp:(k + 1) * step_spp])
        h[k & 1][px] += add[px]
        k += 1
        counts[active] = k * step_spp
        if k % 2 == 0 and k * step_spp >= min_spp:
            active &= ~adapt_rule(h[0], h[1], tol_q16)
            if k * step_spp >= max_spp:
                active[...] = False
    return counts, h[0], h[1]


class Ad:
    """An rt_adapt and the device buffers its counters and resolves use."""

    def __init__(self, env, p, opts=OPTS, ds=None):
        from rtclj._lib import check, lib, rt_adapt_opts
        self.env, self.ds, self.p, self.shape = env, ds or env.ds, p, _shape(p)
        self.n = int(np.prod(self.shape))
        self.tiles = ((self.shape[0] + 7) // 8, (self.shape[1] + 7) // 8)
        self.h = C.c_void_p()
        self.opts = rt_adapt_opts(**opts)
        check(lib.rt_adapt_create(self.ds, C.byref(p), C.byref(self.opts), C.byref(self.h)))
        self.cnt = env.torch.zeros(2, dtype=env.torch.int64, device="cuda")
        env.torch.cuda.synchronize()

    def step(self, cam, p=None, stream=None):
        from rtclj._lib import lib
        return lib.rt_adapt_step(self.ds, C.byref(cam), C.byref(p or self.p), self.h, C.c_void_p(self.cnt.data_ptr()),
                                 _sptr(self.env, stream))

    def run(self, cam, p=None, stream=None):
        from rtclj._lib import lib
        steps = 0
        while True:
            rc = self.step(cam, p, stream)
            assert rc >= 0, lib.rt_last_error()
            if rc == 0:
                return steps
            steps += 1
            assert steps <= 1000

    @property
    def samples(self):
        from rtclj._lib import lib
        return lib.rt_adapt_samples(self.h)

    @property
    def active(self):
        from rtclj._lib import lib
        return lib.rt_adapt_active(self.h)

    def counters(self):
        self.env.torch.cuda.synchronize()
        return self.cnt.cpu().numpy().tolist()

    def counts(self, stream=None):
        from rtclj._lib import check, lib, u32ptr
        out = np.full(self.tiles, 0xffffffff, np.uint32)
        check(lib.rt_adapt_counts(self.h, u32ptr(out), _sptr(self.env, stream)))
        return out

    def read(self, stream=None):
        from rtclj._lib import check, lib, u64ptr
        h0 = np.full(self.shape, 0xffffffffffffffff, np.uint64)
        h1 = h0.copy()
        check(lib.rt_adapt_read(self.h, u64ptr(h0), u64ptr(h1), _sptr(self.env, stream)))
        return h0, h1

    def frame(self, flags=0):
        from rtclj._lib import lib
        torch = self.env.torch
        torch.cuda.synchronize()
        out = torch.full((self.n,), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.rt_adapt_resolve(self.h, flags, C.c_void_p(out.data_ptr()), _sptr(self.env, None))
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
        rc = lib.rt_adapt_resolve_u8(self.h, flags, C.c_void_p(out.data_ptr()), _sptr(self.env, None))
        assert rc == 0, lib.rt_last_error()
        torch.cuda.synchronize()
        b = out.cpu().numpy()
        assert (b[self.n:] == 0xa5).all()
        return b[:self.n].reshape(self.shape)

    def free(self):
        from rtclj._lib import lib
        lib.rt_adapt_free(self.h)
        self.h = C.c_void_p()


def _px(counts, rows, width):
    """Per-pixel view of per-tile values."""
    return np.repeat(np.repeat(counts, 8, 0), 8, 1)[:rows, :width]


def _valid_px(rows, width):
    gy, gx = (rows + 7) // 8, (width + 7) // 8
    return np.array([[min(8, rows - 8 * ty) * min(8, width - 8 * tx) for tx in range(gx)] for ty in range(gy)])


def _frame_per_count(env, cam, counts, flags=0, w=W, h=H, ds=None, seed=9, cache=None):
    """rt_launch's frames at each distinct count, stitched by tile."""
    want = np.full((h, w, 3), np.nan, np.float32)
    px = _px(counts, h, w)
    for c in np.unique(counts):
        key = (int(c), flags)
        if cache is None or key not in cache:
            f = _launch(env, cam, _params(w, h, int(c), flags=flags, seed=seed), ds=ds)
            if cache is not None:
                cache[key] = f
        else:
            f = cache[key]
        want[px == c] = f[px == c]
    assert not np.isnan(want).any()
    return want


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
    e.occ_before = {name: _occupancy(e.ds, w, h, spp) for name, w, h, spp in OCC_SHAPES}
    e.launches = {}   # (spp, flags) -> rt_launch's W x H frame
    yield e
    lib.rt_scene_free(e.ds)
    lib.rt_scene_free(e.ds_cover)


@pytest.fixture(scope="module")
def fx(env):
    """The oracle's samples, its counts and halves, and one adaptive run."""
    cam = _cam(W, H)
    ones = _one_spp_sums(env.sc, cam, W, H, OPTS["max_spp"])
    counts, h0, h1 = simulate(ones, **OPTS)
    values, n = np.unique(counts, return_counts=True)
    print("oracle counts:", dict(zip(values.tolist(), n.tolist())))
    # the oracle's counts alone, before anything is compared
    assert len(values) >= 3
    assert (counts == OPTS["min_spp"]).sum() >= 4
    assert (counts == OPTS["max_spp"]).sum() >= 4
    p = _params(W, H)
    ad = Ad(env, p)
    steps = ad.run(cam)
    d = dict(cam=cam, p=p, ones=ones, counts=counts, h0=h0, h1=h1, steps=steps, got_counts=ad.counts(),
             got_halves=ad.read(), frame=ad.frame(), u8=ad.frame_u8(), counters=ad.counters(), samples=ad.samples,
             active=ad.active)
    ad.free()
    return d


# ---- 1: counts -------------------------------------------------------------------------
def test_counts_are_the_oracles(env, fx):
    from rtclj._lib import check, lib, u8ptr, u64ptr
    assert np.array_equal(fx["got_counts"], fx["counts"]), (fx["got_counts"], fx["counts"])
    assert fx["active"] == 0 and fx["steps"] == OPTS["max_spp"] // OPTS["step_spp"]
    # the device's decisions against rt_adapt_eval_host on the halves read back
    # after every tested step: a tile that stopped there converged, one that
    # went on did not (tiles stopped earlier keep their halves: still converged)
    ad = Ad(env, fx["p"])
    try:
        final = fx["counts"]
        for k in range(1, fx["steps"] + 1):
            assert ad.step(fx["cam"]) > 0
            c = k * OPTS["step_spp"]
            if k % 2 or c < OPTS["min_spp"]:
                continue
            h0, h1 = ad.read()
            conv = np.full(final.shape, 0xa5, np.uint8)
            check(lib.rt_adapt_eval_host(u64ptr(h0), u64ptr(h1), W, H, OPTS["tol_q16"], u8ptr(conv)))
            assert np.array_equal(conv.astype(bool), adapt_rule(h0, h1, OPTS["tol_q16"]))
            if c < OPTS["max_spp"]:
                assert conv[final == c].all() and not conv[final > c].any(), c
            assert conv[final < c].all()
            now = ad.counts()
            assert np.array_equal(now, np.minimum(final, c)), c
        assert ad.step(fx["cam"]) == 0
    finally:
        ad.free()


# ---- 2: frame --------------------------------------------------------------------------
def test_frame_is_rt_launch_at_each_tiles_count(env, fx):
    from rtclj import raytracing as R
    from rtclj._lib import check, fptr, lib, u32ptr, u64ptr
    want = _frame_per_count(env, fx["cam"], fx["counts"], cache=env.launches)
    assert np.array_equal(fx["frame"], want)
    assert np.array_equal(fx["u8"], R.write_color(fx["frame"]))
    # the halves: the even and the odd steps' mirror sums
    assert np.array_equal(fx["got_halves"][0], fx["h0"]) and np.array_equal(fx["got_halves"][1], fx["h1"])
    # and the host conversion gives the device's frame
    host = np.full(want.shape, np.nan, np.float32)
    h0, h1 = fx["got_halves"]
    check(lib.rt_adapt_resolve_host(u64ptr(h0), u64ptr(h1), u32ptr(fx["got_counts"]), W, H, 0, fptr(host)))
    assert np.array_equal(host, want)


# ---- 3: analytic ends ------------------------------------------------------------------
def test_tolerance_one_stops_at_min_spp(env, fx):
    ad = Ad(env, fx["p"], {**OPTS, "tol_q16": 65536})
    try:
        assert ad.run(fx["cam"]) == OPTS["min_spp"] // OPTS["step_spp"]
        assert (ad.counts() == OPTS["min_spp"]).all()
        assert np.array_equal(ad.frame(), _launch(env, fx["cam"], _params(W, H, OPTS["min_spp"])))
    finally:
        ad.free()


def test_tolerance_zero_stops_identical_halves_only(env, fx):
    want_counts, h0, h1 = simulate(fx["ones"], **{**OPTS, "tol_q16": 0})
    ad = Ad(env, fx["p"], {**OPTS, "tol_q16": 0})
    try:
        ad.run(fx["cam"])
        counts = ad.counts()
        assert np.array_equal(counts, want_counts)
        # a tile stops early only where the oracle's halves are identical there
        early = counts < OPTS["max_spp"]
        assert np.array_equal(h0[_px(early, H, W)], h1[_px(early, H, W)])
        print("tol 0: tiles stopped early:", int(early.sum()))
        frame = ad.frame()
        full = _launch(env, fx["cam"], _params(W, H, OPTS["max_spp"]))
        if not early.any():
            assert np.array_equal(frame, full)
        assert np.array_equal(frame, _frame_per_count(env, fx["cam"], counts, cache=env.launches))
        assert np.array_equal(frame[_px(~early, H, W)], full[_px(~early, H, W)])
    finally:
        ad.free()


# ---- 4: independence -------------------------------------------------------------------
@pytest.mark.parametrize("v", [16, 22, 12, 5])
def test_kernel_variants(env, fx, v):
    from rtclj._lib import lib
    old = lib.rt_set_variant(v)
    assert old >= 0
    ad = None
    try:
        ad = Ad(env, fx["p"])
        ad.run(fx["cam"])
        assert np.array_equal(ad.counts(), fx["counts"])
        assert np.array_equal(ad.frame(), fx["frame"])
    finally:
        lib.rt_set_variant(old)
        if ad:
            ad.free()


def test_streamed_flag_other_stream_and_clear(env, fx):
    from rtclj._lib import RT_FLAG_STREAMED, check, lib
    torch = env.torch
    ad = Ad(env, fx["p"])
    try:
        ad.run(fx["cam"], _params(W, H, flags=RT_FLAG_STREAMED))
        assert np.array_equal(ad.counts(), fx["counts"]) and np.array_equal(ad.frame(), fx["frame"])
        # cleared: step 0 again, on another stream
        s = torch.cuda.Stream()
        check(lib.rt_adapt_clear(ad.h, _sptr(env, s)))
        assert ad.samples == 0 and ad.active == ad.tiles[0] * ad.tiles[1]
        assert not ad.counts(s).any() and not ad.read(s)[0].any() and not ad.read(s)[1].any()
        ad.run(fx["cam"], stream=s)
        s.synchronize()
        assert np.array_equal(ad.counts(s), fx["counts"])
        assert np.array_equal(ad.frame(), fx["frame"]) and np.array_equal(ad.frame_u8(), fx["u8"])
        assert ad.samples == fx["samples"]
    finally:
        ad.free()


def test_interleaved_shard(env, fx):
    p = _params(W, H, row_tile=8, tile_first=1, tile_step=2)    # rows 8..15 and 24..31
    ad = Ad(env, p)
    try:
        assert ad.shape == (16, W, 3)
        ad.run(fx["cam"], p)
        assert np.array_equal(ad.counts(), fx["counts"][[1, 3]])
        assert np.array_equal(ad.frame(), np.concatenate([fx["frame"][8:16], fx["frame"][24:32]]))
    finally:
        ad.free()


# ---- 5: flags and another scene --------------------------------------------------------
@pytest.mark.parametrize("which", ["realm", "rejection"])
def test_flag_variants_against_their_mirrors(env, fx, which):
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    flags = RT_FLAG_REALM if which == "realm" else RT_FLAG_REJECTION_SAMPLERS
    ones = _one_spp_sums(env.sc, fx["cam"], W, H, OPTS["max_spp"], realm=which == "realm",
                         rejection=which == "rejection")
    counts, h0, h1 = simulate(ones, **OPTS)
    p = _params(W, H, flags=flags)
    ad = Ad(env, p)
    try:
        ad.run(fx["cam"], p)
        assert np.array_equal(ad.counts(), counts)
        g0, g1 = ad.read()
        assert np.array_equal(g0, h0) and np.array_equal(g1, h1)
        frame = ad.frame(flags)
        assert np.array_equal(frame, _frame_per_count(env, fx["cam"], counts, flags=flags))
        if which == "realm" and (counts == 48).any():   # 48 is no power of two: the quotient differs
            assert not np.array_equal(ad.frame(0), frame)
    finally:
        ad.free()


def test_cover_scene(env):
    from rtclj import scenes
    from rtclj._lib import check, lib, u8ptr, u64ptr
    w, h = 64, 40
    cam = scenes.cover_camera(w, h)
    p = _params(w, h, seed=2)
    ad = Ad(env, p, ds=env.ds_cover)
    try:
        ad.run(cam)
        counts = ad.counts()
        print("cover counts:", dict(zip(*[a.tolist() for a in np.unique(counts, return_counts=True)])))
        assert ((counts % 16 == 0) & (counts >= 16) & (counts <= 64)).all()
        assert np.array_equal(ad.frame(), _frame_per_count(env, cam, counts, w=w, h=h, ds=env.ds_cover, seed=2))
        h0, h1 = ad.read()
        conv = np.zeros(counts.shape, np.uint8)
        check(lib.rt_adapt_eval_host(u64ptr(h0), u64ptr(h1), w, h, OPTS["tol_q16"], u8ptr(conv)))
        assert conv[counts < 64].all()
    finally:
        ad.free()


# ---- 6: counters -----------------------------------------------------------------------
def test_counters_and_samples(env, fx):
    want = int((fx["counts"].astype(np.int64) * _valid_px(H, W)).sum())
    assert fx["counters"][1] == want and fx["samples"] == want
    assert want < W * H * OPTS["max_spp"]
    ad = Ad(env, fx["p"])
    try:
        ad.run(fx["cam"])
        before = ad.counters()
        assert before == fx["counters"]     # segments too: the same samples
        assert ad.step(fx["cam"]) == 0 and ad.step(fx["cam"]) == 0
        assert ad.counters() == before and ad.samples == want and ad.active == 0
        assert np.array_equal(ad.counts(), fx["counts"]) and np.array_equal(ad.frame(), fx["frame"])
    finally:
        ad.free()


# ---- 7: errors -------------------------------------------------------------------------
def test_errors_leave_the_state_unchanged(env, fx):
    from rtclj._lib import lib, rt_adapt_opts
    ad = Ad(env, fx["p"])
    cam = fx["cam"]

    def refused(rc):
        return rc == -1 and lib.rt_last_error() != b""
    try:
        for _ in range(3):
            assert ad.step(cam) > 0
        state = (ad.samples, ad.active, ad.counts().copy(), ad.counters())
        for q in (_params(W + 1, H), _params(W, H + 1), _params(W, H, row_tile=4, tile_first=0, tile_step=2)):
            assert refused(ad.step(cam, q))
        old = lib.rt_set_variant(28)
        assert old >= 0
        try:
            assert refused(ad.step(cam)) and b"8 x 8" in lib.rt_last_error()
        finally:
            lib.rt_set_variant(old)
        assert refused(lib.rt_adapt_step(None, C.byref(cam), C.byref(fx["p"]), ad.h, None, None))
        assert refused(lib.rt_adapt_step(env.ds, C.byref(cam), C.byref(_params(W, H, flags=64)), ad.h, None, None))
        assert refused(lib.rt_adapt_resolve(ad.h, 0, None, None)) and refused(lib.rt_adapt_resolve(ad.h, 64, None, None))
        bad = C.c_void_p()
        o = rt_adapt_opts(**{**OPTS, "min_spp": 24})
        assert refused(lib.rt_adapt_create(env.ds, C.byref(fx["p"]), C.byref(o), C.byref(bad))) and not bad.value
        assert refused(lib.rt_adapt_create(env.ds, C.byref(_params(0, H)), C.byref(ad.opts), C.byref(bad)))
        now = (ad.samples, ad.active, ad.counts(), ad.counters())
        assert now[0] == state[0] and now[1] == state[1] and np.array_equal(now[2], state[2]) and now[3] == state[3]
        ad.run(cam)
        assert np.array_equal(ad.counts(), fx["counts"]) and np.array_equal(ad.frame(), fx["frame"])
        assert ad.counters() == fx["counters"]
    finally:
        ad.free()


# ---- 9: the hosts ----------------------------------------------------------------------
def test_python_hosts(env, fx):
    from rtclj import raytracing as R
    kw = dict(tol_q16=OPTS["tol_q16"], step=OPTS["step_spp"], min_spp=OPTS["min_spp"], max_spp=OPTS["max_spp"])
    with R.Adaptive(env.sc, fx["cam"], W, H, seed=9, **kw) as ad:
        assert ad.shape == (H, W, 3) and ad.tiles == (5, 8) and ad.samples_traced == 0
        assert ad.step() == 40
        assert ad.run() == fx["steps"] - 1
        assert np.array_equal(ad.counts(), fx["counts"])
        assert np.array_equal(ad.frame(), fx["frame"]) and np.array_equal(ad.frame_u8(), fx["u8"])
        h0, h1 = ad.halves()
        assert np.array_equal(h0, fx["h0"]) and np.array_equal(h1, fx["h1"])
        assert ad.samples_traced == fx["samples"] and ad.active == 0
        ad.clear()
        assert ad.samples_traced == 0 and not ad.frame().any()
        ad.run()
        assert np.array_equal(ad.frame(), fx["frame"])
    st = {}
    assert np.array_equal(R.render(env.sc, fx["cam"], W, H, seed=9, adaptive=kw, stats=st), fx["frame"])
    assert st["samples"] == fx["samples"] and np.array_equal(st["tile_spp"], fx["counts"])
    assert np.array_equal(R.render(env.sc, fx["cam"], W, H, seed=9, adaptive=kw, u8=True), fx["u8"])


def test_rt_main_adaptive_writes_the_adaptive_frame(gpu_lib, env, tmp_path):
    import json
    from rtclj import raytracing as R
    assert RT_MAIN.exists(), "lib/rt_main is not built (make -C raytracing-clj_amd)"
    child = dict(os.environ)
    child.pop("RTCLJ_LIBRARY", None)
    r = subprocess.run([str(RT_MAIN), "64", "50", "--width", "64", "--gpus", "1", "--no-png", "--out", "ad.ppm",
                        "--json", "--adaptive", "4096", "--step", "8", "--min-spp", "16", "--max-spp", "64"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120, env=child)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    w, h = 64, 36
    with R.Adaptive(env.sc, _cam(w, h), w, h, seed=1, tol_q16=4096, step=8, min_spp=16, max_spp=64) as ad:
        ad.run()
        want, counts, samples = ad.frame_u8(), ad.counts(), ad.samples_traced
    assert np.array_equal(R.read_ppm(tmp_path / "ad.ppm"), want)
    info = json.loads(r.stdout.strip().splitlines()[-1])["adaptive"]
    assert info == {"on": 1, "steps": int(counts.max()) // 8, "samples_traced": samples, "tiles": counts.size,
                    "tiles_at_cap": int((counts == 64).sum())}
    assert f"{samples} samples traced" in r.stdout


# ---- 8: rt_launch is untouched (after the tests above) ---------------------------------
def test_rt_launch_is_untouched_by_the_steps(env, fx):
    """Adaptive steps on the scene and stream, then plain rt_launch es there:
    the frames they gave before, and the occupancy the launches had before any
    step ran in this module."""
    p8 = _params(W, H, 16)
    ad = Ad(env, fx["p"])
    try:
        for _ in range(3):
            assert ad.step(fx["cam"]) > 0
        a = _launch(env, fx["cam"], p8)
        ad.run(fx["cam"])
        b = _launch(env, fx["cam"], p8)
    finally:
        ad.free()
    want = sum(fx["ones"][:16]).astype(np.float32) * np.float32(2.0 ** -24) / np.float32(16)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    for name, ww, hh, spp in OCC_SHAPES:
        assert _occupancy(env.ds, ww, hh, spp) == env.occ_before[name], name
