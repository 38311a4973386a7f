"""Moving bodies on the device (include/rt.h: rt_launch_ids,
rt_temporal_step_motion): the body-id kernel gives rt_ids_host's integers for
every source of bodies, image shape and edge scene; the motion-aware step gives
rt_temporal_host_motion's bits over consecutive steps, alone and alternating
with rt_temporal_step on one object; zero motion is rt_temporal_step;
render_animation equals the hosts chained over the arrays the device resolved,
and render_sequence when nothing moves.  Every output buffer is pre-filled
(floats with NaN, ids with 0x7fffffff): no fill value may remain.  Cameras are
finite; hostile numbers are tools/motion_check.cpp's business, on the host.
"""
import ctypes as C

import numpy as np
import pytest

import edge_scenes as E
from test_denoise_host import bits
from test_gpu_temporal import orbit_cameras, step_cameras
from test_motion_host import N_BODIES, random_motion, rising
from test_temporal_host import SIZES, cam_of, camera_pairs, smooth_inputs

pytestmark = pytest.mark.gpu

W, H = 160, 90
FILL = 0x7fffffff


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R, scenes
    e = Env()
    e.torch, e.R, e.scenes, e.lib = torch, R, scenes, gpu_lib.lib
    e.ref = R.Scene.from_bodies(R.hittables)
    e.cover = scenes.cover(11)
    return e


def dev(env, a, dtype=np.float32):
    t = env.torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1)).cuda()
    env.torch.cuda.synchronize()
    return t


def nan_buf(env, n):
    t = env.torch.full((int(n),), float("nan"), dtype=env.torch.float32, device="cuda")
    env.torch.cuda.synchronize()
    return t


class Uploaded:
    """A scene on device 0 for a `with` block."""

    def __init__(self, env, sc):
        self.env, self.ds = env, C.c_void_p()
        assert env.lib.rt_scene_upload(0, C.byref(sc.c), C.byref(self.ds)) == 0, env.lib.rt_last_error()

    def __enter__(self):
        return self.ds

    def __exit__(self, *exc):
        self.env.torch.cuda.synchronize()
        self.env.lib.rt_scene_free(self.ds)


def device_ids(env, ds, cam, width, rows, row0=0, stream=None):
    """rt_launch_ids into a pre-filled buffer -> int32 (rows, width)."""
    torch = env.torch
    d = torch.full((rows * width,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    assert env.lib.rt_launch_ids(ds, C.byref(cam), width, rows, row0, C.c_void_p(d.data_ptr()), st) == 0, \
        env.lib.rt_last_error()
    torch.cuda.synchronize()
    got = d.cpu().numpy().reshape(rows, width)
    assert not (got == FILL).any()
    return got


# ---- 1. rt_launch_ids == rt_ids_host ------------------------------------------------------
FRAMES = ((160, 90), (65, 37), (33, 17), (65, 5), (1, 1))     # width x height


@pytest.mark.parametrize("which", ("reference", "cover"))
def test_ids_equal_host(env, which):
    R = env.R
    sc = env.ref if which == "reference" else env.cover
    camera = (lambda w, h: R.camera(w, h, **R.REFERENCE_CAMERA)) if which == "reference" else env.scenes.cover_camera
    out4 = (C.c_int * 4)()
    with Uploaded(env, sc) as ds:
        for w, h in FRAMES:
            cam = camera(w, h)
            want = R.ids_host(sc, cam, w, h)
            for variant in (0, 5, 12, 16):
                old = env.lib.rt_set_variant(variant)
                try:
                    got = device_ids(env, ds, cam, w, h)
                    assert env.lib.rt_ids_occupancy(ds, out4) == 0
                finally:
                    env.lib.rt_set_variant(old)
                assert np.array_equal(got, want), (which, w, h, variant, int((got != want).sum()))
                assert out4[3] == {5: 2, 12: 1, 16: 0}.get(variant, out4[3]) and out4[0] >= 1 and out4[1] > 0
        cam = camera(W, H)
        want = R.ids_host(sc, cam, W, H)
        # a row band, and a stream of its own
        assert np.array_equal(device_ids(env, ds, cam, W, 24, row0=40), want[40:64])
        assert np.array_equal(device_ids(env, ds, cam, W, 24, row0=40), R.ids_host(sc, cam, W, 24, 40))
        assert np.array_equal(device_ids(env, ds, cam, W, H, stream=env.torch.cuda.Stream()), want)
        assert env.lib.rt_set_variant(0) == 0          # the selector is back where it was
        assert len(np.unique(want)) >= (4 if which == "reference" else 20)


def test_ids_of_a_large_scene(env):
    """cover(16): 1025 bodies, a tree of several levels."""
    sc = env.scenes.cover(16)
    assert len(sc) == 1025
    cam = env.scenes.cover_camera(65, 37)
    want = env.R.ids_host(sc, cam, 65, 37)
    with Uploaded(env, sc) as ds:
        for variant in (0, 5, 12, 16):
            old = env.lib.rt_set_variant(variant)
            try:
                got = device_ids(env, ds, cam, 65, 37)
            finally:
                env.lib.rt_set_variant(old)
            assert np.array_equal(got, want), (variant, int((got != want).sum()))
    assert len(np.unique(want)) > 50


@pytest.mark.parametrize("name", ("ties", "ties_big", "nonfinite_few", "nonfinite_64", "nonfinite_65", "nonfinite_80",
                                  "bubble_negative_radius", "neg_radius_field", "camera_inside_glass"))
def test_ids_of_edge_scenes(env, name):
    sc, cam, _ = E.case(name)
    want = env.R.ids_host(sc, cam, E.W, E.H)
    with Uploaded(env, sc) as ds:
        for variant in (0, 5, 12):
            old = env.lib.rt_set_variant(variant)
            try:
                got = device_ids(env, ds, cam, E.W, E.H)
            finally:
                env.lib.rt_set_variant(old)
            assert np.array_equal(got, want), (name, variant, int((got != want).sum()))
    if name.startswith("nonfinite"):     # a body with a NaN, infinite or overflowing radius is never hit
        with np.errstate(over="ignore", invalid="ignore"):
            r2 = sc.sphere[:, 3] * sc.sphere[:, 3]
        assert not np.isin(want, np.flatnonzero(~np.isfinite(r2))).any()
    if name == "ties":                   # coincident bodies: the first in array order
        assert len(np.unique(want)) >= 2


def test_body_ids_into(env):
    """The Python entry for a scene on the host: upload, pass, wait, free."""
    R, torch = env.R, env.torch
    cam = R.camera(W, H, **R.REFERENCE_CAMERA)
    want = R.ids_host(R.hittables, cam, W, H)
    d = torch.full((H * W,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.body_ids_into(R.hittables, cam, W, H, d.data_ptr())
    assert np.array_equal(d.cpu().numpy().reshape(H, W), want)
    band = torch.full((24 * W,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    R.body_ids_into(env.ref, cam, W, H, band.data_ptr(), rows=(40, 64), stream=stream.cuda_stream)
    assert np.array_equal(band.cpu().numpy().reshape(24, W), want[40:64])
    with pytest.raises(R.RTError):
        R.body_ids_into(env.ref, cam, W, H, band.data_ptr(), rows=(40, 40))


def test_ids_argument_errors(env):
    lib, torch = env.lib, env.torch
    cam = env.R.camera(16, 9, **env.R.REFERENCE_CAMERA)
    d = torch.full((16 * 9,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = C.c_void_p(d.data_ptr())
    with Uploaded(env, env.ref) as ds:
        for args, word in (((None, C.byref(cam), 16, 9, 0, p, None), b"NULL"), ((ds, None, 16, 9, 0, p, None), b"NULL"),
                           ((ds, C.byref(cam), 16, 9, 0, None, None), b"NULL"),
                           ((ds, C.byref(cam), 0, 9, 0, p, None), b"width/rows"),
                           ((ds, C.byref(cam), 16, -1, 0, p, None), b"width/rows"),
                           ((ds, C.byref(cam), 1 << 16, 1 << 16, 0, p, None), b"width/rows"),
                           ((ds, C.byref(cam), 16, 9, -1, p, None), b"row0")):
            assert lib.rt_launch_ids(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == FILL).all()
        assert lib.rt_ids_occupancy(ds, None) == -1


# ---- 2. rt_temporal_step_motion == rt_temporal_host_motion -----------------------------------
def device_step(env, tp, cam, half0, half1, feat, ids=None, motion=None, stream=None, **opts):
    """Temporal.step on host arrays -> (out0, out1); with ids, the motion-aware
    step.  The inputs are checked unchanged by bits."""
    rows, width = half0.shape[:2]
    d0, d1, df = dev(env, half0), dev(env, half1), dev(env, feat)
    o0, o1 = nan_buf(env, half0.size), nan_buf(env, half0.size)
    kw = {}
    if ids is not None:
        di, dm = dev(env, ids, np.int32), dev(env, motion)
        kw = dict(d_ids=di.data_ptr(), d_motion=dm.data_ptr() if len(motion) else None, n_bodies=len(motion))
    tp.step(cam, d0.data_ptr(), d1.data_ptr(), df.data_ptr(), o0.data_ptr(), o1.data_ptr(),
            stream=stream.cuda_stream if stream is not None else None, **kw, **opts)
    env.torch.cuda.synchronize()
    got = [o.cpu().numpy().reshape(rows, width, 3) for o in (o0, o1)]
    assert not any(np.isnan(g).any() for g in got)
    for d, a in ((d0, half0), (d1, half1), (df, feat)):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a).reshape(-1))
    if ids is not None:
        assert np.array_equal(di.cpu().numpy(), ids.reshape(-1))
        assert np.array_equal(bits(dm.cpu().numpy()), bits(motion).reshape(-1))
    return got


def check_chain(env, rows, width, steps=4, stream=None, tp=None, row0=0, alternate=False, **opts):
    """`steps` consecutive steps on one object against the host's chain: the
    outputs and rt_temporal_read after every step.  Cameras: test_gpu_temporal's
    three, then a still one.  alternate: the odd steps are rt_temporal_step's."""
    R = env.R
    cams = step_cameras(width, rows + row0 + 3)
    own = tp is None
    tp = tp or R.Temporal(width, rows, row0=row0)
    try:
        assert tp.frames == 0
        prev_cam, prev = None, None
        for s in range(steps):
            half0, half1, feat = smooth_inputs(rows, width, seed=1000 * rows + width + 17 * min(s, 2))
            if s == 3:
                half0, half1 = half1, half0
            ids, motion = random_motion(rows, width, seed=5 * rows + width + s)
            if s == 3:
                motion[:, :3] *= np.float32(0.01)        # nearly still: the smallest images accept history too
            cam = cams[min(s, 2)]
            blind = alternate and s % 2 == 1
            if blind:
                got0, got1 = device_step(env, tp, cam, half0, half1, feat, stream=stream, **opts)
                want0, want1, want_len = R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, **opts)
            else:
                got0, got1 = device_step(env, tp, cam, half0, half1, feat, ids, motion, stream=stream, **opts)
                want0, want1, want_len = R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, ids=ids,
                                                         motion=motion, **opts)
            assert np.array_equal(bits(got0), bits(want0)), (s, int((bits(got0) != bits(want0)).sum()))
            assert np.array_equal(bits(got1), bits(want1)), (s, int((bits(got1) != bits(want1)).sum()))
            a0, a1, guide, length = tp.read(stream=stream.cuda_stream if stream is not None else None)
            assert np.array_equal(bits(a0), bits(want0)) and np.array_equal(bits(a1), bits(want1))
            assert np.array_equal(bits(length), bits(want_len))
            assert np.array_equal(bits(guide), bits(feat[..., 3:7]))
            assert tp.frames == s + 1
            if s > 0 and rows * width >= 200:
                assert 0.03 < (want_len > 1).mean() < 1.0      # history was found, and refused
                if not blind:                                   # ... and the table mattered
                    plain = R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, **opts)[2]
                    assert not np.array_equal(bits(plain), bits(want_len))
            prev_cam, prev = cam, (want0, want1, np.ascontiguousarray(feat[..., 3:7]), want_len)
    finally:
        if own:
            tp.close()


@pytest.mark.parametrize("rows,width", SIZES + ((64, 64), (4, 64), (5, 65)))
def test_device_equals_host(env, rows, width):
    check_chain(env, rows, width, steps=4)


def test_alternating_options_stream_and_reset(env):
    rows, width = 40, 33
    check_chain(env, rows, width, alternate=True)
    check_chain(env, rows, width, steps=3, max_history=4, sigma_z=1.0, normal_min=-1.0)
    check_chain(env, rows, width, steps=3, stream=env.torch.cuda.Stream())
    with env.R.Temporal(width, rows, row0=5) as tp:
        check_chain(env, rows, width, steps=3, tp=tp, row0=5)
        tp.reset()
        check_chain(env, rows, width, steps=2, tp=tp, row0=5, alternate=True)


# ---- 3. zero motion is rt_temporal_step -------------------------------------------------------
def test_zero_motion_is_the_existing_step(env):
    R = env.R
    rows, width = 40, 33
    cams = step_cameras(width, rows + 3)
    ids, motion = random_motion(rows, width, seed=11)
    cases = (("zero table", ids, np.zeros_like(motion)), ("ids -1", np.full_like(ids, -1), motion),
             ("n_bodies 0", ids, np.zeros((0, 4), np.float32)))
    with R.Temporal(width, rows) as plain:
        tps = [R.Temporal(width, rows) for _ in cases]
        try:
            for s, cam in enumerate(cams):
                half0, half1, feat = smooth_inputs(rows, width, seed=300 + 17 * s)
                want = device_step(env, plain, cam, half0, half1, feat)
                state = plain.read()
                for tp, (what, i_, m_) in zip(tps, cases):
                    got = device_step(env, tp, cam, half0, half1, feat, i_, m_)
                    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)), (what, s)
                    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tp.read(), state)), (what, s)
            assert (state[3] > 1).mean() > 0.05
        finally:
            for tp in tps:
                tp.close()


# ---- 4. argument errors ---------------------------------------------------------------------------
def test_device_argument_errors(env):
    from rtclj._lib import rt_temporal_opts
    R, lib = env.R, env.lib
    rows, width = 9, 12
    half0, half1, feat = smooth_inputs(rows, width, seed=2)
    ids, motion = random_motion(rows, width, seed=3)
    cam = cam_of(width, rows)
    d0, d1, df, di, dm = dev(env, half0), dev(env, half1), dev(env, feat), dev(env, ids, np.int32), dev(env, motion)
    o0, o1 = nan_buf(env, half0.size), nan_buf(env, half0.size)
    with R.Temporal(width, rows) as tp:
        got = device_step(env, tp, cam, half0, half1, feat, ids, motion)
        state = tp.read()
        p = [C.c_void_p(t.data_ptr()) for t in (d0, d1, df, di, dm)] + [N_BODIES] + [C.c_void_p(t.data_ptr()) for t in (o0, o1)]

        def call(args, o=None, c=cam):
            return lib.rt_temporal_step_motion(tp._tp, o, C.byref(c) if c is not None else None, *args, None)

        for k in (0, 1, 2, 3, 4, 6, 7):
            bad = list(p)
            bad[k] = None
            assert call(bad) == -1 and b"NULL" in lib.rt_last_error(), k
        assert call(p, c=None) == -1 and b"NULL" in lib.rt_last_error()
        assert call(p[:5] + [-1] + p[6:]) == -1 and b"n_bodies" in lib.rt_last_error()
        assert call(p[:4] + [C.c_void_p(dm.data_ptr() + 4)] + p[5:]) == -1 and b"aligned" in lib.rt_last_error()
        assert call(p, o=C.byref(rt_temporal_opts(0, 0.1, 0.9))) == -1 and b"max_history" in lib.rt_last_error()
        for k in range(5):    # an output may not overlap an input -- the ids and the table included -- nor the other output
            assert call(p[:6] + [p[k], p[7]]) == -1 and b"overlap" in lib.rt_last_error(), k
            assert call(p[:6] + [p[6], p[k]]) == -1 and b"overlap" in lib.rt_last_error(), k
        assert call(p[:6] + [p[6], p[6]]) == -1 and b"overlap" in lib.rt_last_error()
        env.torch.cuda.synchronize()
        assert tp.frames == 1
        for a, b in zip(tp.read(), state):
            assert np.array_equal(bits(a), bits(b))            # the failed calls left the state alone
        assert np.isnan(o0.cpu().numpy()).all() and np.isnan(o1.cpu().numpy()).all()
        # ... the previous camera included: the next step is the host's second step
        cam2 = camera_pairs(width, rows)["pan"][1]
        got2 = device_step(env, tp, cam2, half1, half0, feat, ids, motion)
        want2 = R.temporal_host(cam2, cam, half1, half0, feat, prev=state, ids=ids, motion=motion)
        assert np.array_equal(bits(got2[0]), bits(want2[0])) and np.array_equal(bits(got2[1]), bits(want2[1]))
        # n_bodies = 0 needs no table
        assert call(p[:4] + [None, 0] + p[6:]) == 0
        env.torch.cuda.synchronize()
        assert tp.frames == 3 and not np.isnan(o0.cpu().numpy()).any()
        with pytest.raises(ValueError):
            tp.step(cam, p[0].value, p[1].value, p[2].value, p[6].value, p[7].value, d_motion=dm.data_ptr())
    assert got[0].shape == (rows, width, 3)


# ---- 5. the pipeline ------------------------------------------------------------------------------
def test_pipeline_equals_hosts(env):
    """render_animation over 4 frames at 160 x 90, 2 + 2 spp: the centre sphere
    rises 0.08 a frame under test_gpu_temporal's 0.4-degree orbit.  Every frame
    equals ids_host, temporal_host(..., ids, motion) and denoise_host chained
    over the arrays the device resolved.  The motion-blind host chain on the
    same arrays keeps less of the sphere's history."""
    R = env.R
    cams = orbit_cameras(R, 4)
    scs = [R.Scene.from_bodies(rising(f, 4)) for f in range(4)]
    prev_cam, prev, prev_blind = None, None, None
    for f, (den, h0, h1, feat, acc0, acc1, ids) in enumerate(R.render_animation(scs, cams, W, H, spp=4, seed=5,
                                                                               stages=True)):
        assert not any(np.isnan(a).any() for a in (den, h0, h1, acc0, acc1))
        assert ids.dtype == np.int32 and np.array_equal(ids, R.ids_host(scs[f], cams[f], W, H)), f
        motion = R.body_motion(scs[f], scs[f - 1]) if f else np.zeros((5, 4), np.float32)
        want0, want1, length = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev, ids=ids, motion=motion)
        assert np.array_equal(bits(acc0), bits(want0)) and np.array_equal(bits(acc1), bits(want1)), f
        assert np.array_equal(bits(den), bits(R.denoise_host(want0, want1, feat))), f
        b0, b1, blind_len = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev_blind)
        guide = np.ascontiguousarray(feat[..., 3:7])
        prev_cam, prev, prev_blind = cams[f], (want0, want1, guide, length), (b0, b1, guide, blind_len)
    assert f == 3
    body = ids == 1
    share, share_blind = float((length[body] == 4).mean()), float((blind_len[body] == 4).mean())
    print("the sphere's pixels with L = 4 at the last frame: with motion %.4f, motion-blind %.4f (%d pixels)"
          % (share, share_blind, int(body.sum())))
    assert body.sum() > 400 and share > share_blind


def test_still_bodies_give_render_sequence(env):
    R = env.R
    cams = orbit_cameras(R, 4)
    seq = list(R.render_sequence(env.ref, cams, W, H, spp=4, seed=5, stages=True))
    ani = list(R.render_animation([env.ref] * 4, cams, W, H, spp=4, seed=5, stages=True))
    assert len(seq) == len(ani) == 4
    for f, (s, a) in enumerate(zip(seq, ani)):
        assert len(a) == len(s) + 1
        for x, y in zip(s, a):
            assert np.array_equal(bits(x), bits(y)), f
    plain = list(R.render_animation([R.hittables] * 2, cams[:2], W, H, spp=4, seed=5))
    assert np.array_equal(bits(plain[1]), bits(seq[1][0]))
