"""The colour clamp of temporal accumulation on the device (include/rt.h,
rt_temporal_step_clamp): the box kernel and the clamped step give
rt_temporal_host_clamp's bits over consecutive steps -- image sizes at and
around the 64 x 4 tile, a row band, every radius, with and without ids, a
stream of its own, a reset in between, all three step entries alternating on
one object -- and rt_temporal_read's history is the host's; gamma = +inf is
rt_temporal_step_motion (rt_temporal_step without ids); a refused call leaves
history and previous camera alone; render_animation and render_sequence with
`clamp` equal the hosts chained over the arrays the device resolved, and
without it today's frames.  Every output buffer is pre-filled with NaN: no fill
value may remain.  Inputs are finite; hostile numbers are
tools/clamp_check.cpp's business, on the host.
"""
import ctypes as C

import numpy as np
import pytest

import test_temporal_clamp_host as K
from test_denoise_host import bits
from test_gpu_motion import dev, device_step, env, nan_buf  # noqa: F401  (env: the module's fixture)
from test_motion_host import N_BODIES, random_motion, rising
from test_temporal_host import cam_of, camera_pairs, smooth_inputs

pytestmark = pytest.mark.gpu

FRAMES = ((1, 1), (63, 3), (64, 4), (65, 5), (130, 11), (200, 37))     # width x rows: the tile's edges, the halo's corners


def host_step(R, kind, cam, prev_cam, half0, half1, feat, ids, motion, prev, row0, clamp, **opts):
    """The host's step of one kind: 'clamp' (no ids), 'clamp_ids', 'motion' or 'plain'."""
    kw = dict(prev=prev, row0=row0, **opts)
    if kind in ("clamp_ids", "motion"):
        kw.update(ids=ids, motion=motion)
    if kind.startswith("clamp"):
        kw.update(clamp=clamp)
    return R.temporal_host(cam, prev_cam, half0, half1, feat, **kw)


def check_chain(env, rows, width, kinds, clamp, row0=0, stream=None, tp=None, **opts):
    """One step per entry of `kinds` on one object against the host's chain:
    the outputs and rt_temporal_read after every step.  Returns how many
    pixels the clamped steps changed against the unclamped step of their kind."""
    R = env.R
    _, _, frames = K.chain_inputs(rows, width, row0)
    own = tp is None
    tp = tp or R.Temporal(width, rows, row0=row0)
    changed = 0
    try:
        assert tp.frames == 0
        prev_cam, prev = None, None
        for s, kind in enumerate(kinds):
            cam, half0, half1, feat, ids, motion = frames[s % len(frames)]
            with_ids = kind in ("clamp_ids", "motion")
            got0, got1 = device_step(env, tp, cam, half0, half1, feat, ids if with_ids else None,
                                     motion if with_ids else None, stream=stream,
                                     **(dict(clamp=clamp) if kind.startswith("clamp") else {}), **opts)
            want0, want1, want_len = host_step(R, kind, cam, prev_cam, half0, half1, feat, ids, motion, prev, row0, clamp,
                                               **opts)
            assert np.array_equal(bits(got0), bits(want0)), (s, kind, int((bits(got0) != bits(want0)).sum()))
            assert np.array_equal(bits(got1), bits(want1)), (s, kind, int((bits(got1) != bits(want1)).sum()))
            a0, a1, guide, length = tp.read(stream=stream.cuda_stream if stream is not None else None)
            assert np.array_equal(bits(a0), bits(want0)) and np.array_equal(bits(a1), bits(want1))
            assert np.array_equal(bits(length), bits(want_len))
            assert np.array_equal(bits(guide), bits(feat[..., 3:7]))
            assert tp.frames == s + 1
            if kind.startswith("clamp"):
                free = host_step(R, "motion" if with_ids else "plain", cam, prev_cam, half0, half1, feat, ids, motion,
                                 prev, row0, None, **opts)
                changed += int((bits(free[0]) != bits(want0)).any(axis=-1).sum())
            prev_cam, prev = cam, (want0, want1, np.ascontiguousarray(feat[..., 3:7]), want_len)
    finally:
        if own:
            tp.close()
    return changed


# ---- 1. rt_temporal_step_clamp == rt_temporal_host_clamp ---------------------------------------
@pytest.mark.parametrize("width,rows", FRAMES)
def test_device_equals_host(env, width, rows):
    changed = 0
    for radius in (1, 2, 3):
        for kind in ("clamp", "clamp_ids"):
            changed += check_chain(env, rows, width, [kind] * 4, dict(radius=radius, gamma=1.0))
    changed += check_chain(env, rows, width, ["clamp_ids"] * 4, dict(radius=2, gamma=0.25))
    changed += check_chain(env, rows, width, ["clamp"] * 4, {})
    print(f"{width} x {rows}: pixels the clamp changed over all chains: {changed}")
    if rows * width >= 180:
        assert changed > 0       # the inputs are not blind to the clamp


def test_band_stream_reset_and_alternating_entries(env):
    rows, width = 37, 70
    mixed = ["clamp_ids", "plain", "clamp", "motion", "clamp_ids", "clamp", "motion", "clamp"]
    assert check_chain(env, rows, width, ["clamp_ids"] * 4, dict(radius=3, gamma=0.5), row0=5) > 0
    assert check_chain(env, rows, width, mixed, dict(radius=2, gamma=0.5)) > 0
    assert check_chain(env, rows, width, mixed[:5], dict(radius=1, gamma=2.0), stream=env.torch.cuda.Stream(),
                       max_history=4, sigma_z=1.0, normal_min=-1.0) > 0
    with env.R.Temporal(width, rows, row0=5) as tp:
        check_chain(env, rows, width, ["motion", "clamp_ids", "clamp"], {}, row0=5, tp=tp)
        tp.reset()
        check_chain(env, rows, width, ["clamp", "clamp_ids", "plain", "clamp_ids"], dict(radius=3), row0=5, tp=tp)


# ---- 2. gamma = +inf is the unclamped step -------------------------------------------------------
@pytest.mark.parametrize("with_ids", (True, False))
def test_infinite_gamma_is_the_unclamped_step(env, with_ids):
    R = env.R
    rows, width = 37, 130
    _, _, frames = K.chain_inputs(rows, width, 0)
    tps = [R.Temporal(width, rows) for _ in range(4)]
    try:
        for cam, half0, half1, feat, ids, motion in frames:
            i_, m_ = (ids, motion) if with_ids else (None, None)
            want = device_step(env, tps[0], cam, half0, half1, feat, i_, m_)
            state = tps[0].read()
            for tp, radius in zip(tps[1:], (1, 2, 3)):
                got = device_step(env, tp, cam, half0, half1, feat, i_, m_, clamp=dict(radius=radius, gamma=float("inf")))
                assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)), radius
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tp.read(), state)), radius
        assert (state[3] > 1).mean() > 0.05
    finally:
        for tp in tps:
            tp.close()


# ---- 3. argument errors -----------------------------------------------------------------------------
def test_device_argument_errors(env):
    from rtclj._lib import rt_temporal_clamp_opts, rt_temporal_opts
    R, lib = env.R, env.lib
    rows, width = 9, 12
    half0, half1, feat = smooth_inputs(rows, width, seed=2)
    ids, motion = random_motion(rows, width, seed=3)
    cam = cam_of(width, rows)
    d0, d1, df, di, dm = dev(env, half0), dev(env, half1), dev(env, feat), dev(env, ids, np.int32), dev(env, motion)
    o0, o1 = nan_buf(env, half0.size), nan_buf(env, half0.size)
    with R.Temporal(width, rows) as tp:
        got = device_step(env, tp, cam, half0, half1, feat, ids, motion, clamp={})
        state = tp.read()
        p = [C.c_void_p(t.data_ptr()) for t in (d0, d1, df, di, dm)] + [N_BODIES] + [C.c_void_p(t.data_ptr()) for t in (o0, o1)]

        def call(args, o=None, k=None, c=cam):
            return lib.rt_temporal_step_clamp(tp._tp, o, k, C.byref(c) if c is not None else None, *args, None)

        for i in (0, 1, 2, 4, 6, 7):          # (a NULL d_ids is the step without ids)
            bad = list(p)
            bad[i] = None
            assert call(bad) == -1 and b"NULL" in lib.rt_last_error(), i
        assert call(p, c=None) == -1 and b"NULL" in lib.rt_last_error()
        assert call(p[:5] + [-1] + p[6:]) == -1 and b"n_bodies" in lib.rt_last_error()
        assert call(p[:4] + [C.c_void_p(dm.data_ptr() + 4)] + p[5:]) == -1 and b"aligned" in lib.rt_last_error()
        assert call(p, o=C.byref(rt_temporal_opts(0, 0.1, 0.9))) == -1 and b"max_history" in lib.rt_last_error()
        for radius in (0, 4, -2):
            assert call(p, k=C.byref(rt_temporal_clamp_opts(radius, 1.0))) == -1 and b"radius" in lib.rt_last_error()
        for gamma in (0.0, -1.0, float("nan")):
            assert call(p, k=C.byref(rt_temporal_clamp_opts(2, gamma))) == -1 and b"gamma" in lib.rt_last_error()
        for i in range(5):    # an output may not overlap an input -- the ids and the table included -- nor the other output
            assert call(p[:6] + [p[i], p[7]]) == -1 and b"overlap" in lib.rt_last_error(), i
            assert call(p[:6] + [p[6], p[i]]) == -1 and b"overlap" in lib.rt_last_error(), i
        assert call(p[:6] + [p[6], p[6]]) == -1 and b"overlap" in lib.rt_last_error()
        env.torch.cuda.synchronize()
        assert tp.frames == 1
        for a, b in zip(tp.read(), state):
            assert np.array_equal(bits(a), bits(b))            # the failed calls left the state alone
        assert np.isnan(o0.cpu().numpy()).all() and np.isnan(o1.cpu().numpy()).all()
        # ... the previous camera included: the next step is the host's second step
        cam2 = camera_pairs(width, rows)["pan"][1]
        got2 = device_step(env, tp, cam2, half1, half0, feat, ids, motion, clamp=dict(radius=1))
        want2 = R.temporal_host(cam2, cam, half1, half0, feat, prev=state, ids=ids, motion=motion, clamp=dict(radius=1))
        assert np.array_equal(bits(got2[0]), bits(want2[0])) and np.array_equal(bits(got2[1]), bits(want2[1]))
        # without ids the table and its length are not read
        state2 = tp.read()
        assert call(p[:3] + [None, None, -7] + p[6:]) == 0
        env.torch.cuda.synchronize()
        want3 = R.temporal_host(cam, cam2, half0, half1, feat, prev=state2, clamp={})
        assert np.array_equal(bits(o0.cpu().numpy()), bits(want3[0]).reshape(-1)) and tp.frames == 3
        with pytest.raises(ValueError):
            tp.step(cam, p[0].value, p[1].value, p[2].value, p[6].value, p[7].value, d_motion=dm.data_ptr(), clamp={})
        with pytest.raises(TypeError):
            tp.step(cam, p[0].value, p[1].value, p[2].value, p[6].value, p[7].value, clamp=dict(sigma=2))
    assert got[0].shape == (rows, width, 3)


# ---- 4. the pipeline -----------------------------------------------------------------------------------
PW, PH = 96, 54


def pipeline_cameras(R, n):
    out = []
    for f in range(n):
        ang = np.radians(0.4) * f
        lf = (-2.0 * np.cos(ang) + 1.0 * np.sin(ang), 2.0, 2.0 * np.sin(ang) + 1.0 * np.cos(ang))
        out.append(R.camera(PW, PH, **{**R.REFERENCE_CAMERA, "look_from": lf}))
    return out


@pytest.mark.parametrize("clamp", ({}, dict(radius=1, gamma=0.5), None))
def test_animation_pipeline_equals_hosts(env, clamp):
    """render_animation over 4 frames at 96 x 54, 2 + 2 spp, the centre sphere
    rising 0.08 a frame under a 0.4-degree orbit: every frame equals ids_host,
    temporal_host(..., ids, motion, clamp) and denoise_host chained over the
    arrays the device resolved; clamp = None: the motion-aware step's frames."""
    R = env.R
    cams = pipeline_cameras(R, 4)
    scs = [R.Scene.from_bodies(rising(f, 4)) for f in range(4)]
    prev_cam, prev, changed = None, None, 0
    for f, (den, h0, h1, feat, acc0, acc1, ids) in enumerate(R.render_animation(scs, cams, PW, PH, spp=4, seed=5, stages=True,
                                                                               clamp=clamp)):
        assert not any(np.isnan(a).any() for a in (den, h0, h1, acc0, acc1))
        assert np.array_equal(ids, R.ids_host(scs[f], cams[f], PW, PH)), f
        motion = R.body_motion(scs[f], scs[f - 1]) if f else np.zeros((5, 4), np.float32)
        want0, want1, length = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev, ids=ids, motion=motion, clamp=clamp)
        assert np.array_equal(bits(acc0), bits(want0)) and np.array_equal(bits(acc1), bits(want1)), f
        assert np.array_equal(bits(den), bits(R.denoise_host(want0, want1, feat))), f
        free = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev, ids=ids, motion=motion)
        changed += int((bits(free[0]) != bits(want0)).any(axis=-1).sum())
        prev_cam, prev = cams[f], (want0, want1, np.ascontiguousarray(feat[..., 3:7]), length)
    assert f == 3 and (length > 1).mean() > 0.5
    assert (changed > 100) if clamp is not None else (changed == 0)


def test_sequence_pipeline_equals_hosts(env):
    R = env.R
    cams = pipeline_cameras(R, 3)
    prev_cam, prev = None, None
    for f, (den, h0, h1, feat, acc0, acc1) in enumerate(R.render_sequence(env.ref, cams, PW, PH, spp=4, seed=5, stages=True,
                                                                          clamp=dict(radius=3))):
        want0, want1, length = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev, clamp=dict(radius=3))
        assert np.array_equal(bits(acc0), bits(want0)) and np.array_equal(bits(acc1), bits(want1)), f
        assert np.array_equal(bits(den), bits(R.denoise_host(want0, want1, feat))), f
        prev_cam, prev = cams[f], (want0, want1, np.ascontiguousarray(feat[..., 3:7]), length)
    assert f == 2
    # clamp = None is the call without the keyword
    a = list(R.render_sequence(env.ref, cams[:2], PW, PH, spp=4, seed=5))
    b = list(R.render_sequence(env.ref, cams[:2], PW, PH, spp=4, seed=5, clamp=None))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
