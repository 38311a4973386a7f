"""Temporal accumulation on the device (include/rt.h, rt_temporal_step): the
kernel gives rt_temporal_host's bits over consecutive steps with moving
cameras, whatever the stream and after a reset; render_sequence equals the
same chain run with the hosts on the arrays the device resolves produced; a
row band equals the host on that band.  Every output buffer is NaN-filled
first: no NaN may remain.
"""
import ctypes as C

import numpy as np
import pytest

from test_denoise_host import bits
from test_temporal_host import SIZES, cam_of, camera_pairs, running_mean, smooth_inputs

pytestmark = pytest.mark.gpu

W, H = 160, 90


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    e = Env()
    e.torch, e.R = torch, R
    e.sc = R.Scene.from_bodies(R.hittables)
    return e


def dev(env, a):
    t = env.torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
    env.torch.cuda.synchronize()
    return t


def nan_buf(env, n):
    t = env.torch.full((int(n),), float("nan"), dtype=env.torch.float32, device="cuda")
    env.torch.cuda.synchronize()
    return t


def step_cameras(width, height):
    """Three cameras for three consecutive steps: the base, a pan, then a dolly
    from there -- steps 2 and 3 each move."""
    pairs = camera_pairs(width, height)
    return [pairs["still"][0], pairs["pan"][1], pairs["dolly"][1]]


def device_step(env, tp, cam, half0, half1, feat, stream=None, **opts):
    """Temporal.step on host arrays -> (out0, out1), the inputs checked unchanged."""
    rows, width = half0.shape[:2]
    d0, d1, df = dev(env, half0), dev(env, half1), dev(env, feat)
    o0, o1 = nan_buf(env, half0.size), nan_buf(env, half0.size)
    tp.step(cam, d0.data_ptr(), d1.data_ptr(), df.data_ptr(), o0.data_ptr(), o1.data_ptr(),
            stream=stream.cuda_stream if stream is not None else None, **opts)
    env.torch.cuda.synchronize()
    got = [o.cpu().numpy().reshape(rows, width, 3) for o in (o0, o1)]
    assert not any(np.isnan(g).any() for g in got)
    for d, a in ((d0, half0), (d1, half1), (df, feat)):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a).reshape(-1))   # the inputs are never written
    return got


def check_chain(env, rows, width, steps=3, stream=None, tp=None, row0=0, **opts):
    """`steps` consecutive steps on one object against the host's chain: the
    outputs and rt_temporal_read after every step."""
    R = env.R
    cams = step_cameras(width, rows + row0 + 3)
    own = tp is None
    tp = tp or R.Temporal(width, rows, row0=row0)
    try:
        assert tp.frames == 0
        a0, a1, guide, length = tp.read()
        assert not length.any() and not a0.any() and not a1.any() and not guide.any()   # no history
        prev_cam, prev = None, None
        for s in range(steps):
            half0, half1, feat = smooth_inputs(rows, width, seed=1000 * rows + width + 17 * min(s, 2))
            if s == 3:      # a still step over the same guides, so that the smallest images accept history too
                half0, half1 = half1, half0
            cam = cams[min(s, 2)]
            got0, got1 = device_step(env, tp, cam, half0, half1, feat, stream=stream, **opts)
            want0, want1, want_len = R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, **opts)
            assert np.array_equal(bits(got0), bits(want0)), (s, int((bits(got0) != bits(want0)).sum()))
            assert np.array_equal(bits(got1), bits(want1)), (s, int((bits(got1) != bits(want1)).sum()))
            a0, a1, guide, length = tp.read(stream=stream.cuda_stream if stream is not None else None)
            assert np.array_equal(bits(a0), bits(want0)) and np.array_equal(bits(a1), bits(want1))
            assert np.array_equal(bits(length), bits(want_len))
            assert np.array_equal(bits(guide), bits(feat[..., 3:7]))
            assert tp.frames == s + 1
            if s > 0 and rows * width >= 200:
                assert 0.05 < (want_len > 1).mean() < 1.0      # history was found, and refused
            if s == 3:
                assert (want_len > 1).any()
            prev_cam, prev = cam, (want0, want1, np.ascontiguousarray(feat[..., 3:7]), want_len)
    finally:
        if own:
            tp.close()


# ---- 9. device == host, bit for bit -----------------------------------------------
@pytest.mark.parametrize("rows,width", SIZES + ((64, 64), (4, 64), (5, 65)))
def test_device_equals_host(env, rows, width):
    """Three steps with moving cameras, then a still one: both history sets
    are read and written twice."""
    check_chain(env, rows, width, steps=4)


def test_other_options_stream_and_reset(env):
    rows, width = 40, 33
    check_chain(env, rows, width, max_history=4, sigma_z=1.0, normal_min=-1.0)
    check_chain(env, rows, width, stream=env.torch.cuda.Stream())
    with env.R.Temporal(width, rows, row0=5) as tp:
        check_chain(env, rows, width, tp=tp, row0=5)
        tp.reset()
        check_chain(env, rows, width, steps=2, tp=tp, row0=5)      # from an empty history again


def test_device_argument_errors(env):
    from rtclj._lib import lib, rt_camera, rt_temporal_opts
    R = env.R
    rows, width = 9, 12
    half0, half1, feat = smooth_inputs(rows, width, seed=2)
    cam = cam_of(width, rows)
    d0, d1, df = dev(env, half0), dev(env, half1), dev(env, feat)
    o0, o1 = nan_buf(env, half0.size), nan_buf(env, half0.size)
    with R.Temporal(width, rows) as tp:
        got = device_step(env, tp, cam, half0, half1, feat)
        state = tp.read()
        p = [C.c_void_p(t.data_ptr()) for t in (d0, d1, df, o0, o1)]
        for k in range(5):
            bad = list(p)
            bad[k] = None
            assert lib.rt_temporal_step(tp._tp, None, C.byref(cam), *bad, None) == -1 and b"NULL" in lib.rt_last_error()
        assert lib.rt_temporal_step(tp._tp, None, None, *p, None) == -1
        assert lib.rt_temporal_step(tp._tp, C.byref(rt_temporal_opts(0, 0.1, 0.9)), C.byref(cam), *p, None) == -1
        for k in range(3):   # an output may not overlap an input, nor the other output
            assert lib.rt_temporal_step(tp._tp, None, C.byref(cam), p[0], p[1], p[2], p[k], p[4], None) == -1
            assert b"overlap" in lib.rt_last_error()
        assert lib.rt_temporal_step(tp._tp, None, C.byref(cam), p[0], p[1], p[2], p[3], p[3], None) == -1
        # a degenerate previous camera is found at the step after it; drop it by a reset
        env.torch.cuda.synchronize()
        assert tp.frames == 1
        for a, b in zip(tp.read(), state):
            assert np.array_equal(bits(a), bits(b))            # the failed calls left the state alone
        assert np.isnan(o0.cpu().numpy()).all() and np.isnan(o1.cpu().numpy()).all()
        # ... the previous camera included: the next step is the host's second step
        cam2 = camera_pairs(width, rows)["pan"][1]
        got2 = device_step(env, tp, cam2, half1, half0, feat)
        want2 = R.temporal_host(cam2, cam, half1, half0, feat, prev=state)
        assert np.array_equal(bits(got2[0]), bits(want2[0])) and np.array_equal(bits(got2[1]), bits(want2[1]))
        flat = rt_camera.from_buffer_copy(cam)
        flat.du[0] = flat.du[1] = flat.du[2] = 0.0
        device_step(env, tp, flat, half0, half1, feat)          # (accepted: a camera is judged as the previous one)
        assert lib.rt_temporal_step(tp._tp, None, C.byref(cam), *p, None) == -1 and b"degenerate" in lib.rt_last_error()
        assert tp.frames == 3
        tp.reset()
        assert tp.frames == 0
        assert lib.rt_temporal_step(tp._tp, None, C.byref(cam), *p, None) == 0
        env.torch.cuda.synchronize()
        assert np.array_equal(bits(o0.cpu().numpy()), bits(got[0]).reshape(-1))
    h = C.c_void_p()
    assert lib.rt_temporal_create(lib.rt_device_count(), 8, 8, 0, C.byref(h)) == -5 and not h.value


# ---- 10. the pipeline ---------------------------------------------------------------
def orbit_cameras(R, n, still=False):
    out = []
    for f in range(n):
        ang = 0.0 if still else np.radians(0.4) * f
        lf = (-2.0 * np.cos(ang) + 1.0 * np.sin(ang), 2.0, 2.0 * np.sin(ang) + 1.0 * np.cos(ang))
        out.append(R.camera(W, H, **{**R.REFERENCE_CAMERA, "look_from": lf}))
    return out


def test_pipeline_equals_hosts(env):
    """render_sequence over 4 moving cameras at 160 x 90, 2 + 2 spp: every
    frame equals temporal_host and denoise_host chained over the arrays the
    device resolves produced."""
    R = env.R
    cams = orbit_cameras(R, 4)
    prev_cam, prev = None, None
    lengths = []
    for f, (den, h0, h1, feat, acc0, acc1) in enumerate(R.render_sequence(env.sc, cams, W, H, spp=4, seed=5,
                                                                         stages=True)):
        assert not any(np.isnan(a).any() for a in (den, h0, h1, acc0, acc1))
        want0, want1, length = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev)
        assert np.array_equal(bits(acc0), bits(want0)) and np.array_equal(bits(acc1), bits(want1)), f
        assert np.array_equal(bits(den), bits(R.denoise_host(want0, want1, feat))), f
        prev_cam, prev = cams[f], (want0, want1, np.ascontiguousarray(feat[..., 3:7]), length)
        lengths.append(float(length.mean()))
    assert f == 3
    print("mean history length per frame:", ["%.2f" % v for v in lengths])
    assert lengths[0] == 1.0 and lengths[3] > 2.5            # the history builds under motion
    # the frames' samples differ: frame f starts at sample f * spp
    plain = [out for out in R.render_sequence(env.sc, cams[:1] * 2, W, H, spp=4, seed=5, stages=True)]
    assert not np.array_equal(bits(plain[0][1]), bits(plain[1][1]))
    with R.Progressive(env.sc, cams[0], W, H, seed=5, sample_begin=4) as a0:
        a0.add(2)
        assert np.array_equal(bits(a0.frame()), bits(plain[1][1]))


def test_still_pipeline_is_a_running_mean(env):
    """A still camera: where the history was accepted at every frame (length
    f + 1; the guides of successive frames come from different samples, so a
    few edge pixels are refused), the step's outputs after frame f are the
    fp32 running mean of the per-frame resolves, by the recurrence of
    tests/test_temporal_host.py."""
    R = env.R
    cams = orbit_cameras(R, 4, still=True)
    h0s, h1s = [], []
    always = np.ones((H, W), bool)
    prev_cam, prev = None, None
    for f, (den, h0, h1, feat, acc0, acc1) in enumerate(R.render_sequence(env.sc, cams, W, H, spp=4, seed=9,
                                                                         stages=True)):
        h0s.append(h0)
        h1s.append(h1)
        _, _, length = R.temporal_host(cams[f], prev_cam, h0, h1, feat, prev=prev)
        prev_cam, prev = cams[f], (acc0, acc1, np.ascontiguousarray(feat[..., 3:7]), length)
        always &= length == f + 1
        assert np.array_equal(bits(acc0[always]), bits(running_mean(h0s)[always])), f
        assert np.array_equal(bits(acc1[always]), bits(running_mean(h1s)[always])), f
    print("history accepted at every frame on %.2f %% of the pixels" % (100 * always.mean()))
    assert always.mean() > 0.75      # (most of the frame: the comparison above is not over a few pixels)


# ---- 11. a row band -------------------------------------------------------------------
def test_band_equals_host(env):
    """Rows 40..63 of a 160 x 90 sequence on their own (row0 = 40): the device
    equals the host on the same band, taps outside the band being outside the
    image."""
    R, torch = env.R, env.torch
    r0, rows = 40, 24
    cams = orbit_cameras(R, 3)
    d_h = [nan_buf(env, W * rows * 3) for _ in range(2)]
    d_feat = nan_buf(env, W * rows * 8)
    prev_cam, prev = None, None
    with R.Temporal(W, rows, row0=r0) as tp:
        for f, cam in enumerate(cams):
            kw = dict(seed=5, rows=(r0, r0 + rows))
            with R.Progressive(env.sc, cam, W, H, sample_begin=4 * f, **kw) as a0, \
                    R.Progressive(env.sc, cam, W, H, sample_begin=4 * f + 2, **kw) as a1, \
                    R.Features(env.sc, cam, W, H, sample_begin=4 * f, **kw) as ft:
                a0.add(2)
                a1.add(2)
                ft.add(4)
                a0.resolve_into(d_h[0].data_ptr())
                a1.resolve_into(d_h[1].data_ptr())
                ft.resolve_into(d_feat.data_ptr())
                torch.cuda.synchronize()
            h0, h1 = (d.cpu().numpy().reshape(rows, W, 3) for d in d_h)
            feat = d_feat.cpu().numpy().reshape(rows, W, 8)
            o0, o1 = nan_buf(env, W * rows * 3), nan_buf(env, W * rows * 3)
            tp.step(cam, d_h[0].data_ptr(), d_h[1].data_ptr(), d_feat.data_ptr(), o0.data_ptr(), o1.data_ptr())
            torch.cuda.synchronize()
            want0, want1, length = R.temporal_host(cam, prev_cam, h0, h1, feat, prev=prev, row0=r0)
            assert np.array_equal(bits(o0.cpu().numpy()), bits(want0).reshape(-1)), f
            assert np.array_equal(bits(o1.cpu().numpy()), bits(want1).reshape(-1)), f
            assert np.array_equal(bits(tp.read()[3]), bits(length)), f
            prev_cam, prev = cam, (want0, want1, np.ascontiguousarray(feat[..., 3:7]), length)
        assert (length > 1).mean() > 0.5          # the band found its history: row0 entered the reprojection
