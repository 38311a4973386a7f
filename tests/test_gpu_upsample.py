"""Guided upsampling on the device (include/rt.h: rt_upsample): the kernel gives
rt_upsample_host's bits for every image shape, scale, option set and stream,
one image or two; its argument errors; render_animation(scale=2) equals the
hosts chained over the arrays the device resolved; render_upscaled equals its
steps done by hand and rt_main --denoise --scale 2 writes its frame; the
quality and footprint checks of tests/test_upsample_host.py once more on the
device's own frames; and, reported only, what a render scale costs in error.
Every output buffer is pre-filled with NaN: none may remain.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_upsample_host as T
from test_upsample_host import bits, coarse, random_inputs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_MAIN = ROOT / "raytracing-clj_amd" / "lib" / "rt_main"
W, H = 160, 90
# rows x width, the full size: one pixel; more than one workgroup along x (a
# workgroup is 4 x 64 pixels) with partial ones; the same along y; a partial
# workgroup and partial coarse pixels at every scale; the pipeline's frame
SIZES = ((1, 1), (3, 257), (257, 3), (33, 40), (90, 160))
OPTIONS = (dict(), dict(normal_pow2=5, sigma_z=1.0))


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    e = Env()
    e.torch, e.R, e.lib = torch, R, gpu_lib.lib
    e.sc = R.Scene.from_bodies(R.hittables)
    e.cam = R.camera(W, H, **R.REFERENCE_CAMERA)
    return e


def dev(env, a):
    t = env.torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
    env.torch.cuda.synchronize()
    return t


def nan_buf(env, n):
    t = env.torch.full((int(n),), float("nan"), dtype=env.torch.float32, device="cuda")
    env.torch.cuda.synchronize()
    return t


def run_device(env, half0, half1, fc, ff, stream=None, **opts):
    """upsample_into on host arrays -> (out0, out1 or None), the inputs checked unchanged."""
    rows, width = ff.shape[:2]
    ins = [(dev(env, a), a) for a in (half0, half1, fc, ff) if a is not None]
    d = {id(a): t for t, a in ins}
    o0 = nan_buf(env, rows * width * 3)
    o1 = nan_buf(env, rows * width * 3) if half1 is not None else None
    env.R.upsample_into(d[id(half0)].data_ptr(), d[id(half1)].data_ptr() if half1 is not None else None,
                        d[id(fc)].data_ptr(), d[id(ff)].data_ptr(), width, rows, o0.data_ptr(),
                        o1.data_ptr() if o1 is not None else None,
                        stream=stream.cuda_stream if stream is not None else None, **opts)
    env.torch.cuda.synchronize()
    outs = [t.cpu().numpy().reshape(rows, width, 3) if t is not None else None for t in (o0, o1)]
    assert not any(np.isnan(o).any() for o in outs if o is not None)
    for t, a in ins:
        assert np.array_equal(bits(t.cpu().numpy()), bits(a).reshape(-1))   # the inputs are never written
    return outs


# ---- 8. device == host, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("s", T.SCALES)
def test_device_equals_host(env, rows, width, s):
    half0, half1, fc, ff = random_inputs(rows, width, s, seed=100000 * s + 1000 * rows + width)
    side = env.torch.cuda.Stream()
    for opts in OPTIONS:
        want0, want1 = env.R.upsample_host(half0, half1, fc, ff, scale=s, **opts)
        for stream in (None, side):
            got0, got1 = run_device(env, half0, half1, fc, ff, stream=stream, scale=s, **opts)
            for got, want in ((got0, want0), (got1, want1)):
                assert np.array_equal(bits(got), bits(want)), (opts, stream is not None, int((bits(got) != bits(want)).sum()))
            one, none = run_device(env, half0, None, fc, ff, stream=stream, scale=s, **opts)
            assert none is None and np.array_equal(bits(one), bits(want0)), (opts, stream is not None)


# ---- 9. the device's argument errors -------------------------------------------------------------
def test_device_argument_errors(env):
    from rtclj._lib import rt_upsample_opts
    lib = env.lib
    rows, width, s = 9, 12, 2
    half0, half1, fc, ff = random_inputs(rows, width, s, seed=2)
    d = [dev(env, a) for a in (half0, half1, fc, ff)]
    o0, o1 = nan_buf(env, rows * width * 3), nan_buf(env, rows * width * 3)
    p = [C.c_void_p(t.data_ptr()) for t in d]

    def call(o=None, ins=p, w=width, r=rows, a=C.c_void_p(o0.data_ptr()), b=C.c_void_p(o1.data_ptr())):
        return lib.rt_upsample(None if o is None else C.byref(o), *ins, w, r, a, b, None)

    def refused(code, word):
        return code == -1 and word in lib.rt_last_error()

    for k in (0, 2, 3):
        bad = list(p)
        bad[k] = None
        assert refused(call(ins=bad), b"NULL"), k
    assert refused(call(a=None), b"NULL")
    assert refused(call(ins=[p[0], None, p[2], p[3]]), b"both") and refused(call(b=None), b"both")
    for o, word in ((rt_upsample_opts(1, 0, 0.05), b"scale outside 2..4"), (rt_upsample_opts(5, 0, 0.05), b"scale"),
                    (rt_upsample_opts(2, 9, 0.05), b"normal_pow2 outside 0..8"),
                    (rt_upsample_opts(2, 0, 0.0), b"sigma_z"), (rt_upsample_opts(2, 0, float("nan")), b"sigma_z")):
        assert refused(call(o=o), b"rt_upsample: " + word), lib.rt_last_error()
    for w, r in ((0, rows), (width, -1), (65536, 32768), (1, 4 * 65535 + 1)):
        assert refused(call(w=w, r=r), b"bad width/rows"), (w, r)
    for k in range(4):   # an output may not overlap an input
        assert refused(call(a=p[k]), b"an output overlaps an input"), k
        assert refused(call(b=p[k]), b"an output overlaps an input"), k
    assert refused(call(b=C.c_void_p(o0.data_ptr() + 12)), b"the outputs overlap")
    host = np.zeros(rows * width * 3, np.float32)
    assert refused(call(a=C.c_void_p(host.ctypes.data)), b"not a device pointer")
    env.torch.cuda.synchronize()
    assert np.isnan(o0.cpu().numpy()).all() and np.isnan(o1.cpu().numpy()).all()   # nothing ran
    assert call() == 0
    env.torch.cuda.synchronize()
    want0, want1 = env.R.upsample_host(half0, half1, fc, ff)   # NULL options: the defaults
    assert np.array_equal(bits(o0.cpu().numpy()), bits(want0).reshape(-1))
    assert np.array_equal(bits(o1.cpu().numpy()), bits(want1).reshape(-1))


# ---- 10. the pipeline ------------------------------------------------------------------------------
def rising(R, f, frames):
    """The reference bodies at frame f: the centre sphere rises 0.08 a frame and
    ends at its reference position."""
    bodies = [dict(b) for b in R.hittables]
    bodies[1]["hittable/center"] = (0.0, -0.08 * (frames - 1 - f), -1.2)
    return bodies


def orbit_cameras(R, n):
    """The reference camera turning 0.4 degrees a frame about the vertical."""
    out = []
    for f in range(n):
        ang = np.radians(0.4) * f
        lf = (-2.0 * np.cos(ang) + 1.0 * np.sin(ang), 2.0, 2.0 * np.sin(ang) + 1.0 * np.cos(ang))
        out.append(R.camera(W, H, **{**R.REFERENCE_CAMERA, "look_from": lf}))
    return out


def test_pipeline_equals_hosts(env):
    """render_animation(scale=2) over 3 frames at 160 x 90, 2 + 2 spp per coarse
    pixel, the centre sphere rising under a turning camera: every frame's
    upsampled halves equal upsample_host of the coarse halves and features the
    device resolved, the accumulated halves temporal_host chained over them, the
    frame denoise_host."""
    R = env.R
    cams = orbit_cameras(R, 3)
    scs = [R.Scene.from_bodies(rising(R, f, 3)) for f in range(3)]
    cw, ch = coarse(W, 2), coarse(H, 2)
    prev_cam, prev = None, None
    for f, st in enumerate(R.render_animation(scs, cams, W, H, spp=4, seed=5, stages=True, scale=2)):
        den, h0, h1, feat, acc0, acc1, ids, c0, c1, fc = st
        assert c0.shape == c1.shape == (ch, cw, 3) and fc.shape == (ch, cw, 8) and h0.shape == (H, W, 3)
        assert not any(np.isnan(a).any() for a in (den, h0, h1, acc0, acc1, c0, c1))
        # the coarse frame is the coarsened camera's own frame
        ccam = R.camera_coarsen(cams[f], 2)
        with R.Progressive(scs[f], ccam, cw, ch, seed=5, sample_begin=4 * f) as a0:
            a0.add(2)
            assert np.array_equal(bits(a0.frame()), bits(c0)), f
        up0, up1 = R.upsample_host(c0, c1, fc, feat, scale=2)
        assert np.array_equal(bits(h0), bits(up0)) and np.array_equal(bits(h1), bits(up1)), f
        assert np.array_equal(ids, R.ids_host(scs[f], cams[f], W, H)), f
        motion = R.body_motion(scs[f], scs[f - 1]) if f else np.zeros((5, 4), np.float32)
        want0, want1, length = R.temporal_host(cams[f], prev_cam, up0, up1, feat, prev=prev, ids=ids, motion=motion)
        assert np.array_equal(bits(acc0), bits(want0)) and np.array_equal(bits(acc1), bits(want1)), f
        assert np.array_equal(bits(den), bits(R.denoise_host(want0, want1, feat))), f
        prev_cam, prev = cams[f], (want0, want1, np.ascontiguousarray(feat[..., 3:7]), length)
    assert f == 2
    # without `scale` the calls are what they were: seven items, the full-size halves
    plain = next(R.render_animation(scs, cams, W, H, spp=4, seed=5, stages=True))
    assert len(plain) == 7 and plain[1].shape == (H, W, 3)
    with pytest.raises(ValueError, match="scale and budget"):
        next(R.render_animation(scs, cams, W, H, scale=2, budget=dict(half_spp=2)))
    with pytest.raises(R.RTError):
        next(R.render_animation(scs, cams, W, H, spp=4, scale=5))


# ---- 11. the hosts -----------------------------------------------------------------------------------
def test_render_upscaled_and_rt_main(env, tmp_path):
    import pngdec
    R, torch = env.R, env.torch
    den, mean, feat = R.render_upscaled(env.sc, env.cam, W, H, spp=8, scale=2, seed=3)
    assert den.shape == mean.shape == (H, W, 3) and feat.shape == (H, W, 8)
    assert den.dtype == mean.dtype == feat.dtype == np.float32 and np.isfinite(den).all() and np.isfinite(mean).all()
    # the same steps by hand
    cw, ch = coarse(W, 2), coarse(H, 2)
    ccam = R.camera_coarsen(env.cam, 2)
    with R.Progressive(env.sc, ccam, cw, ch, seed=3) as a0, R.Progressive(env.sc, ccam, cw, ch, seed=3, sample_begin=4) as a1, \
            R.Features(env.sc, ccam, cw, ch, seed=3) as fc, R.Features(env.sc, env.cam, W, H, seed=3) as ft:
        a0.add(4), a1.add(4), fc.add(8), ft.add(8)
        h0, h1, fcf, fff = a0.frame(), a1.frame(), fc.frame(), ft.frame()
    assert np.array_equal(bits(feat), bits(fff))
    up0, up1 = R.upsample_host(h0, h1, fcf, fff, scale=2)
    assert np.array_equal(bits(mean), bits(np.float32(0.5) * (up0 + up1)))
    want = R.denoise_host(up0, up1, fff)
    assert np.array_equal(bits(den), bits(want))
    st = R.render_upscaled(env.sc, env.cam, W, H, spp=8, scale=2, seed=3, stages=True)
    assert len(st) == 7 and np.array_equal(bits(st[1]), bits(up0)) and np.array_equal(bits(st[4]), bits(h0))
    # other options reach the kernel and the filter
    den3, _, _ = R.render_upscaled(env.sc, env.cam, W, H, spp=8, scale=3, seed=3, upsample=dict(normal_pow2=2), levels=3)
    assert den3.shape == (H, W, 3) and np.isfinite(den3).all() and not np.array_equal(den3, den)
    torch.cuda.synchronize()
    # rt_main --denoise --scale 2, a fresh child process
    assert RT_MAIN.exists(), "lib/rt_main is not built (make -C raytracing-clj_amd)"
    child = dict(os.environ)
    child.pop("RTCLJ_LIBRARY", None)
    r = subprocess.run([str(RT_MAIN), "8", "50", "--width", str(W), "--gpus", "1", "--no-png", "--seed", "3",
                        "--denoise", "up", "--scale", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                       env=child)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    q = R.write_color(den)
    assert np.array_equal(R.read_ppm(tmp_path / "up.denoised.ppm"), q)
    png, _ = pngdec.decode((tmp_path / "up.denoised.png").read_bytes())
    assert np.array_equal(png, q)
    for bad in (["--scale", "2"], ["--denoise", "bad", "--scale", "5"]):
        r = subprocess.run([str(RT_MAIN), "8", "50", "--width", str(W), "--gpus", "1", "--no-png", *bad], cwd=tmp_path,
                           capture_output=True, text=True, timeout=120, env=child)
        assert r.returncode == 2 and "--scale" in r.stderr, (bad, r.returncode, r.stderr)
    assert not (tmp_path / "bad.denoised.ppm").exists()


# ---- 12. quality and footprint on the device's own frames -------------------------------------------
class DeviceFrames:
    """test_upsample_host's frame source on the device: rt_launch_accum and
    rt_launch_feat (which equal the oracle's mirror bit for bit)."""

    def __init__(self, env):
        self.env = env

    def render(self, cam, w, h, spp, seed, sample_begin=0):
        with self.env.R.Progressive(self.env.sc, cam, w, h, seed=seed, sample_begin=sample_begin) as a:
            a.add(spp)
            return a.frame()

    def features(self, cam, w, h, spp, seed):
        with self.env.R.Features(self.env.sc, cam, w, h, seed=seed) as ft:
            ft.add(spp)
            return ft.frame()


@pytest.mark.parametrize("which", ("reference", "pinhole"))
def test_quality_on_the_device(env, which):
    """tests/test_upsample_host.py's test 6 with the device's frames and the
    kernel's own reconstruction, under the same thresholds."""
    q = T.quality_setup(which, DeviceFrames(env))
    n = T.quality_numbers(q)
    print(which, n)
    g0, g1 = run_device(env, q["h0"], q["h1"], q["fc"], q["ff"], scale=T.S)
    h0, h1 = env.R.upsample_host(q["h0"], q["h1"], q["fc"], q["ff"], scale=T.S)
    assert np.array_equal(bits(g0), bits(h0)) and np.array_equal(bits(g1), bits(h1))
    assert n["edge_pixels"] > 1000
    assert n["ratio"] < T.RATIO_BOUND[which], n
    if which == "pinhole":
        assert n["ratio_demodulated"] < T.DEMOD_BOUND_PINHOLE, n


def test_footprint_on_the_device(env):
    """tests/test_upsample_host.py's test 7 with rt_launch_accum's frames, under the same threshold."""
    a, control = T.footprint_numbers(DeviceFrames(env))
    print("A / D", a, "control", control)
    assert a < T.FOOTPRINT_MIDPOINT < control, (a, control)


# ---- 13. what a render scale costs (reported, not asserted) ----------------------------------------
def test_report_error_against_sample_count(env):
    """RMSE of the denoised 160 x 90 reference frame against a 1024-spp render
    (seed 77), seeds 1-3: render_upscaled at scale 2 and 8 spp per coarse
    pixel; render_denoised at 2 spp per pixel (the same number of samples);
    render_denoised at 8 spp (four times the samples).  Run with -s; the
    figures stand in DESIGN.md §3.14."""
    R = env.R
    truth = R.render(env.sc, env.cam, W, H, spp=1024, seed=77, n_devices=1).astype(np.float64)

    def rmse(img):
        return float(np.sqrt(((img.astype(np.float64) - truth) ** 2).mean()))

    rows = []
    for seed in (1, 2, 3):
        rows.append((rmse(R.render_upscaled(env.sc, env.cam, W, H, spp=8, scale=2, seed=seed)[0]),
                     rmse(R.render_denoised(env.sc, env.cam, W, H, spp=2, seed=seed)[0]),
                     rmse(R.render_denoised(env.sc, env.cam, W, H, spp=8, seed=seed)[0])))
    for seed, r in zip((1, 2, 3), rows):
        print("seed %d: scale 2 at 8 spp %.5f, full size at 2 spp %.5f, full size at 8 spp %.5f" % (seed, *r))
    print("means: %.5f %.5f %.5f" % tuple(np.mean(rows, axis=0)))
    assert np.isfinite(rows).all()
