"""The colour clamp of temporal accumulation on the host (include/rt.h,
rt_temporal_host_clamp; no GPU needed): bit-equality with a NumPy restatement
of rt.h's definition over chained steps, gamma = +inf as the unclamped steps, a
constructed colour jump (with the unclamped step as the control), the argument
errors, its quality against the fp64 oracle under a mirror that shows a moving
sphere (with a still scene and gamma = 0.25 as the controls), the stand-alone
sanitizer program and the presence of the new entries.
"""
import ctypes as C
import functools
import inspect
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_motion_host as M
import test_temporal_host as T
from test_denoise_host import analytic_guides, bits

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "clamp_check"
F = np.float32
INF = F(np.inf)
CLAMP_FUNCS = ("rt_temporal_step_clamp", "rt_temporal_host_clamp")
SIZES = ((1, 1), (1, 9), (9, 1), (5, 7), (17, 33))   # rows x width
GAMMAS = (0.25, 1.0, 2.5)
DEFAULT_GAMMA, DEFAULT_RADIUS = 1.0, 2


# ---- rt.h's definition in NumPy: float32 element-wise operations in the stated
# order, the taps as fancy-indexed gathers with masks ---------------------------
def box_np(half0, half1, feat, radius=DEFAULT_RADIUS, gamma=DEFAULT_GAMMA, sigma_z=0.1, normal_min=0.9):
    """(lo, hi), (rows, width, 3) each: the colour box of every pixel."""
    rows, width = feat.shape[:2]
    sigma_z, normal_min, gamma = F(sigma_z), F(normal_min), F(gamma)
    z, n = feat[..., 6], feat[..., 3:6]
    y, x = np.mgrid[0:rows, 0:width]
    with np.errstate(all="ignore"):
        pinf, pfin, tol = z == INF, np.isfinite(z), sigma_z * z
        s1, s2 = np.zeros((rows, width, 3), np.float32), np.zeros((rows, width, 3), np.float32)
        cnt = np.zeros((rows, width), np.float32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qx, qy = x + dx, y + dy
                inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
                ix, iy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                zq, nq = z[iy, ix], n[iy, ix]
                dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                same = (pinf & (zq == INF)) | (pfin & np.isfinite(zq) & (np.abs(zq - z) <= tol) & (dot >= normal_min))
                valid = inside & (same if (dx or dy) else True)
                for half in (half0, half1):
                    v = half[iy, ix]
                    s1 = np.where(valid[..., None], s1 + v, s1)
                    s2 = np.where(valid[..., None], s2 + v * v, s2)
                    cnt = np.where(valid, cnt + F(1), cnt)
        mean = s1 / cnt[..., None]
        var = s2 / cnt[..., None] - mean * mean
        var = np.where(var > 0, var, F(0))
        e = gamma * np.sqrt(var)
        lo, hi = mean - e, mean + e
    assert lo.dtype == hi.dtype == np.float32
    return lo, hi


def step_np(cam, prev_cam, half0, half1, feat, prev=None, row0=0, ids=None, motion=None, clamp=None, max_history=32,
            sigma_z=0.1, normal_min=0.9):
    """rt.h's step -- with 2' when ids are given, with the clamp in step 6 when
    `clamp` is a dict -- in NumPy (steps 4-6 as test_temporal_host.temporal_np
    states them)."""
    rows, width = half0.shape[:2]
    if prev_cam is None:
        return half0.copy(), half1.copy(), np.ones((rows, width), np.float32)
    a0, a1, guide, length = prev
    mh = F(float(max_history))
    with np.errstate(all="ignore"):
        if ids is None:
            hist, fx, fy, zexp = T.reproject_np(cam, prev_cam, feat, row0)
        else:
            hist, fx, fy, zexp = M.reproject_motion_np(cam, prev_cam, feat, row0, ids, motion)
        x0, tx = T.split_np(fx, hist)
        y0, ty = T.split_np(fy, hist)
        tol = F(sigma_z) * zexp
        pinf, pfin = zexp == INF, np.isfinite(zexp)
        acc0, acc1 = np.zeros_like(half0), np.zeros_like(half1)
        accl, bsum = np.zeros((rows, width), np.float32), np.zeros((rows, width), np.float32)
        for dy in (0, 1):
            for dx in (0, 1):
                b = (tx if dx else F(1) - tx) * (ty if dy else F(1) - ty)
                qx, qy = x0 + dx, y0 + dy
                inside = hist & (b != 0) & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
                ix, iy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                lq, gq = length[iy, ix], guide[iy, ix]
                zq = gq[..., 3]
                dot = (feat[..., 3] * gq[..., 0] + feat[..., 4] * gq[..., 1]) + feat[..., 5] * gq[..., 2]
                valid = inside & (lq >= 1) & ((pinf & (zq == INF)) | (pfin & np.isfinite(zq) & (np.abs(zq - zexp) <= tol) &
                                                                     (dot >= F(normal_min))))
                acc0 = np.where(valid[..., None], acc0 + b[..., None] * a0[iy, ix], acc0)
                acc1 = np.where(valid[..., None], acc1 + b[..., None] * a1[iy, ix], acc1)
                accl = np.where(valid, accl + b * lq, accl)
                bsum = np.where(valid, bsum + b, bsum)
        accept = hist & (bsum >= F(0.25))
        h0, h1, lh = acc0 / bsum[..., None], acc1 / bsum[..., None], accl / bsum
        if clamp is not None:
            lo, hi = box_np(half0, half1, feat, clamp.get("radius", DEFAULT_RADIUS), clamp.get("gamma", DEFAULT_GAMMA),
                            sigma_z, normal_min)
            h0 = np.where(h0 < lo, lo, np.where(h0 > hi, hi, h0))
            h1 = np.where(h1 < lo, lo, np.where(h1 > hi, hi, h1))
        n = np.where(lh + F(1) < mh, lh + F(1), mh)
        k = F(1) / n
        out0 = np.where(accept[..., None], h0 + k[..., None] * (half0 - h0), half0)
        out1 = np.where(accept[..., None], h1 + k[..., None] * (half1 - h1), half1)
        out_len = np.where(accept, n, F(1))
    assert out0.dtype == out1.dtype == out_len.dtype == np.float32
    return out0, out1, out_len


def host(cam, prev_cam, half0, half1, feat, prev=None, row0=0, ids=None, motion=None, clamp=None, **opts):
    from rtclj import raytracing as R
    return R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, ids=ids, motion=motion, clamp=clamp,
                           **opts)


def chain_inputs(rows, width, row0, steps=4):
    """Per step (cam, half0, half1, feat, ids, motion), and the history and
    camera before the first: smooth_inputs' frames (sky pixels, depth edges,
    shortened normals) with a patch of one colour in both halves (sd = 0)."""
    pairs = T.camera_pairs(width, rows + row0 + 3)
    base = pairs["still"][0]
    cams = [base, pairs["pan"][1], pairs["pan"][1], pairs["rotation"][1]][:steps]
    frames = []
    for s, cam in enumerate(cams):
        half0, half1, feat = T.smooth_inputs(rows, width, seed=1000 * rows + width + 31 * s)
        r1, c1 = max(1, (2 * rows) // 3), max(1, (2 * width) // 3)
        half0[:r1, :c1] = half1[:r1, :c1] = (F(0.3), F(0.7), F(1.1))
        if s == 2:   # the same surface and colour everywhere: every window has sd = 0
            feat[..., 3:6], feat[..., 6], feat[..., 7] = (0.0, 0.6, 0.8), 9.0, 1.0
            half0[...] = half1[...] = F(0.6)
        ids, motion = M.random_motion(rows, width, seed=3 * rows + width + s)
        frames.append((cam, half0, half1, feat, ids, motion))
    return base, T.random_history(frames[0][3], seed=rows + 7 * width), frames


# ---- 1. bit-equality with the definition, 2. gamma = +inf ----------------------------
@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("row0", (0, 3))
@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("with_ids", (False, True))
def test_host_equals_the_definition(rows, width, row0, radius, with_ids):
    base, first, frames = chain_inputs(rows, width, row0)
    clamped = 0
    for gamma in GAMMAS:
        clamp = dict(radius=radius, gamma=gamma)
        prev_cam, prev = base, first
        for s, (cam, half0, half1, feat, ids, motion) in enumerate(frames):
            kw = dict(prev=prev, row0=row0, ids=ids if with_ids else None, motion=motion if with_ids else None)
            keep = [a.copy() for a in (half0, half1, feat, ids, motion) + tuple(prev)]
            got = host(cam, prev_cam, half0, half1, feat, clamp=clamp, **kw)
            want = step_np(cam, prev_cam, half0, half1, feat, clamp=clamp, **kw)
            for g, w, what in zip(got, want, ("out0", "out1", "out_len")):
                assert g.shape == w.shape and np.isfinite(g).all()
                assert np.array_equal(bits(g), bits(w)), (gamma, s, what, int((bits(g) != bits(w)).sum()), g.size)
            for a, k in zip((half0, half1, feat, ids, motion) + tuple(prev), keep):
                assert np.array_equal(a.view(np.uint32), k.view(np.uint32))   # the inputs are never written
            free = step_np(cam, prev_cam, half0, half1, feat, **kw)
            clamped += int((bits(got[0]) != bits(free[0])).any(axis=-1).sum())
            assert np.array_equal(bits(got[2]), bits(free[2]))                # N and the stored L are unchanged
            prev_cam, prev = cam, (got[0], got[1], np.ascontiguousarray(feat[..., 3:7]), got[2])
    print(f"{rows} x {width} row0 {row0} radius {radius} ids {with_ids}: pixels the clamp changed, all steps: {clamped}")
    if rows * width >= 35:
        assert clamped > 0     # the inputs are not blind to the clamp


@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("row0", (0, 3))
@pytest.mark.parametrize("with_ids", (False, True))
def test_infinite_gamma_is_the_unclamped_step(rows, width, row0, with_ids):
    base, first, frames = chain_inputs(rows, width, row0)
    for radius in (1, 2, 3):
        prev_cam, prev = base, first
        for cam, half0, half1, feat, ids, motion in frames:
            if with_ids:
                want = M.host(cam, prev_cam, half0, half1, feat, ids, motion, prev=prev, row0=row0)
            else:
                want = T.host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0)
            got = host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, ids=ids if with_ids else None,
                       motion=motion if with_ids else None, clamp=dict(radius=radius, gamma=float("inf")))
            for g, w in zip(got, want):
                assert np.array_equal(bits(g), bits(w)), radius
            prev_cam, prev = cam, (got[0], got[1], np.ascontiguousarray(feat[..., 3:7]), got[2])


def test_no_previous_camera_and_null_options():
    from rtclj._lib import fptr, lib
    half0, half1, feat = T.smooth_inputs(13, 17, seed=5)
    cam = T.cam_of(17, 13)
    out0, out1, length = host(cam, None, half0, half1, feat, clamp={})
    assert np.array_equal(bits(out0), bits(half0)) and np.array_equal(bits(out1), bits(half1)) and (length == 1).all()
    # NULL options are the defaults, of the step and of the clamp
    prev = T.random_history(feat, seed=9)
    o0, o1, ol = np.empty_like(half0), np.empty_like(half0), np.empty((13, 17), np.float32)
    pan = T.camera_pairs(17, 13)["pan"][1]
    assert lib.rt_temporal_host_clamp(None, None, C.byref(pan), C.byref(cam), 17, 13, 0, fptr(half0), fptr(half1),
                                      fptr(feat), *(fptr(a) for a in prev), None, None, 0, fptr(o0), fptr(o1),
                                      fptr(ol)) == 0
    want = step_np(pan, cam, half0, half1, feat, prev=prev, clamp=dict(radius=DEFAULT_RADIUS, gamma=DEFAULT_GAMMA))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((o0, o1, ol), want))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(host(pan, cam, half0, half1, feat, prev=prev, clamp={}),
                                                                want))


# ---- 3. a colour jump against a long history --------------------------------------------
def test_colour_jump_is_followed_and_the_rest_is_untouched():
    """A still camera over one plane; the history holds 0.5 in both halves with
    L = 20; the current halves are 0.5 plus noise of sample deviation 0.02,
    and inside one rectangle 0.5 + 10 * 0.02 plus the same noise."""
    H, W, sd, old, L = T.H, T.W, 0.02, F(0.5), 20.0
    cam = T.plane_cameras(0)[0]
    feat = T.plane_feat(T.plane_depth(cam))
    rng = np.random.default_rng(12)
    half0 = (old + rng.normal(0.0, sd, (H, W, 3))).astype(np.float32)
    half1 = (old + rng.normal(0.0, sd, (H, W, 3))).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W]
    rect = (y >= 30) & (y < 60) & (x >= 50) & (x < 90)
    inner = (y >= 32) & (y < 58) & (x >= 52) & (x < 88)      # the window lies inside the rectangle
    far = ~((y >= 28) & (y < 62) & (x >= 48) & (x < 92))     # the window does not touch it
    half0[rect] += F(10 * sd)
    half1[rect] += F(10 * sd)
    prev = (np.full((H, W, 3), old), np.full((H, W, 3), old), np.ascontiguousarray(feat[..., 3:7]),
            np.full((H, W), L, np.float32))
    got0, got1, gl = host(cam, cam, half0, half1, feat, prev=prev, clamp={})
    free0, free1, fl = T.host(cam, cam, half0, half1, feat, prev=prev)
    assert (gl == L + 1).all() and (fl == L + 1).all()
    k = F(1) / F(L + 1)
    lo, hi = box_np(half0, half1, feat)
    # inside, the history is below the box and is moved to its lower edge ...
    assert (lo[inner] > old + F(8 * sd)).all()
    for got, half in ((got0, half0), (got1, half1)):
        assert np.array_equal(bits(got[inner]), bits((lo + k * (half - lo))[inner]))
        # ... so the result lies between the box and the current sample
        assert (got[inner] >= np.minimum(lo, half)[inner]).all() and (got[inner] <= np.maximum(hi, half)[inner]).all()
        assert np.abs(got[inner] - (old + F(10 * sd))).max() < 3 * sd
    # the rest: wherever the old colour lies inside the pixel's box, the unclamped step's bits
    rest = ((lo <= old) & (old <= hi)).all(axis=-1)
    assert not rest[inner].any() and rest[far].mean() > 0.95
    for got, free in ((got0, free0), (got1, free1)):
        assert np.array_equal(bits(got[rest]), bits(free[rest]))
    # the control: the unclamped step stays within 1 / N of the old colour, inside the rectangle too
    for free, half in ((free0, half0), (free1, half1)):
        assert (np.abs(free - old) <= np.abs(half - old) * k * F(1 + 1e-5) + F(1e-7)).all()
        assert np.abs(free[inner] - old).max() < 1.5 * sd and np.abs(free[inner] - (old + F(10 * sd))).min() > 8 * sd


# ---- 4. arguments ------------------------------------------------------------------------
def test_argument_errors():
    from rtclj._lib import fptr, i32ptr, lib, rt_temporal_clamp_opts
    from rtclj import raytracing as R
    rows, width = 5, 6
    half0, half1, feat = T.smooth_inputs(rows, width, seed=3)
    prev = T.random_history(feat, seed=4)
    ids, motion = M.random_motion(rows, width, seed=5)
    cam = T.cam_of(width, rows)
    out = [np.full_like(half0, 7.0), np.full_like(half0, 7.0), np.full((rows, width), 7.0, np.float32)]
    ok = [None, None, C.byref(cam), C.byref(cam), width, rows, 0, fptr(half0), fptr(half1), fptr(feat)] + \
         [fptr(a) for a in prev] + [i32ptr(ids), fptr(motion), M.N_BODIES] + [fptr(a) for a in out]
    assert len(ok) == 20 and lib.rt_temporal_host_clamp(*ok) == 0
    done = [a.copy() for a in out]

    def refused(args, word):
        for a in out:
            a[...] = 7.0
        assert lib.rt_temporal_host_clamp(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert all((a == 7.0).all() for a in out)            # nothing was written

    for k in (2, 7, 8, 9, 10, 11, 12, 13, 15, 17, 18, 19):
        bad = list(ok)
        bad[k] = None
        refused(bad, b"NULL")
    refused(ok[:16] + [-1] + ok[17:], b"n_bodies")
    no_ids = list(ok)
    no_ids[14], no_ids[15], no_ids[16] = None, None, -5         # without ids the table and its length are not read
    assert lib.rt_temporal_host_clamp(*no_ids) == 0
    want = host(cam, cam, half0, half1, feat, prev=prev, clamp={})
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, want))
    no_prev = list(ok)
    no_prev[3] = no_prev[10] = no_prev[11] = no_prev[12] = no_prev[13] = None
    assert lib.rt_temporal_host_clamp(*no_prev) == 0
    good = rt_temporal_clamp_opts(radius=DEFAULT_RADIUS, gamma=DEFAULT_GAMMA)
    assert lib.rt_temporal_host_clamp(ok[0], C.byref(good), *ok[2:]) == 0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, done))
    for radius in (0, 4, -1, 1 << 30):
        refused([None, C.byref(rt_temporal_clamp_opts(radius=radius, gamma=1.0))] + ok[2:], b"radius")
    for gamma in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
        refused([None, C.byref(rt_temporal_clamp_opts(radius=2, gamma=gamma))] + ok[2:], b"gamma")
    for gamma in (float("inf"), 1e-42, 3e38):
        assert lib.rt_temporal_host_clamp(None, C.byref(rt_temporal_clamp_opts(radius=2, gamma=gamma)), *ok[2:]) == 0
    from rtclj._lib import rt_temporal_opts
    refused([C.byref(rt_temporal_opts(max_history=0, sigma_z=0.1, normal_min=0.9))] + ok[1:], b"max_history")
    for w_, r_ in ((0, rows), (width, 0), (1 << 16, 1 << 16)):
        refused(ok[:4] + [w_, r_, 0] + ok[7:], b"width/rows")
    refused(ok[:6] + [-1] + ok[7:], b"row0")
    for k in (17, 18):     # an output may not overlap an input, the history, the ids or the table
        for alias in (half0, half1, feat, prev[0], prev[2], ids, motion):
            bad = list(ok)
            bad[k] = C.cast(alias.ctypes.data, C.POINTER(C.c_float))
            keep = alias.copy()
            assert lib.rt_temporal_host_clamp(*bad) == -1 and b"overlap" in lib.rt_last_error()
            assert np.array_equal(alias.view(np.uint32), keep.view(np.uint32))
    bad = list(ok)
    bad[18] = bad[17]
    refused(bad, b"overlap")
    # the device entry refuses a NULL handle before any device call
    assert lib.rt_temporal_step_clamp(None, None, None, None, None, None, None, None, None, 0, None, None, None) == -1
    assert b"NULL" in lib.rt_last_error()
    # the Python layer
    with pytest.raises(TypeError):
        R.temporal_host(cam, None, half0, half1, feat, clamp=dict(sigma=1.0))
    with pytest.raises(R.RTError):
        R.temporal_host(cam, None, half0, half1, feat, clamp=dict(radius=0))
    with pytest.raises(R.RTError):
        R.temporal_host(cam, None, half0, half1, feat, clamp=dict(gamma=float("nan")))
    with pytest.raises(TypeError):
        next(R.render_sequence(R.hittables, [cam], 16, 9, spp=2, clamp=dict(width=3)))
    with pytest.raises(TypeError):
        next(R.render_animation([R.hittables], [cam], 16, 9, spp=2, clamp=dict(width=3)))


# ---- 5. quality, against the fp64 oracle -----------------------------------------------------
# MSE(clamped motion chain + denoiser) / MSE(rt_temporal_host_motion chain + denoiser), seeds 1-3, as
# measured by quality_ratios() below.
#   moving sphere, over the mirror's pixels (id 4), at the default gamma:
MEASURED_MIRROR = (0.2529, 0.3236, 0.2985)
#   still scene, over all pixels, at the default gamma and at gamma = 0.25 (the negative control):
MEASURED_STILL = (0.9203, 0.9456, 0.9058)
MEASURED_STILL_CONTROL = (1.0279, 1.0697, 1.0084)
#   still scene, every candidate of the default (gamma: seeds 1-3).  The default is the smallest
#   whose ratio is on all three seeds nearer to 1 than to the control's.  The control harms little
#   here (eight frames of 2 + 2 spp are worth about what a 5 x 5 window of the current frame is), so
#   "the control's ratio" matters: held against the same seed's control ratio 0.5 would pass; held
#   against every seed's -- so also the smallest, 1.0084, the one the no-harm bound is built on --
#   0.5 fails on seed 2 (1.0232 is nearer to 1.0084 than to 1) and 1.0 is the smallest that passes.
#   The stricter reading is the one taken.
MEASURED_STILL_CANDIDATES = {0.5: (0.9735, 1.0232, 0.9722), 1.0: (0.9203, 0.9456, 0.9058),
                             1.5: (0.8991, 0.9171, 0.8882), 2.0: (0.8960, 0.9122, 0.8878),
                             3.0: (0.8970, 0.9118, 0.9314)}
#   moving sphere, the mirror's pixels, the other candidates, for the record (not asserted):
#   0.25: 0.0585 0.0897 0.0726; 0.5: 0.1065 0.1544 0.1320; 1.5: 0.3854 0.4641 0.4483;
#   2.0: 0.4829 0.5661 0.5541; 3.0: 0.5996 0.6770 0.6709


def mirror_bodies(f, moving, frames=8):
    """The reference bodies with the right sphere a mirror (fuzz 0); `moving`:
    the centre sphere rising as test_motion_host.rising."""
    from rtclj import raytracing as R
    bodies = M.rising(f, frames) if moving else [dict(b) for b in R.hittables]
    bodies[4] = {**bodies[4], "material/fuzz": 0.0}
    return bodies


@functools.lru_cache(maxsize=None)
def quality_ratios(moving, gammas):
    """Per gamma of `gammas` the three seeds' MSE(clamped chain + denoiser) /
    MSE(unclamped motion chain + denoiser) -- over the last frame's pixels with
    id 4 if `moving`, else over all pixels -- and the least share of those
    pixels with L >= 4 over the chains."""
    import oracle
    from rtclj import raytracing as R
    from test_denoise_host import host as denoise
    w, h, frames = 160, 90, 8
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    bodies = [mirror_bodies(f, moving, frames) for f in range(frames)]
    scenes = [R.Scene.from_bodies(b) for b in bodies]
    flat = [R.flatten64(b) for b in bodies]
    feats = [analytic_guides(*fl, cam, w, h) for fl in flat]
    ids = [R.ids_host(sc, cam, w, h) for sc in scenes]
    motions = [None] + [R.body_motion(scenes[f], scenes[f - 1]) for f in range(1, frames)]
    ref = oracle.render(oracle.MODE_REF64D, *flat[-1], cam.as_list(), cam.defocus, w, h, 1024, 50,
                        seed=77)[0].astype(np.float64)
    mask = ids[-1] == 4 if moving else np.ones((h, w), bool)
    assert mask.sum() > 400
    ratios, long_share = {g: [] for g in gammas}, 1.0
    for seed in (1, 2, 3):
        prev_cam, prevs = None, {g: None for g in (None,) + gammas}
        for f in range(frames):
            args = (*flat[f], cam.as_list(), cam.defocus, w, h)
            h0 = oracle.render(oracle.MODE_REF64D, *args, 2, 50, seed=seed, sample_begin=4 * f)[0]
            h1 = oracle.render(oracle.MODE_REF64D, *args, 2, 50, seed=seed, sample_begin=4 * f + 2)[0]
            guide = np.ascontiguousarray(feats[f][..., 3:7])
            for g in prevs:
                o0, o1, ln = host(cam, prev_cam, h0, h1, feats[f], prev=prevs[g], ids=ids[f], motion=motions[f],
                                  clamp=None if g is None else dict(gamma=g))
                prevs[g] = (o0, o1, guide, ln)
            prev_cam = cam
        mse = {}
        for g, (o0, o1, _, ln) in prevs.items():
            mse[g] = float(((denoise(o0, o1, feats[-1]) - ref)[mask] ** 2).mean())
            long_share = min(long_share, float((ln[mask] >= 4).mean()))
        for g in gammas:
            ratios[g].append(mse[g] / mse[None])
    return ratios, long_share


def midpoint(a, b):
    return 0.5 * (a + b)


def test_quality_under_a_mirror_that_shows_a_moving_sphere():
    """The reference scene with the right sphere a mirror, 160 x 90, the still
    reference camera, eight frames, the centre sphere rising 0.08 a frame;
    2 + 2 spp a frame (MODE_REF64D), analytic guides, ids from ids_host,
    displacements from body_motion; against 1024 spp of the last scene at seed
    77, over the last frame's pixels with id 4 (the mirror, which shows the
    sphere).  MSE(clamped motion chain, then the denoiser) /
    MSE(rt_temporal_host_motion chain, then the denoiser), seeds 1, 2, 3, at the
    default gamma -- measured: see MEASURED_MIRROR; asserted: each below the
    midpoint between the largest of them and 1, 0.6618 (DESIGN.md §3.12 records
    them).
    At least 80 % of those pixels must have L >= 4 in both chains, or the test
    measures restarts and not the clamp."""
    ratios, long_share = quality_ratios(True, (DEFAULT_GAMMA,))
    print("mirror, moving sphere: MSE(clamped) / MSE(unclamped), seeds 1-3:", ["%.4f" % r for r in ratios[DEFAULT_GAMMA]],
          "; least share of its pixels with L >= 4: %.4f" % long_share)
    assert long_share >= 0.8, long_share
    bound = midpoint(max(MEASURED_MIRROR), 1.0)
    assert all(r < bound for r in ratios[DEFAULT_GAMMA]), (ratios, bound)


def test_quality_no_harm_on_a_still_scene():
    """The same frames with the centre sphere not moving, over all pixels: the
    same ratio at the default gamma and at gamma = 0.25, the negative control
    that clamps into the noise -- measured: see MEASURED_STILL and
    MEASURED_STILL_CONTROL; asserted: each default-gamma ratio below the
    midpoint between the largest of them and the smallest control ratio,
    0.9770."""
    ratios, long_share = quality_ratios(False, (DEFAULT_GAMMA, 0.25))
    print("still scene: MSE(clamped) / MSE(unclamped), seeds 1-3: default gamma", ["%.4f" % r for r in ratios[DEFAULT_GAMMA]],
          "; gamma 0.25", ["%.4f" % r for r in ratios[0.25]], "; least share of pixels with L >= 4: %.4f" % long_share)
    assert long_share >= 0.8, long_share
    bound = midpoint(max(MEASURED_STILL), min(MEASURED_STILL_CONTROL))
    assert all(r < bound for r in ratios[DEFAULT_GAMMA]), (ratios, bound)


def test_the_default_gamma_is_the_recorded_choice():
    """rt.h's default, the binding's and the one the recorded measurements
    select: the smallest candidate whose still-scene ratio is, on all three
    seeds, nearer to 1 than to any seed's control ratio (see the note at
    MEASURED_STILL_CANDIDATES)."""
    from rtclj import _lib
    hdr = (ROOT / "include" / "rt.h").read_text()
    assert _lib.TEMPORAL_CLAMP_DEFAULTS == dict(radius=DEFAULT_RADIUS, gamma=DEFAULT_GAMMA)
    assert re.search(r"radius\s+2\s+1\.\.3", hdr) and re.search(r"gamma\s+%s\s+> 0" % re.escape(repr(DEFAULT_GAMMA)), hdr)
    assert sorted(MEASURED_STILL_CANDIDATES) == [0.5, 1.0, 1.5, 2.0, 3.0]
    passing = [g for g, rs in sorted(MEASURED_STILL_CANDIDATES.items())
               if all(abs(r - 1.0) < abs(r - c) for r in rs for c in MEASURED_STILL_CONTROL)]
    assert passing and passing[0] == DEFAULT_GAMMA, passing
    assert tuple(MEASURED_STILL_CANDIDATES[DEFAULT_GAMMA]) == MEASURED_STILL


# ---- 6. the sanitizers, stand-alone -----------------------------------------------------------
def test_sanitizer_program_exits_clean():
    """lib/clamp_check: csrc/temporal.h (rt_temporal_host_clamp's body with
    tp_clamp_box, the text temporal_box_kernel runs) under
    -fsanitize=address,undefined,float-cast-overflow with hostile inputs, a
    program of its own."""
    assert TOOL.exists(), "lib/clamp_check is not built (make -C raytracing-clj_amd)"
    r = subprocess.run([str(TOOL)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["bad_status"] == 0 and rep["bad_len"] == 0 and rep["bad_identity"] == 0
    assert rep["calls"] > 1000 and rep["refused"] > 0 and rep["accepted"] > 1000 and rep["pixels"] > 100_000
    assert rep["identity_calls"] > 100
    mk = (ROOT / "raytracing-clj_amd" / "Makefile").read_text()
    rule = mk[mk.index("$(OUT)/clamp_check:"):]
    assert "-fsanitize=address,undefined,float-cast-overflow" in rule[:700] and "-fno-sanitize-recover=all" in rule[:700]
    assert "-static-libasan" in rule[:700] and "clamp_check" in mk[mk.index("all:"):mk.index("all:") + 400]


# ---- presence -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["product", "diag"])
def test_symbols_and_signatures(which):
    import rtclj
    from rtclj import _lib
    dll = C.CDLL(str(rtclj.library_path if which == "product" else _lib.diag_library_path))
    hdr = (ROOT / "include" / "rt.h").read_text()
    for name in CLAMP_FUNCS:
        assert hasattr(dll, name), name
        assert name in _lib.SIGNATURES and name in _lib.ADDITIVE
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    assert re.search(r"typedef struct rt_temporal_clamp_opts", hdr)
    assert C.sizeof(_lib.rt_temporal_clamp_opts) == 8 and C.sizeof(_lib.rt_temporal_opts) == 12
    assert len(_lib.SIGNATURES["rt_temporal_step_clamp"][1]) == 13 and len(_lib.SIGNATURES["rt_temporal_host_clamp"][1]) == 20
    # the existing entries keep their argument lists
    assert len(_lib.SIGNATURES["rt_temporal_step"][1]) == 9 and len(_lib.SIGNATURES["rt_temporal_host"][1]) == 16
    assert len(_lib.SIGNATURES["rt_temporal_step_motion"][1]) == 12
    assert len(_lib.SIGNATURES["rt_temporal_host_motion"][1]) == 19


def test_python_host_exposes_the_clamp():
    from rtclj import raytracing as R
    for fn in (R.temporal_host, R.Temporal.step, R.render_sequence, R.render_animation):
        p = inspect.signature(fn).parameters
        assert "clamp" in p and p["clamp"].default is None, fn
