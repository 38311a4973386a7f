"""Temporal accumulation on the host (include/rt.h, rt_temporal_host; no GPU
needed): bit-equality with a NumPy restatement of rt.h's definition, the exact
running mean under a still camera, the exact shift, disocclusion, the sky, the
argument errors, its quality against the fp64 oracle, the stand-alone
sanitizer program and the presence of the new entries.
"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_denoise_host import SIZES as DENOISE_SIZES, analytic_guides, bits, random_inputs

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "temporal_check"
F = np.float32
INF = F(np.inf)
SIZES = DENOISE_SIZES + ((3, 257), (257, 3))   # rows x width
TEMPORAL_FUNCS = ("rt_temporal_create", "rt_temporal_free", "rt_temporal_reset", "rt_temporal_frames",
                  "rt_temporal_step", "rt_temporal_read", "rt_temporal_host")
OPTIONS = (dict(), dict(max_history=1), dict(max_history=4), dict(sigma_z=1.0), dict(normal_min=-1.0))


# ---- rt.h's definition in NumPy: float32 element-wise operations in the stated
# order, the taps as fancy-indexed gathers with masks; float64 only for R -------
def setup_np(cam, prev_cam):
    """(R (3, 3) float32, dc (3,) float32): the host set-up of a step."""
    c = np.array(prev_cam.as_list()[:12], np.float32).astype(np.float64).reshape(4, 3)
    center, p00, du, dv = c
    q = p00 - center

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    c0, c1, c2 = cross(dv, q), cross(q, du), cross(du, dv)
    det = (du[0] * c0[0] + du[1] * c0[1]) + du[2] * c0[2]
    with np.errstate(all="ignore"):
        R = np.stack([c0 / det, c1 / det, c2 / det]).astype(np.float32)
    dc = np.array(cam.center[:], np.float32) - np.array(prev_cam.center[:], np.float32)
    return R, dc


def reproject_np(cam, prev_cam, feat, row0):
    """Steps 1-3: (hist, fx, fy, zexp) per pixel."""
    rows, width = feat.shape[:2]
    R, dc = setup_np(cam, prev_cam)
    center, p00, du, dv = np.array(cam.as_list()[:12], np.float32).reshape(4, 3)
    y, x = np.mgrid[0:rows, 0:width]
    xf, jf = x.astype(np.float32), (row0 + y).astype(np.float32)
    e = [((p00[c] + xf * du[c]) + jf * dv[c]) - center[c] for c in range(3)]
    zp = feat[..., 6]
    fin = np.isfinite(zp)
    ln = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    sc = zp / ln
    w = [np.where(fin, sc * e[c] + dc[c], e[c]) for c in range(3)]
    zexp = np.where(fin, np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), INF)
    al, be, ga = ((R[k, 0] * w[0] + R[k, 1] * w[1]) + R[k, 2] * w[2] for k in range(3))
    fx = al / ga
    fy = be / ga - F(row0)
    hist = (ga > 0) & (fx > F(-1)) & (fx < F(width)) & (fy > F(-1)) & (fy < F(rows))
    assert all(a.dtype == np.float32 for a in (fx, fy, zexp))
    return hist, fx, fy, zexp


def split_np(f, hist):
    """Step 4 for one axis: (integer corner, snapped fraction)."""
    fl = np.floor(f)
    t = f - fl
    lo = t < F(2.0 ** -6)
    hi = ~lo & (t > F(1) - F(2.0 ** -6))
    i0 = np.where(hist, fl, F(0)).astype(np.int64) + hi
    return i0, np.where(lo | hi, F(0), t)


def temporal_np(cam, prev_cam, half0, half1, feat, prev=None, row0=0, max_history=32, sigma_z=0.1, normal_min=0.9):
    rows, width = half0.shape[:2]
    if prev_cam is None:
        return half0.copy(), half1.copy(), np.ones((rows, width), np.float32)
    a0, a1, guide, length = prev
    sigma_z, normal_min, mh = F(sigma_z), F(normal_min), F(float(max_history))
    with np.errstate(all="ignore"):
        hist, fx, fy, zexp = reproject_np(cam, prev_cam, feat, row0)
        x0, tx = split_np(fx, hist)
        y0, ty = split_np(fy, hist)
        tol = sigma_z * zexp
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
                valid = inside & (lq >= 1) & ((pinf & (zq == INF)) |
                                              (pfin & np.isfinite(zq) & (np.abs(zq - zexp) <= tol) & (dot >= normal_min)))
                acc0 = np.where(valid[..., None], acc0 + b[..., None] * a0[iy, ix], acc0)
                acc1 = np.where(valid[..., None], acc1 + b[..., None] * a1[iy, ix], acc1)
                accl = np.where(valid, accl + b * lq, accl)
                bsum = np.where(valid, bsum + b, bsum)
        accept = hist & (bsum >= F(0.25))
        h0, h1, lh = acc0 / bsum[..., None], acc1 / bsum[..., None], accl / bsum
        n = np.where(lh + F(1) < mh, lh + F(1), mh)
        k = F(1) / n
        out0 = np.where(accept[..., None], h0 + k[..., None] * (half0 - h0), half0)
        out1 = np.where(accept[..., None], h1 + k[..., None] * (half1 - h1), half1)
        out_len = np.where(accept, n, F(1))
    assert out0.dtype == out1.dtype == out_len.dtype == np.float32
    return out0, out1, out_len


def host(cam, prev_cam, half0, half1, feat, prev=None, row0=0, **opts):
    from rtclj import raytracing as R
    return R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, **opts)


# ---- cameras ----------------------------------------------------------------
BASE = dict(vfov=20.0, look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), defocus_angle=0.6,
            focus_dist=10.0)


def cam_of(width, height, **change):
    from rtclj import raytracing as R
    return R.camera(width, height, **{**BASE, **change})


def camera_pairs(width, height):
    """name -> (previous, current) for a width x height frame whose surfaces
    lie 0.5 .. 30 away (random_inputs' depths)."""
    base = cam_of(width, height)
    lf, la = np.array(BASE["look_from"]), np.array(BASE["look_at"])
    fwd = (la - lf) / np.linalg.norm(la - lf)
    px = 2 * np.tan(np.radians(10.0)) * 10.0 / height     # a pixel's size on the focus plane
    side = np.cross(fwd, (0.0, 1.0, 0.0))
    side /= np.linalg.norm(side)
    return {
        "still": (base, base),
        "pan": (base, cam_of(width, height, look_at=tuple(la + 2.6 * px * side + 1.3 * px * np.array([0, 1.0, 0])))),
        "dolly": (base, cam_of(width, height, look_from=tuple(lf + 0.7 * fwd))),
        "rotation": (base, cam_of(width, height, vup=(0.05, 1.0, -0.02), look_at=tuple(la + 3.1 * px * side))),
        # the previous camera stood 12 ahead: surfaces nearer than that lie behind its image plane
        "behind": (cam_of(width, height, look_from=tuple(lf + 12.0 * fwd), look_at=tuple(la + 12.0 * fwd)), base),
    }


PAIRS = ("still", "pan", "dolly", "rotation", "behind")


def random_history(feat, seed):
    """A history for a frame whose guides are `feat`: the same surfaces, with
    some depths and normals off, some pixels sky, lengths 0, 1, fractions and
    long ones."""
    rows, width = feat.shape[:2]
    rng = np.random.default_rng(seed)
    a0 = rng.uniform(0.0, 2.0, (rows, width, 3)).astype(np.float32)
    a1 = rng.uniform(0.0, 2.0, (rows, width, 3)).astype(np.float32)
    guide = feat[..., 3:7].copy()
    off = rng.random((rows, width))
    guide[..., 3] = np.where(off < 0.15, guide[..., 3] * F(1.3), guide[..., 3] * rng.uniform(0.97, 1.03, (rows, width)).astype(np.float32))
    guide[..., 3][rng.random((rows, width)) < 0.05] = INF
    guide[..., :3][rng.random((rows, width)) < 0.1] = (0.0, -1.0, 0.0)
    length = rng.choice(np.array([0.0, 1.0, 1.0, 2.5, 7.0, 31.5, 40.0], np.float32), (rows, width))
    return a0, a1, np.ascontiguousarray(guide), np.ascontiguousarray(length)


def smooth_inputs(rows, width, seed):
    """random_inputs with most of the frame one smooth surface, so that moving
    cameras find history that passes the tests, beside the random rest."""
    half0, half1, feat = random_inputs(rows, width, seed)
    rng = np.random.default_rng(seed + 1)
    smooth = rng.random((rows, width)) < 0.7
    y, x = np.mgrid[0:rows, 0:width]
    feat[..., 3:6][smooth] = (0.0, 0.6, 0.8)
    feat[..., 6][smooth] = (F(9.0) + F(0.01) * x + F(0.02) * y).astype(np.float32)[smooth]
    feat[..., 7][smooth] = 1.0
    return half0, half1, feat


# ---- 1. bit-equality with the definition --------------------------------------
@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("row0", (0, 5))
def test_host_equals_the_definition(rows, width, pair, row0):
    half0, half1, feat = smooth_inputs(rows, width, seed=1000 * rows + width)
    prev = random_history(feat, seed=rows + 7 * width)
    prev_cam, cam = camera_pairs(width, rows + row0 + 3)[pair]
    keep = [a.copy() for a in (half0, half1, feat) + prev]
    accepted = []
    for opts in OPTIONS:
        got = host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, **opts)
        want = temporal_np(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, **opts)
        for g, w, what in zip(got, want, ("out0", "out1", "out_len")):
            assert g.shape == w.shape and np.isfinite(g).all()
            assert np.array_equal(bits(g), bits(w)), (opts, what, int((bits(g) != bits(w)).sum()), g.size)
        accepted.append(float((got[2] > 1).mean()))
    print(f"{rows} x {width} {pair} row0 {row0}: history accepted on", ["%.2f" % a for a in accepted])
    for a, k in zip((half0, half1, feat) + prev, keep):
        assert np.array_equal(bits(a), bits(k))   # the inputs are never written
    if pair == "still" and rows * width >= 200:
        assert 0.2 < accepted[0] < 1.0 and accepted[4] > accepted[0]
    if pair == "behind":   # gamma <= 0 occurs, and not everywhere
        hist = reproject_np(cam, prev_cam, feat, row0)[0]
        assert rows * width < 200 or 0 < hist.mean() < 1


def test_no_previous_camera_and_null_options():
    from rtclj._lib import fptr, lib
    half0, half1, feat = smooth_inputs(13, 17, seed=5)
    cam = cam_of(17, 13)
    out0, out1, length = host(cam, None, half0, half1, feat)
    assert np.array_equal(bits(out0), bits(half0)) and np.array_equal(bits(out1), bits(half1)) and (length == 1).all()
    # NULL options are the defaults
    prev = random_history(feat, seed=9)
    o0, o1, ol = np.empty_like(half0), np.empty_like(half0), np.empty((13, 17), np.float32)
    pan = camera_pairs(17, 13)["pan"][1]
    assert lib.rt_temporal_host(None, C.byref(pan), C.byref(cam), 17, 13, 0, fptr(half0), fptr(half1), fptr(feat),
                                *(fptr(a) for a in prev), fptr(o0), fptr(o1), fptr(ol)) == 0
    want = host(pan, cam, half0, half1, feat, prev=prev)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((o0, o1, ol), want))


# ---- 2. a still camera is an exact running mean ---------------------------------
def running_mean(frames, max_history=None):
    """The fp32 recurrence of rt.h's step 6 under a still camera: at step k the
    length is N = min(k, max_history) and m += (1 / N) * (x - m), every
    operation rounded once (1 / N is the definition's k; it is rounded before
    the product, so this is not (x - m) / N for an N that is no power of two)."""
    m = frames[0].copy()
    for k in range(2, len(frames) + 1):
        n = F(min(k, max_history) if max_history else k)
        m = m + (F(1) / n) * (frames[k - 1] - m)
    return m


@pytest.mark.parametrize("max_history", (32, 4))
def test_still_camera_is_an_exact_running_mean(max_history):
    rows, width = 13, 17
    cam = cam_of(width, rows)
    rng = np.random.default_rng(21)
    # fixed guides: a unit normal and a depth of its own per pixel, a fifth of the pixels sky
    feat = np.zeros((rows, width, 8), np.float32)
    nrm = rng.normal(size=(rows, width, 3))
    sky = rng.random((rows, width)) < 0.2
    feat[..., :3] = 0.5
    feat[..., 3:6] = np.where(sky[..., None], 0.0, nrm / np.linalg.norm(nrm, axis=-1, keepdims=True))
    feat[..., 6] = np.where(sky, np.inf, rng.uniform(0.5, 30.0, (rows, width)))
    feat[..., 7] = ~sky
    xs0 = [rng.uniform(0.0, 2.0, (rows, width, 3)).astype(np.float32) for _ in range(6)]
    xs1 = [rng.uniform(0.0, 2.0, (rows, width, 3)).astype(np.float32) for _ in range(6)]
    prev_cam, prev = None, None
    for k in range(1, 7):
        out0, out1, length = host(cam, prev_cam, xs0[k - 1], xs1[k - 1], feat, prev=prev, max_history=max_history)
        assert np.array_equal(bits(out0), bits(running_mean(xs0[:k], max_history))), k
        assert np.array_equal(bits(out1), bits(running_mean(xs1[:k], max_history))), k
        assert (length == min(k, max_history)).all(), k
        prev_cam, prev = cam, (out0, out1, np.ascontiguousarray(feat[..., 3:7]), length)
    # beside the true mean: within a few ulp of it while nothing is capped
    if max_history == 32:
        mean = np.mean(np.stack(xs0).astype(np.float64), axis=0)
        assert np.abs(out0 - mean).max() < 1e-6


def test_still_cover_camera_reprojects_onto_itself():
    """rt.h's snap makes a still camera an identity: |fx - x| stays far below
    2^-6 (160 x 90, the cover camera and the reference camera)."""
    from rtclj import raytracing as R, scenes
    w, h = 160, 90
    for cam in (scenes.cover_camera(w, h), R.camera(w, h, **R.REFERENCE_CAMERA)):
        feat = np.zeros((h, w, 8), np.float32)
        feat[..., 6] = np.random.default_rng(1).uniform(0.5, 30.0, (h, w))
        hist, fx, fy, _ = reproject_np(cam, cam, feat, 0)
        y, x = np.mgrid[0:h, 0:w]
        err = max(float(np.abs(fx - x).max()), float(np.abs(fy - y).max()))
        print("still camera: max |f - pixel| = %.3g" % err)
        assert hist.all() and err < 2.0 ** -8


# ---- 3. the exact shift, 4. disocclusion ------------------------------------------
W, H = 160, 90


def plane_cameras(shift_px):
    """Two cameras looking down -z at the plane z = 0 from 10 away (the focus
    distance: the pixel grid lies in the plane), the second moved sideways by
    exactly shift_px pixels."""
    kw = dict(vfov=20.0, vup=(0.0, 1.0, 0.0), defocus_angle=0.0, focus_dist=10.0)
    from rtclj import raytracing as R
    c0 = R.camera(W, H, look_from=(0.0, 0.0, 10.0), look_at=(0.0, 0.0, 0.0), **kw)
    dx = shift_px * float(c0.du[0])
    c1 = R.camera(W, H, look_from=(dx, 0.0, 10.0), look_at=(dx, 0.0, 0.0), **kw)
    return c0, c1


def plane_depth(cam, scale=1.0):
    """The distance from the camera's centre to the plane z = 10 (1 - scale)
    through every pixel centre, in float64 on the camera's fp32 fields,
    rounded to fp32 (scale 1: the plane z = 0)."""
    c = np.array(cam.as_list()[:12], np.float64).reshape(4, 3)
    y, x = np.mgrid[0:H, 0:W]
    e = c[1] + x[..., None] * c[2] + y[..., None] * c[3] - c[0]
    return (np.linalg.norm(e, axis=-1) * scale).astype(np.float32)


def plane_feat(depth):
    feat = np.zeros((H, W, 8), np.float32)
    feat[..., :3] = 0.5
    feat[..., 5] = 1.0
    feat[..., 6] = depth
    feat[..., 7] = 1.0
    return feat


def test_exact_shift():
    c0, c1 = plane_cameras(3)
    rng = np.random.default_rng(4)
    a0 = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    a1 = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    half0 = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    half1 = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    f0, f1 = plane_feat(plane_depth(c0)), plane_feat(plane_depth(c1))
    prev = (a0, a1, np.ascontiguousarray(f0[..., 3:7]), np.full((H, W), 5.0, np.float32))
    hist, fx, fy, _ = reproject_np(c1, c0, f1, 0)
    y, x = np.mgrid[0:H, 0:W]
    print("shift: max |fx - (x + 3)| = %.3g, max |fy - y| = %.3g" % (np.abs(fx - (x + 3)).max(), np.abs(fy - y).max()))
    assert np.abs(fx - (x + 3)).max() < 2.0 ** -8 and np.abs(fy - y).max() < 2.0 ** -8
    out0, out1, length = host(c1, c0, half0, half1, f1, prev=prev)
    k = F(1) / F(6)
    for out, a, half in ((out0, a0, half0), (out1, a1, half1)):
        h = a[:, 3:]                                     # the history, 3 columns over, unblurred
        assert np.array_equal(bits(out[:, :W - 3]), bits(h + k * (half[:, :W - 3] - h)))
        assert np.array_equal(bits(out[:, W - 3:]), bits(half[:, W - 3:]))   # the columns that entered the frame
    assert (length[:, :W - 3] == 6).all() and (length[:, W - 3:] == 1).all()
    for got, want in zip((out0, out1, length), temporal_np(c1, c0, half0, half1, f1, prev=prev)):
        assert np.array_equal(bits(got), bits(want))


def test_disocclusion():
    """A strip at half the distance (columns 60..80 of the previous frame, so
    54..74 of the current one: twice the far plane's parallax of 3 pixels) in
    front of the plane.  Columns 75..77 show the plane now and showed the strip
    before."""
    c0, c1 = plane_cameras(3)
    far0, far1 = plane_depth(c0), plane_depth(c1)
    near0, near1 = plane_depth(c0, 0.5), plane_depth(c1, 0.5)
    cols = np.arange(W)
    strip0, strip1 = (cols >= 60) & (cols <= 80), (cols >= 54) & (cols <= 74)
    uncovered = (cols >= 75) & (cols <= 77)
    f0 = plane_feat(np.where(strip0[None, :], near0, far0))
    f1 = plane_feat(np.where(strip1[None, :], near1, far1))
    a = np.zeros((H, W, 3), np.float32)
    a[:, strip0] = 100.0
    prev = (a, a.copy(), np.ascontiguousarray(f0[..., 3:7]), np.full((H, W), 8.0, np.float32))
    zero = np.zeros((H, W, 3), np.float32)
    out0, out1, length = host(c1, c0, zero, zero, f1, prev=prev)
    assert (out0[:, uncovered] == 0).all() and (out1[:, uncovered] == 0).all() and (length[:, uncovered] == 1).all()
    # the strip's own history followed it, and the plane's beside it
    k = F(1) / F(9)
    assert np.array_equal(bits(out0[:, strip1]), bits(np.broadcast_to(F(100) + k * (F(0) - F(100)), (H, 21, 3))))
    assert (length[:, strip1] == 9).all() and (out0[:, ~strip1] == 0).all()
    # the control: with the tests off, the uncovered pixels do pick the strip's colour up
    c0_, _, cl = host(c1, c0, zero, zero, f1, prev=prev, sigma_z=1e6, normal_min=-1.0)
    assert (c0_[:, uncovered] > 80).all() and (cl[:, uncovered] == 9).all()


# ---- 5. the sky -------------------------------------------------------------------
def test_sky_follows_direction():
    from rtclj import raytracing as R
    kw = dict(vfov=20.0, look_from=(0.0, 0.0, 10.0), vup=(0.0, 1.0, 0.0), defocus_angle=0.0, focus_dist=10.0)
    c0 = R.camera(W, H, look_at=(0.0, 0.0, 0.0), **kw)
    c1 = R.camera(W, H, look_at=(0.11, -0.07, 0.0), **kw)         # a pure rotation of a few pixels
    sky = np.zeros((H, W, 8), np.float32)
    sky[..., :3] = 0.7
    sky[..., 6] = INF
    rng = np.random.default_rng(8)
    a = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    half = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    prev = (a, a.copy(), np.ascontiguousarray(sky[..., 3:7]), np.full((H, W), 3.0, np.float32))
    got = host(c1, c0, half, half, sky, prev=prev)
    hist, fx, fy, _ = reproject_np(c1, c0, sky, 0)
    inner = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    assert inner.mean() > 0.9 and (got[2][inner] > 3.5).all()      # the history is kept: L = 3 + 1 up to rounding
    for g, w_ in zip(got, temporal_np(c1, c0, half, half, sky, prev=prev)):
        assert np.array_equal(bits(g), bits(w_))
    # a translation does not move the sky at all
    c2 = R.camera(W, H, **{**kw, "look_from": (0.5, 0.25, 10.0)}, look_at=(0.5, 0.25, 0.0))
    g2 = host(c2, c0, half, half, sky, prev=prev)
    k = F(1) / F(4)
    assert np.array_equal(bits(g2[0]), bits(a + k * (half - a))) and (g2[2] == 4).all()


def test_sky_and_surface_never_mix():
    from rtclj import raytracing as R
    kw = dict(vfov=20.0, vup=(0.0, 1.0, 0.0), defocus_angle=0.0, focus_dist=10.0)
    c0 = R.camera(W, H, look_from=(0.0, 0.0, 10.0), look_at=(0.0, 0.0, 0.0), **kw)
    c1 = R.camera(W, H, look_from=(0.013, 0.004, 10.0), look_at=(0.05, -0.03, 0.0), **kw)   # fractional motion
    cols = np.arange(W)
    surf = (cols >= 70)[None, :].repeat(H, 0)
    surf[:30, 60:70] = True
    feats = []
    for cam in (c0, c1):
        f = plane_feat(plane_depth(cam))
        f[~surf, 3:6] = 0.0
        f[~surf, 6] = INF
        f[~surf, 7] = 0.0
        feats.append(f)
    a = np.where(surf[..., None], F(0), F(128)) * np.ones((H, W, 3), np.float32)   # (128: b * 128 is exact)
    prev = (a, a.copy(), np.ascontiguousarray(feats[0][..., 3:7]), np.full((H, W), 6.0, np.float32))
    out0, out1, length = host(c1, c0, a, a, feats[1], prev=prev, sigma_z=1e6, normal_min=-1.0)
    # exactly one of a tap's and the pixel's depths is +inf: the tap is out,
    # whatever the options: every pixel keeps its own side's colour exactly
    assert (out0[surf] == 0).all() and (out0[~surf] == 128).all() and np.array_equal(bits(out0), bits(out1))
    assert 0.5 < (length > 1).mean() < 1.0


# ---- 6. arguments -----------------------------------------------------------------
def test_argument_errors():
    from rtclj._lib import fptr, lib, rt_camera, rt_temporal_opts
    from rtclj import raytracing as R
    rows, width = 5, 6
    half0, half1, feat = smooth_inputs(rows, width, seed=3)
    prev = random_history(feat, seed=4)
    cam = cam_of(width, rows)
    out = [np.full_like(half0, 7.0), np.full_like(half0, 7.0), np.full((rows, width), 7.0, np.float32)]
    ok = [None, C.byref(cam), C.byref(cam), width, rows, 0, fptr(half0), fptr(half1), fptr(feat)] + \
         [fptr(a) for a in prev] + [fptr(a) for a in out]
    assert lib.rt_temporal_host(*ok) == 0
    done = [a.copy() for a in out]

    def refused(args, word):
        for a in out:
            a[...] = 7.0
        assert lib.rt_temporal_host(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert all((a == 7.0).all() for a in out)            # nothing was written

    for k in (1, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        bad = list(ok)
        bad[k] = None
        refused(bad, b"NULL")
    no_prev = list(ok)
    no_prev[2] = no_prev[9] = no_prev[10] = no_prev[11] = no_prev[12] = None    # no history: none of it is needed
    assert lib.rt_temporal_host(*no_prev) == 0
    good = dict(max_history=32, sigma_z=0.1, normal_min=0.9)
    assert lib.rt_temporal_host(C.byref(rt_temporal_opts(**good)), *ok[1:]) == 0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, done))
    for field, values in (("max_history", (0, -1, 65537)),
                          ("sigma_z", (0.0, -1.0, float("nan"), float("inf"))),
                          ("normal_min", (-1.5, 1.5, float("nan"), float("inf"), float("-inf")))):
        for v in values:
            o = rt_temporal_opts(**{**good, field: v})
            refused([C.byref(o)] + ok[1:], field.encode())
    for w_, r_, r0 in ((0, rows, 0), (width, 0, 0), (-1, rows, 0), (width, -3, 0), (1 << 16, 1 << 16, 0)):
        refused(ok[:3] + [w_, r_, r0] + ok[6:], b"width/rows")
    refused(ok[:5] + [-1] + ok[6:], b"row0")
    for k in (13, 14):     # an output may not overlap an input, the history or the other output
        for alias in (half0, half1, feat, prev[0], prev[1], prev[2]):
            bad = list(ok)
            bad[k] = fptr(alias)
            keep = alias.copy()
            assert lib.rt_temporal_host(*bad) == -1 and b"overlap" in lib.rt_last_error()
            assert np.array_equal(bits(alias), bits(keep))
    bad = list(ok)
    bad[14] = bad[13]
    refused(bad, b"overlap")
    bad = list(ok)
    bad[15] = fptr(prev[3])
    assert lib.rt_temporal_host(*bad) == -1 and b"overlap" in lib.rt_last_error()
    # a degenerate previous camera: det = 0
    flat = rt_camera.from_buffer_copy(cam)
    flat.du[0] = flat.du[1] = flat.du[2] = 0.0
    refused(ok[:2] + [C.byref(flat)] + ok[3:], b"degenerate")
    nanc = rt_camera.from_buffer_copy(cam)
    nanc.p00[1] = float("nan")
    refused(ok[:2] + [C.byref(nanc)] + ok[3:], b"degenerate")
    # the device entries refuse NULL handles and bad shapes before any device call
    h = C.c_void_p()
    assert lib.rt_temporal_create(0, 8, 8, 0, None) == -1
    for w_, r_, r0 in ((0, 8, 0), (8, 0, 0), (-4, 8, 0), (1 << 16, 1 << 16, 0), (8, 8, -1)):
        assert lib.rt_temporal_create(0, w_, r_, r0, C.byref(h)) == -1 and not h.value
    assert lib.rt_temporal_create(lib.rt_device_count(), 8, 8, 0, C.byref(h)) == -5 and not h.value
    assert lib.rt_temporal_create(-1, 8, 8, 0, C.byref(h)) == -5 and not h.value
    assert lib.rt_temporal_step(None, None, None, None, None, None, None, None, None) == -1
    assert b"NULL" in lib.rt_last_error()
    assert lib.rt_temporal_reset(None, None) == -1 and lib.rt_temporal_read(None, None, None, None, None, None) == -1
    assert lib.rt_temporal_frames(None) == -1 and lib.rt_temporal_free(None) == 0
    with pytest.raises(TypeError):
        R.temporal_host(cam, None, half0, half1, feat, sigma=1.0)
    with pytest.raises(ValueError):
        R.temporal_host(cam, None, half0, half1[:-1], feat)
    with pytest.raises(ValueError):
        R.temporal_host(cam, cam, half0, half1, feat)
    with pytest.raises(R.RTError):
        R.temporal_host(cam, None, half0, half1, feat, max_history=0)
    with pytest.raises(ValueError):
        next(R.render_sequence(R.hittables, [cam], 16, 9, spp=3))


# ---- 7. quality, against the fp64 oracle ------------------------------------------
# MSE(temporal + denoiser) / MSE(denoiser alone on the last frame), seeds 1-3, as
# measured by the test below; the asserted bound is the midpoint between the
# largest of them and 1.
MEASURED_RATIOS = (0.6749, 0.7267, 0.6448)
QUALITY_BOUND = 0.5 * (max(MEASURED_RATIOS) + 1.0)    # 0.8633


def orbit(f, frames=8):
    """look-from of frame f: a slow orbit about the look-at point that ends at
    the reference camera."""
    from rtclj import raytracing as R
    lf, la = np.array(R.REFERENCE_CAMERA["look_from"]), np.array(R.REFERENCE_CAMERA["look_at"])
    ang = np.radians(0.25) * (f - (frames - 1))
    d = lf - la
    rot = np.array([d[0] * np.cos(ang) + d[2] * np.sin(ang), d[1], -d[0] * np.sin(ang) + d[2] * np.cos(ang)])
    return tuple(la + rot)


def test_quality_against_the_fp64_oracle():
    """The reference scene at 160 x 90: eight frames along a slow orbit of
    look-from (0.25 degrees a frame), 2 + 2 spp a frame (MODE_REF64D, sample
    ranges [4 f, 4 f + 2) and [4 f + 2, 4 f + 4)), analytic guides, against a
    1024-spp frame of the last camera at seed 77.
    MSE(temporal accumulation, then the denoiser) / MSE(the denoiser alone on
    the last frame), seeds 1, 2, 3 -- measured: see MEASURED_RATIOS; asserted:
    each below QUALITY_BOUND, the midpoint between the largest of them and 1
    (DESIGN.md §3.9 records them).  At most 15 % of the last frame's pixels may
    have L = 1, or the test measures disocclusion."""
    import oracle
    from rtclj import raytracing as R
    from test_denoise_host import host as denoise
    w, h, frames = 160, 90, 8
    sph64, kind, mat64 = R.flatten64(R.hittables)
    cams = [R.camera(w, h, **{**R.REFERENCE_CAMERA, "look_from": orbit(f, frames)}) for f in range(frames)]
    feats = [analytic_guides(sph64, kind, mat64, cam, w, h) for cam in cams]
    last = cams[-1]
    ref = oracle.render(oracle.MODE_REF64D, sph64, kind, mat64, last.as_list(), last.defocus, w, h, 1024, 50,
                        seed=77)[0].astype(np.float64)
    ratios, fresh = [], []
    for seed in (1, 2, 3):
        prev_cam, prev = None, None
        for f, (cam, feat) in enumerate(zip(cams, feats)):
            args = (sph64, kind, mat64, cam.as_list(), cam.defocus, w, h)
            h0 = oracle.render(oracle.MODE_REF64D, *args, 2, 50, seed=seed, sample_begin=4 * f)[0]
            h1 = oracle.render(oracle.MODE_REF64D, *args, 2, 50, seed=seed, sample_begin=4 * f + 2)[0]
            out0, out1, length = host(cam, prev_cam, h0, h1, feat, prev=prev)
            prev_cam, prev = cam, (out0, out1, np.ascontiguousarray(feat[..., 3:7]), length)
        with_history = denoise(out0, out1, feats[-1])
        alone = denoise(h0, h1, feats[-1])
        ratios.append(float(((with_history - ref) ** 2).mean() / ((alone - ref) ** 2).mean()))
        fresh.append(float((length == 1).mean()))
    print("MSE(temporal + denoiser) / MSE(denoiser alone), seeds 1-3:", ["%.4f" % r for r in ratios],
          "; pixels with L = 1 at the last frame:", ["%.4f" % v for v in fresh])
    assert max(fresh) <= 0.15, fresh
    assert QUALITY_BOUND is not None and all(r < QUALITY_BOUND for r in ratios), (ratios, QUALITY_BOUND)


# ---- 8. the sanitizers, stand-alone ------------------------------------------------
def test_sanitizer_program_exits_clean():
    """lib/temporal_check: csrc/temporal.h (rt_temporal_host's body, the text
    the kernel runs) under -fsanitize=address,undefined with hostile inputs, a
    program of its own."""
    assert TOOL.exists(), "lib/temporal_check is not built (make -C raytracing-clj_amd)"
    r = subprocess.run([str(TOOL)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["bad_status"] == 0 and rep["bad_len"] == 0
    assert rep["calls"] > 1000 and rep["degenerate"] > 0 and rep["accepted"] > 1000 and rep["pixels"] > 100_000
    mk = (ROOT / "raytracing-clj_amd" / "Makefile").read_text()
    rule = mk[mk.index("$(OUT)/temporal_check:"):]
    assert "-fsanitize=address,undefined" in rule[:600] and "-fno-sanitize-recover" in rule[:600]


# ---- presence ---------------------------------------------------------------------
@pytest.mark.parametrize("which", ["product", "diag"])
def test_symbols_and_signatures(which):
    import rtclj
    from rtclj import _lib
    dll = C.CDLL(str(rtclj.library_path if which == "product" else _lib.diag_library_path))
    hdr = (ROOT / "include" / "rt.h").read_text()
    for name in TEMPORAL_FUNCS:
        assert hasattr(dll, name), name
        assert name in _lib.SIGNATURES and name in _lib.ADDITIVE
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    assert re.search(r"typedef struct rt_temporal_opts", hdr)
    assert C.sizeof(_lib.rt_temporal_opts) == 12
    assert len(_lib.SIGNATURES["rt_temporal_step"][1]) == 9 and len(_lib.SIGNATURES["rt_temporal_host"][1]) == 16
    assert len(_lib.SIGNATURES["rt_temporal_create"][1]) == 5 and len(_lib.SIGNATURES["rt_temporal_read"][1]) == 6


def test_python_host_exposes_temporal_accumulation():
    from rtclj import raytracing as R
    for name in ("temporal_host", "Temporal", "render_sequence"):
        assert name in R.__all__ and hasattr(R, name), name
    for name in ("step", "read", "reset", "close", "frames", "__enter__", "__exit__"):
        assert hasattr(R.Temporal, name), name
