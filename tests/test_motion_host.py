"""Moving bodies on the host (include/rt.h: rt_ids_host, rt_body_motion,
rt_temporal_host_motion; no GPU needed): the ids against a float64 nearest-body
search, the motion-aware step bit for bit against a NumPy restatement of rt.h,
zero motion as the existing step, the exact shift of a displaced body (with the
motion-blind step as the control), a NaN displacement, the displacement table,
the quality against the fp64 oracle under a rising sphere, the argument errors,
the stand-alone sanitizer program and the presence of the new entries.
"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_temporal_host as T
from test_denoise_host import analytic_guides, bits

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "motion_check"
F = np.float32
INF = F(np.inf)
W, H = T.W, T.H
MOTION_FUNCS = ("rt_launch_ids", "rt_ids_host", "rt_ids_occupancy", "rt_body_motion", "rt_temporal_step_motion",
                "rt_temporal_host_motion")


# ---- 1. ids_host against a float64 nearest-body search ----------------------------
def ids_np(sphere, cam, width, rows, row0=0):
    """analytic_guides' loop in float64 on the fp32 inputs, returning the index
    and which pixels are undecided: some body's |disc| < 2^-18 |oc|^2 (a
    silhouette), or the runner-up root within 2^-18 relative of the best."""
    sphere = np.asarray(sphere, np.float64)
    c = np.array(cam.as_list(), np.float64).reshape(6, 3)
    o, p00, du, dv = c[0], c[1], c[2], c[3]
    j, i = np.mgrid[row0:row0 + rows, 0:width]
    d = p00 + i[..., None] * du + j[..., None] * dv - o
    dl = np.linalg.norm(d, axis=-1)
    u = d / dl[..., None]
    tmin = 1e-3 * dl
    best = np.full((rows, width), np.inf)
    second = np.full((rows, width), np.inf)
    idx = np.full((rows, width), -1)
    edge = np.zeros((rows, width), bool)
    for b in range(len(sphere)):
        oc = sphere[b, :3] - o
        h = (u * oc).sum(-1)
        disc = h * h - ((oc * oc).sum() - sphere[b, 3] ** 2)
        edge |= np.abs(disc) < 2.0 ** -18 * (oc * oc).sum()
        sq = np.sqrt(np.maximum(disc, 0.0))
        t = np.where(h - sq > tmin, h - sq, np.where(h + sq > tmin, h + sq, np.inf))
        t = np.where(disc >= 0, t, np.inf)
        second = np.where(t < best, best, np.minimum(second, t))
        idx = np.where(t < best, b, idx)
        best = np.minimum(best, t)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(second) & (second - best <= 2.0 ** -18 * best)
    return idx, edge | close


def id_cases():
    from rtclj import raytracing as R, scenes
    ref = R.Scene.from_bodies(R.hittables)
    cov = scenes.cover(11)
    out = []
    for w, h in ((160, 90), (65, 37), (33, 17)):
        out.append(("reference", ref, R.camera(w, h, **R.REFERENCE_CAMERA), w, h, 0))
        out.append(("cover", cov, scenes.cover_camera(w, h), w, h, 0))
    out.append(("reference band", ref, R.camera(160, 90, **R.REFERENCE_CAMERA), 160, 24, 40))
    out.append(("cover band", cov, scenes.cover_camera(160, 90), 160, 24, 40))
    return out


def test_ids_host_equals_the_float64_search():
    from rtclj import raytracing as R
    for name, sc, cam, w, rows, row0 in id_cases():
        got = R.ids_host(sc, cam, w, rows, row0)
        want, undecided = ids_np(sc.sphere, cam, w, rows, row0)
        assert got.dtype == np.int32 and got.shape == (rows, w)
        assert got.min() >= -1 and got.max() < len(sc)
        wrong = (got != want) & ~undecided
        print(f"{name} {w} x {rows} row0 {row0}: undecided {100 * undecided.mean():.3f} %, sky "
              f"{100 * (want < 0).mean():.1f} %, bodies seen {len(np.unique(got[got >= 0]))}, wrong {int(wrong.sum())}")
        assert not wrong.any(), (name, np.argwhere(wrong)[:5])
        assert undecided.mean() <= 0.03, (name, float(undecided.mean()))
        if name == "cover":
            assert 0.05 < (got < 0).mean() < 0.4 and len(np.unique(got)) > 20
    # a band is the frame's rows
    sc, cam = id_cases()[0][1:3]
    assert np.array_equal(R.ids_host(sc, cam, 160, 24, 40), R.ids_host(sc, cam, 160, 90)[40:64])


def test_ids_follow_the_array_order():
    """Negative control: the centre sphere and the metal one swapped in the
    array swap their ids and nothing else."""
    from rtclj import raytracing as R
    cam = R.camera(160, 90, **R.REFERENCE_CAMERA)
    a = R.ids_host(R.hittables, cam, 160, 90)
    swapped = list(R.hittables)
    swapped[1], swapped[4] = swapped[4], swapped[1]
    b = R.ids_host(swapped, cam, 160, 90)
    assert (a == 1).sum() > 100 and (a == 4).sum() > 100
    assert not np.array_equal(a, b)
    relabel = np.array([0, 4, 2, 3, 1, -1])
    assert np.array_equal(b, relabel[a])
    # the bubble inside the glass sphere is never the first hit from outside (this camera sees no sky)
    assert set(np.unique(a).tolist()) == {0, 1, 2, 4}


# ---- 2. the motion-aware step against rt.h in NumPy ---------------------------------
def motion_of(ids, motion, finite):
    """rt.h's step 2': per pixel (m_x, m_y, m_z) -- the table's row for an id
    inside it, else 0; a sky pixel ignores its id."""
    n = len(motion)
    inside = finite & (ids >= 0) & (ids < n)
    row = np.where(inside, ids, 0)
    tab = np.asarray(motion, np.float32).reshape(-1, 4) if n else np.zeros((1, 4), np.float32)
    return [np.where(inside, tab[row, c], F(0)) for c in range(3)]


def reproject_motion_np(cam, prev_cam, feat, row0, ids, motion):
    """Steps 1-3 with the displacement: (hist, fx, fy, zexp) per pixel."""
    rows, width = feat.shape[:2]
    R, dc = T.setup_np(cam, prev_cam)
    center, p00, du, dv = np.array(cam.as_list()[:12], np.float32).reshape(4, 3)
    y, x = np.mgrid[0:rows, 0:width]
    xf, jf = x.astype(np.float32), (row0 + y).astype(np.float32)
    e = [((p00[c] + xf * du[c]) + jf * dv[c]) - center[c] for c in range(3)]
    zp = feat[..., 6]
    fin = np.isfinite(zp)
    m = motion_of(ids, motion, fin)
    ln = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    sc = zp / ln
    w = [np.where(fin, (sc * e[c] + dc[c]) - m[c], e[c]) for c in range(3)]
    zexp = np.where(fin, np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), INF)
    al, be, ga = ((R[k, 0] * w[0] + R[k, 1] * w[1]) + R[k, 2] * w[2] for k in range(3))
    fx = al / ga
    fy = be / ga - F(row0)
    hist = (ga > 0) & (fx > F(-1)) & (fx < F(width)) & (fy > F(-1)) & (fy < F(rows))
    assert all(a.dtype == np.float32 for a in (fx, fy, zexp))
    return hist, fx, fy, zexp


def temporal_motion_np(cam, prev_cam, half0, half1, feat, ids, motion, prev=None, row0=0, max_history=32, sigma_z=0.1,
                       normal_min=0.9):
    """rt.h's step with 2' in NumPy: float32 element-wise operations in the
    stated order (steps 4-6 as test_temporal_host.temporal_np states them)."""
    rows, width = half0.shape[:2]
    if prev_cam is None:
        return half0.copy(), half1.copy(), np.ones((rows, width), np.float32)
    a0, a1, guide, length = prev
    sigma_z, normal_min, mh = F(sigma_z), F(normal_min), F(float(max_history))
    with np.errstate(all="ignore"):
        hist, fx, fy, zexp = reproject_motion_np(cam, prev_cam, feat, row0, ids, motion)
        x0, tx = T.split_np(fx, hist)
        y0, ty = T.split_np(fy, hist)
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


def host(cam, prev_cam, half0, half1, feat, ids, motion, prev=None, row0=0, **opts):
    from rtclj import raytracing as R
    return R.temporal_host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0, ids=ids, motion=motion, **opts)


N_BODIES = 7


def random_motion(rows, width, seed, n=N_BODIES):
    """ids in [-3, n + 3) and a table of displacements of up to a few pixels at
    the frame's depths, two rows NaN."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-3, n + 3, (rows, width)).astype(np.int32)
    motion = np.zeros((n, 4), np.float32)
    motion[:, :3] = rng.uniform(-0.08, 0.08, (n, 3))
    motion[0, :3] = 0.0
    motion[2, :3] = np.nan
    motion[5, 1] = np.nan
    return ids, motion


@pytest.mark.parametrize("rows,width", T.SIZES)
@pytest.mark.parametrize("pair", T.PAIRS)
@pytest.mark.parametrize("row0", (0, 5))
def test_host_equals_the_definition(rows, width, pair, row0):
    half0, half1, feat = T.smooth_inputs(rows, width, seed=1000 * rows + width)
    prev = T.random_history(feat, seed=rows + 7 * width)
    ids, motion = random_motion(rows, width, seed=3 * rows + width)
    prev_cam, cam = T.camera_pairs(width, rows + row0 + 3)[pair]
    keep = [a.copy() for a in (half0, half1, feat, ids, motion) + prev]
    accepted = []
    for opts in T.OPTIONS:
        got = host(cam, prev_cam, half0, half1, feat, ids, motion, prev=prev, row0=row0, **opts)
        want = temporal_motion_np(cam, prev_cam, half0, half1, feat, ids, motion, prev=prev, row0=row0, **opts)
        for g, w, what in zip(got, want, ("out0", "out1", "out_len")):
            assert g.shape == w.shape and np.isfinite(g).all()
            assert np.array_equal(bits(g), bits(w)), (opts, what, int((bits(g) != bits(w)).sum()), g.size)
        accepted.append(float((got[2] > 1).mean()))
    blind = T.host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0)
    print(f"{rows} x {width} {pair} row0 {row0}: history accepted on", ["%.2f" % a for a in accepted],
          "; pixels that differ from the motion-blind step: %.2f" % float((bits(got[2]) != bits(blind[2])).mean()))
    for a, k in zip((half0, half1, feat, ids, motion) + prev, keep):
        assert np.array_equal(a.view(np.uint32), k.view(np.uint32))   # the inputs are never written
    if pair == "still" and rows * width >= 200:
        assert 0.1 < accepted[0] < 1.0
        # the NaN rows' finite-depth pixels have no history, whatever the options
        fin = np.isfinite(feat[..., 6])
        for opts in T.OPTIONS:
            ln = host(cam, prev_cam, half0, half1, feat, ids, motion, prev=prev, row0=row0, **opts)[2]
            assert (ln[fin & ((ids == 2) | (ids == 5))] == 1).all()


# ---- 3. zero motion is the existing step -----------------------------------------------
@pytest.mark.parametrize("pair", ("still", "pan", "rotation"))
def test_zero_motion_is_the_existing_step(pair):
    rows, width, row0 = 40, 33, 5
    half0, half1, feat = T.smooth_inputs(rows, width, seed=77)
    prev = T.random_history(feat, seed=78)
    ids, motion = random_motion(rows, width, seed=79)
    prev_cam, cam = T.camera_pairs(width, rows + row0 + 3)[pair]
    want = T.host(cam, prev_cam, half0, half1, feat, prev=prev, row0=row0)
    zero = np.zeros_like(motion)
    minus = np.full_like(ids, -1)
    for what, i_, m_ in (("zero table", ids, zero), ("ids -1", minus, motion), ("n_bodies 0", ids, None),
                         ("ids past the table", ids + N_BODIES + 3, motion)):
        got = host(cam, prev_cam, half0, half1, feat, i_, m_, prev=prev, row0=row0)
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w)), what
    # ... and a table that is not zero does change the step (the inputs above are not blind to it)
    got = host(cam, prev_cam, half0, half1, feat, ids, motion, prev=prev, row0=row0)
    assert not np.array_equal(bits(got[2]), bits(want[2]))


# ---- 4. the exact shift of a displaced body, 5. a NaN displacement ---------------------
R0, R1, C0, C1 = 30, 60, 50, 90          # the rectangle's rows and columns in the previous frame


def shift_setup(k):
    """A still camera 10 from the plane z = 0 (body 1, the background) with a
    rectangle of body 0 in the plane z = 5 before it, displaced by exactly k
    pixels to the right between the frames: there a pixel is du / 2 wide.
    Returns (cam, feat, ids, motion, prev, half0, half1, was, now): the masks
    of the rectangle's pixels before and now."""
    cam = T.plane_cameras(0)[0]
    far, near = T.plane_depth(cam), T.plane_depth(cam, 0.5)
    y, x = np.mgrid[0:H, 0:W]
    was = (y >= R0) & (y < R1) & (x >= C0) & (x < C1)
    now = (y >= R0) & (y < R1) & (x >= C0 + k) & (x < C1 + k)
    f_prev, feat = T.plane_feat(np.where(was, near, far)), T.plane_feat(np.where(now, near, far))
    ids = np.where(now, 0, 1).astype(np.int32)
    motion = np.zeros((2, 4), np.float32)
    motion[0, 0] = F(k) * (F(cam.du[0]) * F(0.5))
    rng = np.random.default_rng(40 + k)
    a0, a1, half0, half1 = (rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32) for _ in range(4))
    prev = (a0, a1, np.ascontiguousarray(f_prev[..., 3:7]), np.full((H, W), 5.0, np.float32))
    return cam, feat, ids, motion, prev, half0, half1, was, now


@pytest.mark.parametrize("k", (1, 3))
def test_exact_body_shift(k):
    cam, feat, ids, motion, prev, half0, half1, was, now = shift_setup(k)
    a0, a1 = prev[0], prev[1]
    hist, fx, fy, _ = reproject_motion_np(cam, cam, feat, 0, ids, motion)
    y, x = np.mgrid[0:H, 0:W]
    err = np.abs(fx - np.where(now, x - k, x)).max(), np.abs(fy - y).max()
    print("body shift %d: max |fx - expected| = %.3g, max |fy - y| = %.3g" % ((k,) + err))
    assert max(err) < 2.0 ** -8 and hist.all()
    out0, out1, length = host(cam, cam, half0, half1, feat, ids, motion, prev=prev)
    kk = F(1) / F(6)
    back = ~now & ~was                      # the background that was and is visible
    uncovered = was & ~now                  # the background the body just left
    assert now.sum() == (R1 - R0) * (C1 - C0) and uncovered.sum() == (R1 - R0) * k and back.sum() > 5000
    for out, a, half in ((out0, a0, half0), (out1, a1, half1)):
        moved = np.roll(a, k, axis=1)       # the history, k columns over, unblurred
        assert np.array_equal(bits(out[now]), bits((moved + kk * (half - moved))[now]))
        assert np.array_equal(bits(out[back]), bits((a + kk * (half - a))[back]))
        assert np.array_equal(bits(out[uncovered]), bits(half[uncovered]))
    assert (length[now] == 6).all() and (length[back] == 6).all() and (length[uncovered] == 1).all()
    for got, want in zip((out0, out1, length), temporal_motion_np(cam, cam, half0, half1, feat, ids, motion, prev=prev)):
        assert np.array_equal(bits(got), bits(want))
    # The control: the motion-blind step on the same inputs.  Where the body was
    # and is, it takes the history of the pixel itself -- another surface
    # point's -- with full length: silent ghosting; the k columns the body
    # entered are refused on depth.
    b0, _, bl = T.host(cam, cam, half0, half1, feat, prev=prev)
    moved = np.roll(a0, k, axis=1)
    shifted = (moved + kk * (half0 - moved))
    both, entered = now & was, now & ~was
    assert not np.array_equal(bits(b0[now]), bits(shifted[now]))
    assert (bits(b0[both]) != bits(shifted[both])).any(axis=-1).all()          # wrong on every such pixel
    assert np.array_equal(bits(b0[both]), bits((a0 + kk * (half0 - a0))[both])) and (bl[both] == 6).all()
    assert (bl[entered] == 1).all() and entered.sum() == (R1 - R0) * k


def test_nan_displacement_restarts_exactly_that_body():
    cam, feat, ids, motion, prev, half0, half1, was, now = shift_setup(0)
    assert np.array_equal(was, now)
    # a third body, still, and a strip of sky that carries body 0's id
    ids = ids.copy()
    ids[:, 120:] = 2
    motion = np.zeros((3, 4), np.float32)
    sky = np.zeros((H, W), bool)
    sky[70:80, 20:100] = True
    feat = feat.copy()
    feat[sky, 3:6] = 0.0
    feat[sky, 6] = INF
    feat[sky, 7] = 0.0
    ids[sky] = 0
    prev = (prev[0], prev[1], np.ascontiguousarray(feat[..., 3:7]), prev[3])
    length = host(cam, cam, half0, half1, feat, ids, motion, prev=prev)[2]
    assert (length == 6).all()
    for lanes in ((0,), (1,), (2,), (0, 1, 2)):
        m = motion.copy()
        m[0, list(lanes)] = np.nan
        length = host(cam, cam, half0, half1, feat, ids, m, prev=prev)[2]
        body = (ids == 0) & ~sky
        assert body.sum() == (R1 - R0) * (C1 - C0)
        assert (length[body] == 1).all() and (length[~body] == 6).all(), lanes
    m = motion.copy()
    m[0, 3] = np.nan                                                      # lane 3 is not read
    assert (host(cam, cam, half0, half1, feat, ids, m, prev=prev)[2] == 6).all()
    for v in (np.inf, -np.inf, 2.0 ** 40):                                # nowhere near: no history either
        m = motion.copy()
        m[0, 0] = v
        length = host(cam, cam, half0, half1, feat, ids, m, prev=prev)[2]
        assert (length[body] == 1).all() and (length[~body] == 6).all(), v


# ---- 6. rt_body_motion -----------------------------------------------------------------
def test_body_motion():
    from rtclj import raytracing as R
    from rtclj._lib import fptr, lib, rt_scene
    prev = R.Scene.from_bodies(R.hittables)
    moved = [dict(b) for b in R.hittables]
    moved[1]["hittable/center"] = (0.1, 0.08, -1.2)
    moved[4]["hittable/center"] = (1.0, 0.0, -1.25)
    cur = R.Scene.from_bodies(moved)
    m = R.body_motion(cur, prev)
    assert m.dtype == np.float32 and m.shape == (5, 4)
    want = np.zeros((5, 4), np.float32)
    want[:, :3] = cur.sphere[:, :3] - prev.sphere[:, :3]                  # one fp32 subtraction per component
    assert np.array_equal(bits(m), bits(want))
    assert m[1, 0] == F(0.1) and m[1, 1] == F(0.08) and m[4, 2] == F(-1.25) - F(-1.0) and not m[[0, 2, 3]].any()
    assert np.array_equal(bits(R.body_motion(prev, cur)[:, :3]), bits(prev.sphere[:, :3] - cur.sphere[:, :3]))
    assert np.array_equal(R.body_motion(R.hittables, R.hittables), np.zeros((5, 4), np.float32))

    def changed(**kw):
        s = R.Scene(kw.get("sphere", cur.sphere.copy()), kw.get("kind", cur.kind.copy()), kw.get("mat", cur.mat.copy()))
        return R.body_motion(s, prev)

    sph = cur.sphere.copy()
    sph[2, 3] = np.nextafter(sph[2, 3], F(1))                              # a radius one ulp off
    kind = cur.kind.copy()
    kind[4] = 0                                                            # metal -> lambertian
    for lane in range(4):
        mat = cur.mat.copy()
        mat[0, lane] = -0.0 if mat[0, lane] == 0 else np.nextafter(mat[0, lane], F(0))   # (-0 differs from +0 by bits)
        got = changed(mat=mat)
        assert np.isnan(got[0, :3]).all() and got[0, 3] == 0 and np.array_equal(bits(got[1:]), bits(want[1:])), lane
    got = changed(sphere=sph)
    assert np.isnan(got[2, :3]).all() and got[2, 3] == 0 and np.array_equal(bits(got[[0, 1, 3, 4]]), bits(want[[0, 1, 3, 4]]))
    got = changed(kind=kind)
    assert np.isnan(got[4, :3]).all() and np.array_equal(bits(got[:4]), bits(want[:4]))
    # the same NaN radius on both sides is the same body
    sn = cur.sphere.copy()
    sn[3, 3] = np.nan
    same = R.body_motion(R.Scene(sn, cur.kind, cur.mat), R.Scene(sn, cur.kind, cur.mat))
    assert not np.isnan(same).any()
    # errors
    out = np.full((5, 4), 7.0, np.float32)
    four = R.Scene(cur.sphere[:4], cur.kind[:4], cur.mat[:4])
    for args, word in (((None, C.byref(prev.c), fptr(out)), b"NULL"), ((C.byref(cur.c), None, fptr(out)), b"NULL"),
                       ((C.byref(cur.c), C.byref(prev.c), None), b"NULL"),
                       ((C.byref(cur.c), C.byref(four.c), fptr(out)), b"counts differ"),
                       ((C.byref(rt_scene(5, None, None, None)), C.byref(prev.c), fptr(out)), b"scene arrays")):
        assert lib.rt_body_motion(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert (out == 7.0).all()
    empty = R.Scene(np.zeros((0, 4)), np.zeros(0), np.zeros((0, 4)))
    assert R.body_motion(empty, empty).shape == (0, 4)
    with pytest.raises(R.RTError):
        R.body_motion(cur, four)


# ---- 7. quality, against the fp64 oracle ---------------------------------------------------
# MSE(motion step + denoiser) / MSE(rt_temporal_host + denoiser) over the centre
# sphere's pixels of the last frame, seeds 1-3, as measured by the test below;
# the asserted bound is the midpoint between the largest of them and 1.
MEASURED_RATIOS = (0.1539, 0.1605, 0.1541)
QUALITY_BOUND = 0.5 * (max(MEASURED_RATIOS) + 1.0)    # 0.5803


def rising(f, frames=8):
    """The reference bodies at frame f: the centre sphere rises 0.08 a frame and
    ends at its reference position."""
    from rtclj import raytracing as R
    bodies = [dict(b) for b in R.hittables]
    bodies[1]["hittable/center"] = (0.0, -0.08 * (frames - 1 - f), -1.2)
    return bodies


def test_quality_against_the_fp64_oracle():
    """The reference scene at 160 x 90 under the still reference camera, eight
    frames, the centre sphere rising 0.08 a frame (about 6 pixels); 2 + 2 spp a
    frame (MODE_REF64D, sample ranges [4 f, 4 f + 2) and [4 f + 2, 4 f + 4)),
    analytic guides, ids from ids_host, displacements from body_motion; against
    a 1024-spp frame of the last scene at seed 77, over the last frame's pixels
    with id 1.  MSE(rt_temporal_host_motion, then the denoiser) /
    MSE(rt_temporal_host on the same inputs, then the denoiser), seeds 1, 2, 3
    -- measured: see MEASURED_RATIOS; asserted: each below QUALITY_BOUND, the
    midpoint between the largest of them and 1 (DESIGN.md §3.10 records them).
    At least 80 % of those pixels must have L >= 4 under the motion step, or
    the test measures restarts and not accumulation."""
    import oracle
    from rtclj import raytracing as R
    from test_denoise_host import host as denoise
    w, h, frames = 160, 90, 8
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    bodies = [rising(f, frames) for f in range(frames)]
    scenes = [R.Scene.from_bodies(b) for b in bodies]
    flat = [R.flatten64(b) for b in bodies]
    feats = [analytic_guides(*fl, cam, w, h) for fl in flat]
    ids = [R.ids_host(sc, cam, w, h) for sc in scenes]
    motions = [None] + [R.body_motion(scenes[f], scenes[f - 1]) for f in range(1, frames)]
    assert np.array_equal(motions[3][1], np.array([0, scenes[3].sphere[1, 1] - scenes[2].sphere[1, 1], 0, 0], np.float32))
    ref = oracle.render(oracle.MODE_REF64D, *flat[-1], cam.as_list(), cam.defocus, w, h, 1024, 50,
                        seed=77)[0].astype(np.float64)
    body = ids[-1] == 1
    assert body.sum() > 400
    ratios, long_motion, long_blind = [], [], []
    for seed in (1, 2, 3):
        prev_cam, prev_m, prev_b = None, None, None
        for f in range(frames):
            args = (*flat[f], cam.as_list(), cam.defocus, w, h)
            h0 = oracle.render(oracle.MODE_REF64D, *args, 2, 50, seed=seed, sample_begin=4 * f)[0]
            h1 = oracle.render(oracle.MODE_REF64D, *args, 2, 50, seed=seed, sample_begin=4 * f + 2)[0]
            m0, m1, ml = host(cam, prev_cam, h0, h1, feats[f], ids[f], motions[f], prev=prev_m)
            b0, b1, bl = T.host(cam, prev_cam, h0, h1, feats[f], prev=prev_b)
            guide = np.ascontiguousarray(feats[f][..., 3:7])
            prev_cam, prev_m, prev_b = cam, (m0, m1, guide, ml), (b0, b1, guide, bl)
        with_motion, blind = denoise(m0, m1, feats[-1]), denoise(b0, b1, feats[-1])
        ratios.append(float(((with_motion - ref)[body] ** 2).mean() / ((blind - ref)[body] ** 2).mean()))
        long_motion.append(float((ml[body] >= 4).mean()))
        long_blind.append(float((bl[body] >= 4).mean()))
    print("MSE(motion step + denoiser) / MSE(motion-blind step + denoiser) on the sphere, seeds 1-3:",
          ["%.4f" % r for r in ratios], "; its pixels with L >= 4: motion", ["%.4f" % v for v in long_motion],
          "blind", ["%.4f" % v for v in long_blind])
    assert min(long_motion) >= 0.8, long_motion
    assert QUALITY_BOUND is not None and all(r < QUALITY_BOUND for r in ratios), (ratios, QUALITY_BOUND)


# ---- 8. presence and errors ---------------------------------------------------------------
def test_argument_errors():
    from rtclj._lib import fptr, i32ptr, lib, rt_scene
    from rtclj import raytracing as R
    rows, width = 5, 6
    half0, half1, feat = T.smooth_inputs(rows, width, seed=3)
    prev = T.random_history(feat, seed=4)
    ids, motion = random_motion(rows, width, seed=5)
    cam = T.cam_of(width, rows)
    out = [np.full_like(half0, 7.0), np.full_like(half0, 7.0), np.full((rows, width), 7.0, np.float32)]
    ok = [None, C.byref(cam), C.byref(cam), width, rows, 0, fptr(half0), fptr(half1), fptr(feat)] + \
         [fptr(a) for a in prev] + [i32ptr(ids), fptr(motion), N_BODIES] + [fptr(a) for a in out]
    assert lib.rt_temporal_host_motion(*ok) == 0

    def refused(args, word):
        for a in out:
            a[...] = 7.0
        assert lib.rt_temporal_host_motion(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert all((a == 7.0).all() for a in out)            # nothing was written

    for k in (1, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 18):
        bad = list(ok)
        bad[k] = None
        refused(bad, b"NULL")
    refused(ok[:15] + [-1] + ok[16:], b"n_bodies")
    none = list(ok)
    none[14], none[15] = None, 0                              # no table: none is needed
    assert lib.rt_temporal_host_motion(*none) == 0
    for w_, r_ in ((0, rows), (width, 0), (1 << 16, 1 << 16)):
        refused(ok[:3] + [w_, r_, 0] + ok[6:], b"width/rows")
    refused(ok[:5] + [-1] + ok[6:], b"row0")
    for k in (16, 17):     # an output may not overlap the ids or the table either
        for alias in (ids, motion, half0, prev[2]):
            bad = list(ok)
            bad[k] = C.cast(alias.ctypes.data, C.POINTER(C.c_float))
            keep = alias.copy()
            assert lib.rt_temporal_host_motion(*bad) == -1 and b"overlap" in lib.rt_last_error()
            assert np.array_equal(alias.view(np.uint32), keep.view(np.uint32))
    # rt_ids_host
    sc = R.Scene.from_bodies(R.hittables)
    o = np.full((rows, width), 0x7fffffff, np.int32)
    assert lib.rt_ids_host(C.byref(sc.c), C.byref(cam), width, rows, 0, i32ptr(o)) == 0 and (o < 5).all()
    o[...] = 0x7fffffff
    for args, word in (((None, C.byref(cam), width, rows, 0, i32ptr(o)), b"NULL"),
                       ((C.byref(sc.c), None, width, rows, 0, i32ptr(o)), b"NULL"),
                       ((C.byref(sc.c), C.byref(cam), width, rows, 0, None), b"NULL"),
                       ((C.byref(sc.c), C.byref(cam), 0, rows, 0, i32ptr(o)), b"width/rows"),
                       ((C.byref(sc.c), C.byref(cam), width, -2, 0, i32ptr(o)), b"width/rows"),
                       ((C.byref(sc.c), C.byref(cam), 1 << 16, 1 << 16, 0, i32ptr(o)), b"width/rows"),
                       ((C.byref(sc.c), C.byref(cam), width, rows, -1, i32ptr(o)), b"row0"),
                       ((C.byref(rt_scene(-1, None, None, None)), C.byref(cam), width, rows, 0, i32ptr(o)), b"scene")):
        assert lib.rt_ids_host(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert (o == 0x7fffffff).all()
    empty = rt_scene(0, None, None, None)
    assert lib.rt_ids_host(C.byref(empty), C.byref(cam), width, rows, 0, i32ptr(o)) == 0 and (o == -1).all()
    # the device entries refuse NULL handles and bad shapes before any device call
    assert lib.rt_launch_ids(None, C.byref(cam), 8, 8, 0, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_ids_occupancy(None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_temporal_step_motion(None, None, None, None, None, None, None, None, 0, None, None, None) == -1
    assert b"NULL" in lib.rt_last_error()
    # the Python layer
    with pytest.raises(ValueError):
        R.temporal_host(cam, None, half0, half1, feat, motion=motion)          # motion without ids
    with pytest.raises(ValueError):
        R.temporal_host(cam, None, half0, half1, feat, ids=ids[:-1])
    with pytest.raises(ValueError):
        R.temporal_host(cam, None, half0, half1, feat, ids=ids, motion=motion[:, :3])
    with pytest.raises(R.RTError):
        R.ids_host(sc, cam, 0, 4)
    with pytest.raises(ValueError):
        next(R.render_animation([R.hittables], [cam], 16, 9, spp=3))


def test_sanitizer_program_exits_clean():
    """lib/motion_check: csrc/body_ids.h and csrc/temporal.h (the bodies of
    rt_ids_host, rt_body_motion and rt_temporal_host_motion, the texts the
    kernels run) under -fsanitize=address,undefined with hostile inputs, a
    program of its own."""
    assert TOOL.exists(), "lib/motion_check is not built (make -C raytracing-clj_amd)"
    r = subprocess.run([str(TOOL)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["bad_status"] == 0 and rep["bad_id"] == 0 and rep["bad_len"] == 0
    assert rep["id_calls"] > 1000 and rep["id_hits"] > 1000 and rep["id_pixels"] > 100_000
    assert rep["step_calls"] > 1000 and rep["degenerate"] > 0 and rep["accepted"] > 1000 and rep["step_pixels"] > 100_000
    assert rep["motion_calls"] > 10 and rep["motion_nan"] > 0
    mk = (ROOT / "raytracing-clj_amd" / "Makefile").read_text()
    rule = mk[mk.index("$(OUT)/motion_check:"):]
    assert "-fsanitize=address,undefined,float-cast-overflow" in rule[:700] and "-fno-sanitize-recover=all" in rule[:700]
    assert "-static-libasan" in rule[:700] and "motion_check" in mk[mk.index("all:"):mk.index("all:") + 400]


@pytest.mark.parametrize("which", ["product", "diag"])
def test_symbols_and_signatures(which):
    import rtclj
    from rtclj import _lib
    dll = C.CDLL(str(rtclj.library_path if which == "product" else _lib.diag_library_path))
    hdr = (ROOT / "include" / "rt.h").read_text()
    for name in MOTION_FUNCS:
        assert hasattr(dll, name), name
        assert name in _lib.SIGNATURES and name in _lib.ADDITIVE
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    n = {name: len(_lib.SIGNATURES[name][1]) for name in MOTION_FUNCS}
    assert n == {"rt_launch_ids": 7, "rt_ids_host": 6, "rt_ids_occupancy": 2, "rt_body_motion": 3,
                 "rt_temporal_step_motion": 12, "rt_temporal_host_motion": 19}
    # the existing entries keep their argument lists
    assert len(_lib.SIGNATURES["rt_temporal_step"][1]) == 9 and len(_lib.SIGNATURES["rt_temporal_host"][1]) == 16


def test_python_host_exposes_moving_bodies():
    import inspect
    from rtclj import raytracing as R
    for name in ("ids_host", "body_ids_into", "body_motion", "render_animation"):
        assert name in R.__all__ and hasattr(R, name), name
    step = inspect.signature(R.Temporal.step).parameters
    assert all(k in step for k in ("d_ids", "d_motion", "n_bodies")) and step["d_ids"].default is None
    th = inspect.signature(R.temporal_host).parameters
    assert th["ids"].default is None and th["motion"].default is None
    assert "stages" in inspect.signature(R.render_animation).parameters
