"""The sample budget on the host (include/rt.h: rt_temporal_host_probe,
rt_budget_plan_host, rt_temporal_host_budget; no GPU needed): bit-equality of
the probe and the weighted step with NumPy restatements of rt.h's definitions
over chained steps, the probe as the prediction of the step's stored length,
the plan against an integer restatement and its constructed cases, multipliers
of one as the clamped step, the clamp of the multipliers, the constructed
weights (L = 8, then k = 1 / 9), the argument errors, the stand-alone
sanitizer program and the presence of the new entries.
"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_motion_host as M
import test_temporal_clamp_host as K
import test_temporal_host as T
from test_denoise_host import bits

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "budget_check"
F = np.float32
INF = F(np.inf)
SIZES = ((1, 1), (1, 9), (9, 1), (5, 7), (17, 33))            # rows x width
PLAN_SIZES = ((1, 1), (9, 12), (17, 33), (40, 33))            # with partial tiles
NEW_FUNCS = ("rt_temporal_probe", "rt_temporal_host_probe", "rt_budget_plan_host", "rt_budget_create", "rt_budget_free",
             "rt_budget_plan", "rt_budget_plan_mult", "rt_budget_trace", "rt_budget_resolve", "rt_budget_resolve_half",
             "rt_budget_read", "rt_budget_mult_read", "rt_budget_device_mult", "rt_budget_samples",
             "rt_temporal_step_budget", "rt_temporal_host_budget")


def tiles(rows, width):
    return (rows + 7) // 8, (width + 7) // 8


# ---- rt.h's definitions in NumPy -------------------------------------------------------
def gather_np(cam, prev_cam, feat, prev, row0=0, ids=None, motion=None, sigma_z=0.1, normal_min=0.9):
    """Steps 1-5 (2' with ids): (accept, acc0, acc1, accL, bsum), float32
    element-wise operations in the stated order, as
    test_temporal_clamp_host.step_np states them."""
    rows, width = feat.shape[:2]
    a0, a1, guide, length = prev
    with np.errstate(all="ignore"):
        if ids is None:
            hist, fx, fy, zexp = T.reproject_np(cam, prev_cam, feat, row0)
        else:
            hist, fx, fy, zexp = M.reproject_motion_np(cam, prev_cam, feat, row0, ids, motion)
        x0, tx = T.split_np(fx, hist)
        y0, ty = T.split_np(fy, hist)
        tol = F(sigma_z) * zexp
        pinf, pfin = zexp == INF, np.isfinite(zexp)
        acc0 = np.zeros((rows, width, 3), np.float32) if a0 is not None else None
        acc1 = np.zeros((rows, width, 3), np.float32) if a1 is not None else None
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
                if acc0 is not None:
                    acc0 = np.where(valid[..., None], acc0 + b[..., None] * a0[iy, ix], acc0)
                    acc1 = np.where(valid[..., None], acc1 + b[..., None] * a1[iy, ix], acc1)
                accl = np.where(valid, accl + b * lq, accl)
                bsum = np.where(valid, bsum + b, bsum)
        accept = hist & (bsum >= F(0.25))
    return accept, acc0, acc1, accl, bsum


def probe_np(cam, prev_cam, feat, prev=None, row0=0, ids=None, motion=None, sigma_z=0.1, normal_min=0.9):
    rows, width = feat.shape[:2]
    if prev_cam is None:
        return np.zeros((rows, width), np.float32)
    accept, _, _, accl, bsum = gather_np(cam, prev_cam, feat, (None, None, prev[2], prev[3]), row0, ids, motion, sigma_z,
                                         normal_min)
    with np.errstate(all="ignore"):
        out = np.where(accept, accl / bsum, F(0))
    assert out.dtype == np.float32
    return out


def weight_np(mult, rows, width):
    """wt per pixel: float(min(max(mult[y / 8, x / 8], 1), 16))."""
    m = np.clip(np.asarray(mult, np.uint32).astype(np.int64), 1, 16)
    y, x = np.mgrid[0:rows, 0:width]
    return m[y // 8, x // 8].astype(np.float32)


def step_np(cam, prev_cam, half0, half1, feat, mult, prev=None, row0=0, ids=None, motion=None, clamp=None, max_history=32,
            sigma_z=0.1, normal_min=0.9):
    """rt.h's weighted step (clamp None: the clamp's defaults)."""
    rows, width = half0.shape[:2]
    wt, mh = weight_np(mult, rows, width), F(float(max_history))
    if prev_cam is None:
        return half0.copy(), half1.copy(), np.where(wt < mh, wt, mh)
    clamp = {} if clamp is None else clamp
    accept, acc0, acc1, accl, bsum = gather_np(cam, prev_cam, feat, prev, row0, ids, motion, sigma_z, normal_min)
    with np.errstate(all="ignore"):
        h0, h1, lh = acc0 / bsum[..., None], acc1 / bsum[..., None], accl / bsum
        lo, hi = K.box_np(half0, half1, feat, clamp.get("radius", K.DEFAULT_RADIUS), clamp.get("gamma", K.DEFAULT_GAMMA),
                          sigma_z, normal_min)
        h0 = np.where(h0 < lo, lo, np.where(h0 > hi, hi, h0))
        h1 = np.where(h1 < lo, lo, np.where(h1 > hi, hi, h1))
        n = np.where(lh + wt < mh, lh + wt, mh)
        k = wt / n
        out0 = np.where(accept[..., None], h0 + k[..., None] * (half0 - h0), half0)
        out1 = np.where(accept[..., None], h1 + k[..., None] * (half1 - h1), half1)
        out_len = np.where(accept, n, np.where(wt < mh, wt, mh))
    assert out0.dtype == out1.dtype == out_len.dtype == np.float32
    return out0, out1, out_len


def plan_np(length, half_spp=1, target=8, max_mult=8, quantile_64=16):
    """rt.h's rule, in integers."""
    rows, width = length.shape
    gy, gx = tiles(rows, width)
    mult = np.ones((gy, gx), np.uint32)
    with np.errstate(invalid="ignore"):
        for ty in range(gy):
            for tx in range(gx):
                t = length[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
                npx = int(t.size)
                for j in range(1, target + 1):
                    c = int((~(t >= F(j))).sum())
                    if c * 64 >= quantile_64 * npx:
                        mult[ty, tx] = min(max(target - (j - 1), 1), max_mult)
                        break
    return mult


def random_mult(rows, width, seed, wild=False):
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, 3, 8, 16, 17, 1 << 31, (1 << 32) - 1] if wild else [1, 2, 3, 5, 8, 16], np.uint32)
    return pool[rng.integers(0, len(pool), tiles(rows, width))]


def host(cam, prev_cam, half0, half1, feat, mult, **kw):
    from rtclj import raytracing as R
    return R.temporal_host(cam, prev_cam, half0, half1, feat, mult=mult, **kw)


def probe(cam, prev_cam, feat, **kw):
    from rtclj import raytracing as R
    return R.temporal_probe_host(cam, prev_cam, feat, **kw)


# ---- 1. the probe ------------------------------------------------------------------------
@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("row0", (0, 3))
@pytest.mark.parametrize("with_ids", (False, True))
def test_probe_equals_the_definition_and_predicts_the_step(rows, width, row0, with_ids):
    """Over K.chain_inputs' chain (a still, two panned and a rotated camera: a
    moving camera), with and without ids and motion."""
    base, first, frames = K.chain_inputs(rows, width, row0)
    ones = np.ones(tiles(rows, width), np.uint32)
    prev_cam, prev, found = base, first, 0
    for s, (cam, half0, half1, feat, ids, motion) in enumerate(frames):
        kw = dict(prev=prev, row0=row0, ids=ids if with_ids else None, motion=motion if with_ids else None)
        keep = [a.copy() for a in (feat, ids, motion) + tuple(prev)]
        got = probe(cam, prev_cam, feat, **kw)
        want = probe_np(cam, prev_cam, feat, **kw)
        assert got.shape == (rows, width) and np.array_equal(bits(got), bits(want)), (s, int((bits(got) != bits(want)).sum()))
        for a, k in zip((feat, ids, motion) + tuple(prev), keep):
            assert np.array_equal(a.view(np.uint32), k.view(np.uint32))     # nothing is modified
        found += int((got > 0).sum())
        # the colours are not read: a history without them gives the same lengths
        again = probe(cam, prev_cam, feat, **{**kw, "prev": (None, None, prev[2], prev[3])})
        assert np.array_equal(bits(again), bits(got))
        # followed by the step at mult = 1: out_len == min(len + 1, max_history), bit for bit
        for mh in (32, 3):
            out = host(cam, prev_cam, half0, half1, feat, ones, max_history=mh, **kw)
            with np.errstate(all="ignore"):
                pred = np.where(got + F(1) < F(mh), got + F(1), F(mh))
            assert np.array_equal(bits(out[2]), bits(pred)), (s, mh)
        out = host(cam, prev_cam, half0, half1, feat, ones, **kw)
        prev_cam, prev = cam, (out[0], out[1], np.ascontiguousarray(feat[..., 3:7]), out[2])
    if rows * width >= 35:
        assert found > 0          # the chain is not blind to the history


def test_probe_without_a_previous_camera_is_zero():
    _, _, feat = T.smooth_inputs(13, 17, seed=5)
    ids, motion = M.random_motion(13, 17, seed=6)
    cam = T.cam_of(17, 13)
    for kw in ({}, dict(ids=ids, motion=motion)):
        got = probe(cam, None, feat, **kw)
        assert got.shape == (13, 17) and got.dtype == np.float32 and (bits(got) == 0).all()


# ---- 2. the plan -------------------------------------------------------------------------
def random_lengths(rows, width, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2.0, 40.0, (rows, width)).astype(np.float32)
    pick = rng.integers(0, 10, (rows, width))
    a[pick == 0] = np.nan
    a[pick == 1] = 0.0
    a[pick == 2] = np.floor(a[pick == 2])          # exactly on a threshold
    a[pick == 3] = 64.0                            # >= any target
    a[pick == 4] = -np.inf
    # the first tile short of 3 frames throughout (quantile_64 = 64 asks for every pixel)
    a[:8, :8] = rng.uniform(0.0, 2.9, a[:8, :8].shape).astype(np.float32)
    return a


@pytest.mark.parametrize("rows,width", PLAN_SIZES)
@pytest.mark.parametrize("quantile_64", (1, 16, 64))
@pytest.mark.parametrize("target", (1, 8, 32))
def test_plan_equals_the_integer_rule(rows, width, quantile_64, target):
    from rtclj import raytracing as R
    seen = set()
    for max_mult in (1, 4, 16):
        for seed in (1, 2):
            length = random_lengths(rows, width, 100 * rows + width + seed)
            keep = length.copy()
            o = dict(half_spp=2, target=target, max_mult=max_mult, quantile_64=quantile_64)
            got = R.budget_plan_host(length, **o)
            want = plan_np(length, **o)
            assert got.dtype == np.uint32 and got.shape == tiles(rows, width) and np.array_equal(got, want)
            assert got.min() >= 1 and got.max() <= max_mult
            assert np.array_equal(bits(length), bits(keep))
            seen |= set(got.ravel().tolist())
    if target > 1 and rows * width > 64:
        assert len(seen) > 1


def test_plan_constructed_tiles():
    from rtclj import raytracing as R
    o = dict(half_spp=1, target=8, max_mult=8, quantile_64=16)
    tile = np.full((8, 8), 32.0, np.float32)
    assert R.budget_plan_host(tile, **o).tolist() == [[1]]                     # all long
    assert R.budget_plan_host(np.zeros((8, 8), np.float32), **o).tolist() == [[8]]
    assert R.budget_plan_host(np.zeros((8, 8), np.float32), **{**o, "max_mult": 3}).tolist() == [[3]]
    assert R.budget_plan_host(np.zeros((8, 8), np.float32), **{**o, "target": 5}).tolist() == [[5]]   # min(target, max_mult)
    short = tile.copy()
    short.ravel()[:16] = 0.0                                                   # exactly the quantile's count: 16 of 64
    assert R.budget_plan_host(short, **o).tolist() == [[8]]
    short.ravel()[15] = 32.0                                                   # one fewer
    assert R.budget_plan_host(short, **o).tolist() == [[1]]
    short.ravel()[:16] = 5.0                                                   # the shortest quarter holds 5 frames
    assert R.budget_plan_host(short, **o).tolist() == [[3]]
    short.ravel()[:16] = 7.5                                                   # short of 8 only
    assert R.budget_plan_host(short, **o).tolist() == [[1]]
    # a partial tile: 3 x 5 = 15 pixels, the quantile is ceil(15 * 16 / 64) = 4 of them
    part = np.full((3, 5), 32.0, np.float32)
    part.ravel()[:4] = np.nan
    assert R.budget_plan_host(part, **o).tolist() == [[8]]
    part.ravel()[3] = 32.0
    assert R.budget_plan_host(part, **o).tolist() == [[1]]
    # four tiles, each of its own kind
    four = np.full((16, 16), 32.0, np.float32)
    four[:8, 8:] = 0.0
    four[8:, :8] = 6.0
    assert R.budget_plan_host(four, **o).tolist() == [[1, 8], [2, 1]]


# ---- 3. the weighted step ----------------------------------------------------------------
@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("row0", (0, 3))
@pytest.mark.parametrize("with_ids", (False, True))
def test_weighted_step_equals_the_definition(rows, width, row0, with_ids):
    base, first, frames = K.chain_inputs(rows, width, row0)
    for clamp in (None, dict(radius=1, gamma=0.25), dict(radius=2, gamma=float("inf"))):
        prev_cam, prev, weighted = base, first, 0
        for s, (cam, half0, half1, feat, ids, motion) in enumerate(frames):
            mult = random_mult(rows, width, seed=rows + width + s, wild=(s % 2 == 1))
            kw = dict(prev=prev, row0=row0, ids=ids if with_ids else None, motion=motion if with_ids else None,
                      clamp=clamp)
            keep = [a.copy() for a in (half0, half1, feat, ids, motion, mult) + tuple(prev)]
            got = host(cam, prev_cam, half0, half1, feat, mult, **kw)
            want = step_np(cam, prev_cam, half0, half1, feat, mult, **kw)
            for g, w, what in zip(got, want, ("out0", "out1", "out_len")):
                assert g.shape == w.shape and np.isfinite(g).all()
                assert np.array_equal(bits(g), bits(w)), (clamp, s, what, int((bits(g) != bits(w)).sum()), g.size)
            for a, k in zip((half0, half1, feat, ids, motion, mult) + tuple(prev), keep):
                assert np.array_equal(a.view(np.uint32), k.view(np.uint32))   # the inputs are never written
            # multipliers outside 1..16 are clamped
            clamped = host(cam, prev_cam, half0, half1, feat, np.clip(mult.astype(np.int64), 1, 16).astype(np.uint32), **kw)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, clamped))
            plain = K.host(cam, prev_cam, half0, half1, feat, **{**kw, "clamp": clamp or {}})
            weighted += int((bits(got[2]) != bits(plain[2])).sum())
            prev_cam, prev = cam, (got[0], got[1], np.ascontiguousarray(feat[..., 3:7]), got[2])
        assert weighted > 0       # the weights are not all one


@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("with_ids", (False, True))
@pytest.mark.parametrize("gamma", (1.0, float("inf")))
def test_multipliers_of_one_are_the_clamped_step(rows, width, with_ids, gamma):
    base, first, frames = K.chain_inputs(rows, width, 3)
    ones = np.ones(tiles(rows, width), np.uint32)
    clamp = dict(radius=2, gamma=gamma)
    prev_cam, prev = base, first
    for cam, half0, half1, feat, ids, motion in frames:
        kw = dict(prev=prev, row0=3, ids=ids if with_ids else None, motion=motion if with_ids else None, clamp=clamp)
        got = host(cam, prev_cam, half0, half1, feat, ones, **kw)
        want = K.host(cam, prev_cam, half0, half1, feat, **kw)
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w))
        # ... and zeros are clamped to ones
        zeros = host(cam, prev_cam, half0, half1, feat, np.zeros_like(ones), **kw)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(zeros, want))
        prev_cam, prev = cam, (got[0], got[1], np.ascontiguousarray(feat[..., 3:7]), got[2])
    # NULL clamp options are the clamp's defaults
    cam, half0, half1, feat, ids, motion = frames[1]
    a = host(cam, base, half0, half1, feat, ones, prev=first, row0=3)
    b = K.host(cam, base, half0, half1, feat, prev=first, row0=3, clamp={})
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_eight_frames_worth_then_one_ninth():
    """A still camera over one plane.  Frame 1 finds no history and is traced
    at mult = 8: it stores L = 8.  Frame 2 at mult = 1 blends with k = 1 / 9."""
    H, W = T.H, T.W
    cam = T.plane_cameras(0)[0]
    feat = T.plane_feat(T.plane_depth(cam))
    rng = np.random.default_rng(3)
    a0, a1, b0, b1 = (rng.uniform(0.1, 1.0, (H, W, 3)).astype(np.float32) for _ in range(4))
    empty = (np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.float32),
             np.zeros((H, W), np.float32))
    inf = dict(gamma=float("inf"))
    eight, ones = np.full(tiles(H, W), 8, np.uint32), np.ones(tiles(H, W), np.uint32)
    assert (probe(cam, cam, feat, prev=empty) == 0).all()
    o0, o1, l1 = host(cam, cam, a0, a1, feat, eight, prev=empty, clamp=inf)
    assert np.array_equal(bits(o0), bits(a0)) and np.array_equal(bits(o1), bits(a1)) and (l1 == 8).all()
    prev = (o0, o1, np.ascontiguousarray(feat[..., 3:7]), l1)
    assert (probe(cam, cam, feat, prev=prev) == 8).all()
    p0, p1, l2 = host(cam, cam, b0, b1, feat, ones, prev=prev, clamp=inf)
    k = F(1) / F(9)
    assert (l2 == 9).all()
    assert np.array_equal(bits(p0), bits(a0 + k * (b0 - a0))) and np.array_equal(bits(p1), bits(a1 + k * (b1 - a1)))
    # the unweighted step would have stored L = 1 and blended 1 : 1
    _, _, u1 = K.host(cam, cam, a0, a1, feat, prev=empty, clamp=inf)
    assert (u1 == 1).all()
    # max_history caps a weight as it caps a length
    assert (host(cam, cam, a0, a1, feat, eight, prev=empty, clamp=inf, max_history=5)[2] == 5).all()
    # and a weighted frame on top of a history: N = L + 8, k = 8 / N
    q0, _, l3 = host(cam, cam, b0, b1, feat, eight, prev=(p0, p1, prev[2], l2), clamp=inf)
    assert (l3 == 17).all() and np.array_equal(bits(q0), bits(p0 + (F(8) / F(17)) * (b0 - p0)))


# ---- 4. arguments ------------------------------------------------------------------------
def test_argument_errors():
    from rtclj._lib import fptr, i32ptr, lib, rt_budget_opts, rt_temporal_clamp_opts, rt_temporal_opts, u32ptr
    from rtclj import raytracing as R
    rows, width = 5, 6
    half0, half1, feat = T.smooth_inputs(rows, width, seed=3)
    prev = T.random_history(feat, seed=4)
    ids, motion = M.random_motion(rows, width, seed=5)
    mult = np.full(tiles(rows, width), 3, np.uint32)
    cam = T.cam_of(width, rows)

    def refused(fn, args, word, outs):
        for a in outs:
            a[...] = 7
        assert fn(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert all((a == 7).all() for a in outs)             # nothing was written

    # rt_temporal_host_budget
    out = [np.full_like(half0, 7.0), np.full_like(half0, 7.0), np.full((rows, width), 7.0, np.float32)]
    ok = [None, None, C.byref(cam), C.byref(cam), width, rows, 0, fptr(half0), fptr(half1), fptr(feat)] + \
         [fptr(a) for a in prev] + [i32ptr(ids), fptr(motion), M.N_BODIES, u32ptr(mult)] + [fptr(a) for a in out]
    fn = lib.rt_temporal_host_budget
    assert len(ok) == 21 and fn(*ok) == 0
    for k in (2, 7, 8, 9, 10, 11, 12, 13, 15, 17, 18, 19, 20):
        bad = list(ok)
        bad[k] = None
        refused(fn, bad, b"NULL", out)
    refused(fn, ok[:16] + [-1] + ok[17:], b"n_bodies", out)
    no_ids = list(ok)
    no_ids[14], no_ids[15], no_ids[16] = None, None, -5      # without ids the table and its length are not read
    assert fn(*no_ids) == 0
    for radius in (0, 4):
        refused(fn, [None, C.byref(rt_temporal_clamp_opts(radius=radius, gamma=1.0))] + ok[2:], b"radius", out)
    for gamma in (0.0, -1.0, float("nan")):
        refused(fn, [None, C.byref(rt_temporal_clamp_opts(radius=2, gamma=gamma))] + ok[2:], b"gamma", out)
    refused(fn, [C.byref(rt_temporal_opts(max_history=0, sigma_z=0.1, normal_min=0.9))] + ok[1:], b"max_history", out)
    refused(fn, ok[:4] + [0, rows, 0] + ok[7:], b"width/rows", out)
    refused(fn, ok[:6] + [-1] + ok[7:], b"row0", out)
    for k in (18, 19):         # an output may not overlap an input: the multipliers among them
        for alias in (half0, feat, prev[2], ids, motion, mult):
            bad = list(ok)
            bad[k] = C.cast(alias.ctypes.data, C.POINTER(C.c_float))
            keep = alias.copy()
            assert fn(*bad) == -1 and b"overlap" in lib.rt_last_error()
            assert np.array_equal(alias.view(np.uint32), keep.view(np.uint32))
    # rt_temporal_host_probe
    length = np.full((rows, width), 7.0, np.float32)
    okp = [None, C.byref(cam), C.byref(cam), width, rows, 0, fptr(feat), fptr(prev[2]), fptr(prev[3]), i32ptr(ids),
           fptr(motion), M.N_BODIES, fptr(length)]
    fn = lib.rt_temporal_host_probe
    assert fn(*okp) == 0
    for k in (1, 6, 7, 8, 10, 12):
        bad = list(okp)
        bad[k] = None
        refused(fn, bad, b"NULL", [length])
    refused(fn, okp[:11] + [-1] + okp[12:], b"n_bodies", [length])
    refused(fn, [C.byref(rt_temporal_opts(max_history=32, sigma_z=0.0, normal_min=0.9))] + okp[1:], b"sigma_z", [length])
    refused(fn, okp[:3] + [width, 0, 0] + okp[6:], b"width/rows", [length])
    refused(fn, okp[:5] + [-1] + okp[6:], b"row0", [length])
    for alias in (feat, prev[2], prev[3], ids):
        bad = list(okp)
        bad[12] = C.cast(alias.ctypes.data, C.POINTER(C.c_float))
        keep = alias.copy()
        assert fn(*bad) == -1 and b"overlap" in lib.rt_last_error()
        assert np.array_equal(alias.view(np.uint32), keep.view(np.uint32))
    degenerate = type(cam).from_buffer_copy(cam)
    degenerate.du[0] = degenerate.du[1] = degenerate.du[2] = 0.0
    refused(fn, okp[:2] + [C.byref(degenerate)] + okp[3:], b"degenerate", [length])
    no_prev = list(okp)
    no_prev[2] = no_prev[7] = no_prev[8] = None
    assert fn(*no_prev) == 0 and (length == 0).all()
    # rt_budget_plan_host
    lens = np.zeros((rows, width), np.float32)
    m = np.full(tiles(rows, width), 7, np.uint32)
    good = rt_budget_opts(half_spp=1, target=8, max_mult=8, quantile_64=16)
    fn = lib.rt_budget_plan_host
    assert fn(C.byref(good), fptr(lens), width, rows, u32ptr(m)) == 0 and (m == 8).all()
    for bad, word in ((dict(half_spp=0), b"half_spp"), (dict(target=0), b"target"), (dict(target=33), b"target"),
                      (dict(max_mult=0), b"max_mult"), (dict(max_mult=17), b"max_mult"),
                      (dict(quantile_64=0), b"quantile_64"), (dict(quantile_64=65), b"quantile_64"),
                      (dict(half_spp=(1 << 24) // 16 + 1), b"RT_MAX_SPP")):
        o = rt_budget_opts(**{**dict(half_spp=1, target=8, max_mult=8, quantile_64=16), **bad})
        refused(fn, [C.byref(o), fptr(lens), width, rows, u32ptr(m)], word, [m])
    refused(fn, [None, fptr(lens), width, rows, u32ptr(m)], b"NULL", [m])
    refused(fn, [C.byref(good), None, width, rows, u32ptr(m)], b"NULL", [m])
    assert fn(C.byref(good), fptr(lens), width, rows, None) == -1 and b"NULL" in lib.rt_last_error()
    refused(fn, [C.byref(good), fptr(lens), 0, rows, u32ptr(m)], b"width/rows", [m])
    # the device entries refuse NULL handles before any device call
    assert lib.rt_temporal_probe(None, None, None, None, None, None, 0, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_temporal_step_budget(*([None] * 9), 0, *([None] * 4)) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_budget_create(None, None, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_budget_plan(None, None, None) == -1 and lib.rt_budget_plan_mult(None, None, None) == -1
    assert lib.rt_budget_trace(None, None, None, None, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_budget_resolve(None, 0, None, None) == -1 and lib.rt_budget_resolve_half(None, 0, 0, None, None) == -1
    assert lib.rt_budget_read(None, None, None, None) == -1 and lib.rt_budget_mult_read(None, None, None) == -1
    assert lib.rt_budget_device_mult(None, None) == -1
    assert lib.rt_budget_samples(None) == 0 and lib.rt_budget_free(None) == 0
    # the Python layer
    with pytest.raises(TypeError):
        R.budget_plan_host(lens, target=8)                   # half_spp is required
    with pytest.raises(TypeError):
        R.budget_plan_host(lens, half_spp=1, quantile=3)
    with pytest.raises(R.RTError):
        R.budget_plan_host(lens, half_spp=1, max_mult=17)
    with pytest.raises(ValueError):
        R.temporal_host(cam, None, half0, half1, feat, mult=np.ones((2, 2), np.uint32))
    with pytest.raises(TypeError):
        next(R.render_animation([R.hittables], [cam], 16, 9, budget=dict(target=8)))
    with pytest.raises(TypeError):
        next(R.render_animation([R.hittables], [cam], 16, 9, budget=dict(half_spp=1, tiles=3)))


# ---- 5. the stand-alone program and the interface ----------------------------------------------
def test_budget_check_runs_clean():
    """tools/budget_check.cpp: the host probe, plan and weighted step under
    AddressSanitizer and UndefinedBehaviorSanitizer, over constructed and
    hostile inputs."""
    assert TOOL.exists(), f"{TOOL} is missing (make -C raytracing-clj_amd)"
    out = subprocess.run([str(TOOL)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["bad_len"] == 0 and rep["with_history"] > 1000 and rep["calls"] > 1000


def test_new_entries_are_declared_bound_and_cited():
    from rtclj._lib import ADDITIVE, SIGNATURES, lib
    from rtclj import raytracing as R
    header = (ROOT / "include" / "rt.h").read_text()
    for name in NEW_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in SIGNATURES and name in ADDITIVE and hasattr(lib, name), name
    # every new entry's comment cites the reference lines it stands for
    section = header[header.index("the sample budget: samples where"):header.index("an uploaded scene updated in place")]
    for name in NEW_FUNCS:
        assert name in section
    assert section.count("raytracing.clj:") >= 10
    for name in ("temporal_probe_host", "budget_plan_host", "Budget"):
        assert name in R.__all__ and hasattr(R, name)
    assert hasattr(R.Temporal, "probe")
