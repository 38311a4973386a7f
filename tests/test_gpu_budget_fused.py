"""The fused budget trace on the device (include/rt.h: rt_budget_trace_fused,
rt_budget_units_read): on one plan it leaves in H0 and in H1, integer for
integer, what rt_budget_trace's passes leave, with the same counters, from two
launches; its device-built unit tables equal rt_budget_units_host on the
device's own list and multipliers; the packed fields at their full width
(max_mult = 16: k up to 31, s = 32); the compact sums' wrap-counting branch
(total spp > 255); max_mult = 1; flags, variants and the camera prelude; a band
on a stream of its own; the refusals; and render_animation(budget=dict(...,
fused=True)) against fused=False, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from test_budget_host import tiles
from test_denoise_host import bits
from test_gpu_budget import BEGIN, PATTERN, accum_sums, blocks, env, pattern_for, per_pixel  # noqa: F401  (fixtures)
from test_gpu_motion import Uploaded, dev
from test_motion_host import rising

pytestmark = pytest.mark.gpu


def both_ways(env, ds, cam, w, h, raw, begin=BEGIN, flags=0, rows=None, stream=None, variant=None, **opts):
    """One plan of `raw` multipliers on two Budgets, traced by the passes and
    fused: H0, H1 and the counters agree; -> (h0, h1, clamped multipliers)."""
    R, lib, torch = env.R, env.lib, env.torch
    d_raw = dev(env, raw, np.uint32)
    sp = stream.cuda_stream if stream is not None else None
    got = []
    for fused in (False, True):
        with R.Budget(ds, w, h, seed=9, flags=flags, rows=rows, **opts) as bd:
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            bd.plan_mult(d_raw.data_ptr(), stream=sp)
            old = lib.rt_set_variant(variant) if variant is not None else None
            try:
                n = bd.trace(ds, cam, sample_begin=begin, stream=sp, d_counters=cnt.data_ptr(), fused=fused)
                torch.cuda.synchronize()
                h0, h1 = bd.halves()
            finally:
                if old is not None:
                    lib.rt_set_variant(old)
            mult = bd.mult()
            assert n == (2 if fused else 2 * int(mult.max()))
            got.append((h0, h1, cnt.cpu().numpy().copy(), mult))
    (p0, p1, pc, pm), (f0, f1, fc, fm) = got
    assert p0.any() and p1.any()
    assert np.array_equal(f0, p0), int((f0 != p0).sum())         # integer for integer, per half
    assert np.array_equal(f1, p1), int((f1 != p1).sum())
    assert np.array_equal(fc, pc) and pc[1] > 0, (fc, pc)        # {segments, samples}
    assert np.array_equal(fm, pm)
    return f0, f1, fm


# ---- 1. fused equals the passes -------------------------------------------------------------
@pytest.mark.parametrize("w,h", ((64, 40), (33, 17)))
def test_fused_equals_passes_and_launch_accum(env, blocks, w, h):
    b = blocks[(w, h)]
    with Uploaded(env, env.ref) as ds:
        h0, h1, mult = both_ways(env, ds, b["cam"], w, h, pattern_for(w, h), half_spp=1, max_mult=4)
    assert set(mult.ravel().tolist()) == {1, 2, 3, 4}
    m_px = per_pixel(mult, h, w)
    for m in (1, 2, 3, 4):
        sel = m_px == m
        assert sel.any() and np.array_equal((h0 + h1)[sel], b["whole"][m][sel]), m
    zero = np.zeros_like(h0)
    want = [zero.copy(), zero.copy()]
    for j in range(4):
        for half in (0, 1):
            want[half] += np.where((m_px > j)[..., None], b["one"][2 * j + half], zero)
    assert np.array_equal(h0, want[0]) and np.array_equal(h1, want[1])


@pytest.mark.parametrize("w,h", ((9, 12), (33, 17)))
def test_device_table_equals_host(env, w, h):
    R = env.R
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    raw = pattern_for(w, h)
    d_raw = dev(env, raw, np.uint32)
    n_tiles = raw.size
    with Uploaded(env, env.ref) as ds, R.Budget(ds, w, h, seed=9, half_spp=1, max_mult=4) as bd:
        with pytest.raises(R.RTError, match="rt_budget_trace_fused"):
            bd.units(0)                                          # nothing has built a table yet
        bd.plan_mult(d_raw.data_ptr())
        assert bd.trace(ds, cam, sample_begin=BEGIN, fused=True) == 2
        mult, order = bd.mult(), bd.tile_list()
        assert sorted(order.tolist()) == list(range(n_tiles))
        assert (np.diff(mult.ravel()[order].astype(np.int64)) <= 0).all()
        for half in (0, 1):
            got = bd.units(half)
            want = R.budget_units_host(order, mult, half, 4)
            assert got.dtype == np.int32 and got.shape == (int(mult.sum()), 2) and np.array_equal(got, want), half
        with pytest.raises(R.RTError, match="half"):
            bd.units(2)
        # the passes build none: after the next plan the old tables are not this plan's
        bd.plan_mult(d_raw.data_ptr())
        assert bd.trace(ds, cam, sample_begin=BEGIN) == 8
        with pytest.raises(R.RTError, match="rt_budget_trace_fused"):
            bd.units(0)


def test_full_width_of_the_packed_fields(env):
    """max_mult = 16, half_spp = 3: k up to 31, s = 32, spp = 96."""
    R = env.R
    w, h = 33, 17
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    gy, gx = tiles(h, w)
    raw = (1 + np.arange(gy * gx) % 3).astype(np.uint32).reshape(gy, gx)
    raw[1, 2] = 16
    with Uploaded(env, env.ref) as ds:
        h0, h1, mult = both_ways(env, ds, cam, w, h, raw, half_spp=3, max_mult=16)
        assert np.array_equal(mult, raw)
        whole = accum_sums(env, ds, cam, w, h, 96, BEGIN)
    sel = per_pixel(mult, h, w) == 16
    assert sel.sum() == 64 and np.array_equal((h0 + h1)[sel], whole[sel])


def test_total_spp_above_255(env):
    """half_spp = 40, max_mult = 4: the frame's spp is 320, so the compact
    variant's u32 sums count their wraps while a unit adds only 40 samples."""
    R = env.R
    w, h = 17, 9
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    with Uploaded(env, env.ref) as ds:
        _, _, mult = both_ways(env, ds, cam, w, h, pattern_for(w, h), half_spp=40, max_mult=4)
    assert mult.max() == 4 and mult.min() == 1


def test_max_mult_one_is_two_uniform_accumulators(env):
    R = env.R
    w, h = 33, 17
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    with Uploaded(env, env.ref) as ds, R.Budget(ds, w, h, seed=9, half_spp=2, max_mult=1) as bd:
        d_len = dev(env, np.zeros((h, w), np.float32))
        bd.plan(d_len.data_ptr())
        assert (bd.mult() == 1).all() and bd.trace(ds, cam, sample_begin=BEGIN, fused=True) == 2
        h0, h1 = bd.halves()
        assert np.array_equal(h0, accum_sums(env, ds, cam, w, h, 2, BEGIN))
        assert np.array_equal(h1, accum_sums(env, ds, cam, w, h, 2, BEGIN + 2))
        assert bd.samples == w * h * 4
        assert np.array_equal(bd.units(1), R.budget_units_host(bd.tile_list(), bd.mult(), 1, 1))


@pytest.mark.parametrize("which", ("realm", "rejection", "variant12", "variant30"))
def test_fused_flags_and_variants(env, blocks, which):
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    w, h = 33, 17
    cam = blocks[(w, h)]["cam"]
    flags = {"realm": RT_FLAG_REALM, "rejection": RT_FLAG_REJECTION_SAMPLERS}.get(which, 0)
    variant = {"variant12": 12, "variant30": 30}.get(which)
    with Uploaded(env, env.ref) as ds:
        whole = blocks[(w, h)]["whole"] if not flags else \
            {m: accum_sums(env, ds, cam, w, h, 2 * m, BEGIN, flags=flags) for m in (1, 2, 3, 4)}
        h0, h1, mult = both_ways(env, ds, cam, w, h, pattern_for(w, h), flags=flags, variant=variant, half_spp=1, max_mult=4)
        if which == "variant30":                                 # the prelude on against the default, off
            d0, d1, _ = both_ways(env, ds, cam, w, h, pattern_for(w, h), half_spp=1, max_mult=4)
            assert np.array_equal(h0, d0) and np.array_equal(h1, d1)
    m_px = per_pixel(mult, h, w)
    for m in (1, 2, 3, 4):
        assert np.array_equal((h0 + h1)[m_px == m], whole[m][m_px == m]), (which, m)
    if flags == RT_FLAG_REJECTION_SAMPLERS:
        assert not np.array_equal(whole[1], blocks[(w, h)]["whole"][1])   # the flag reached the kernel


def test_fused_band_and_stream(env, blocks):
    """Rows 8 to 33 of 64 x 40 (a last tile row of one pixel row), on a stream of its own."""
    w, h = 64, 40
    b = blocks[(w, h)]
    raw = pattern_for(w, 25)
    with Uploaded(env, env.ref) as ds:
        h0, h1, mult = both_ways(env, ds, b["cam"], w, h, raw, rows=(8, 33), stream=env.torch.cuda.Stream(), half_spp=1,
                                 max_mult=4)
    assert h0.shape == (25, w, 3) and mult.shape == tiles(25, w)
    m_px = per_pixel(mult, 25, w)
    for m in (1, 2, 3, 4):
        sel = m_px == m
        assert sel.any() and np.array_equal((h0 + h1)[sel], b["whole"][m][8:33][sel]), m


# ---- 2. the refusals ------------------------------------------------------------------------
def test_fused_errors_leave_the_frame_unchanged(env, blocks):
    from rtclj._lib import rt_params
    R, lib = env.R, env.lib
    w, h = 33, 17
    cam = blocks[(w, h)]["cam"]
    raw = pattern_for(w, h)
    d_raw = dev(env, raw, np.uint32)
    with Uploaded(env, env.ref) as ds, R.Budget(ds, w, h, seed=9, half_spp=1, max_mult=4) as bd:
        with pytest.raises(R.RTError, match="plan"):             # a trace without a plan
            bd.trace(ds, cam, sample_begin=BEGIN, fused=True)
        bd.plan_mult(d_raw.data_ptr())
        old = lib.rt_set_variant(28)
        assert old >= 0
        try:
            with pytest.raises(R.RTError, match="8 x 8"):
                bd.trace(ds, cam, sample_begin=BEGIN, fused=True)
        finally:
            lib.rt_set_variant(old)
        with pytest.raises(R.RTError, match="2\\^31"):
            bd.trace(ds, cam, sample_begin=(1 << 31) - 8, fused=True)
        p = rt_params(width=w + 1, height=h, row_begin=0, row_end=h, spp=1, max_depth=50, seed=9, sample_begin=BEGIN)
        assert lib.rt_budget_trace_fused(ds, C.byref(cam), C.byref(p), bd._bd, None, None) == -1
        z0, z1 = bd.halves()
        assert not z0.any() and not z1.any()                     # nothing was traced
        assert bd.trace(ds, cam, sample_begin=BEGIN, fused=True) == 2   # and the plan is still fresh
        h0, h1 = bd.halves()
        m_px = per_pixel(np.clip(raw.astype(np.int64), 1, 4), h, w)
        for m in (1, 2, 3, 4):
            assert np.array_equal((h0 + h1)[m_px == m], blocks[(w, h)]["whole"][m][m_px == m])
        for fused in (True, False):                              # one trace per plan, whichever way
            with pytest.raises(R.RTError, match="plan"):
                bd.trace(ds, cam, sample_begin=BEGIN, fused=fused)
        a0, a1 = bd.halves()
        assert np.array_equal(a0, h0) and np.array_equal(a1, h1)


# ---- 3. the pipeline ------------------------------------------------------------------------
def test_animation_fused_equals_passes(env):
    """render_animation over 3 frames of the rising sphere at 40 x 33 under a
    small orbit: with fused=True every stage, the multipliers included, has the
    bits of fused=False."""
    R = env.R
    w, h, n = 40, 33, 3
    cams = []
    for f in range(n):
        ang = np.radians(0.4) * f
        lf = (-2.0 * np.cos(ang) + 1.0 * np.sin(ang), 2.0, 2.0 * np.sin(ang) + 1.0 * np.cos(ang))
        cams.append(R.camera(w, h, **{**R.REFERENCE_CAMERA, "look_from": lf}))
    scs = [R.Scene.from_bodies(rising(f, n)) for f in range(n)]
    budget = dict(half_spp=1, target=8, max_mult=8, quantile_64=16)
    plain = list(R.render_animation(scs, cams, w, h, seed=5, stages=True, budget=budget))
    fused = list(R.render_animation(scs, cams, w, h, seed=5, stages=True, budget=dict(budget, fused=True)))
    assert len(plain) == len(fused) == n and budget == dict(half_spp=1, target=8, max_mult=8, quantile_64=16)
    seen = set()
    for f, (a, b) in enumerate(zip(plain, fused)):
        assert len(a) == len(b) == 8
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and x.shape == y.shape
            same = np.array_equal(x, y) if x.dtype.kind in "iu" else np.array_equal(bits(x), bits(y))
            assert same, (f, k)
        assert not np.isnan(a[0]).any()
        seen |= set(a[7].ravel().tolist())
    assert len(seen) > 1                                         # the plans were not uniform
