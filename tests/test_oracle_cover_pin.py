"""Oracle pinning, part 3: the kernel's fp32 contract against the reference's
fp64 semantics on the benchmark workload itself (the RTIOW cover scene).

MODE_REF64 restates the Clojure path line by line in double
(raytracing.clj:33-58, 89-155; hittable.clj:9-31; material.clj:13-46;
vec3a.clj:71-101).  MODE_MIRROR32 is the kernel's fp32 contract, which the
GPU equals bit for bit (tests/test_gpu_parity.py).  Both draw from the same
keyed stream, so on the cover scene -- r = 1000 ground, self-hit guard,
unit-direction hit test -- their pixels differ only where an fp32 decision
flips.  Tolerances (written here; measured values in brackets):

  C0 cover 200x112, 10 spp, depth 50 (BASELINE.json configs[0]):
    segments/sample relative |d|      <= 2e-3   [4.2e-4]
    linear mean |d|                   <= 5e-4   [1.4e-4]
    8-bit per-pixel mean |d|          <= 0.25   [0.039]
    8-bit values off by > 1           <= 2 %    [0.65 %]
    16x9 block means (8-bit) mean |d| <= 0.25, max <= 2.5   [0.023 / 0.33]
      (SURVEY.md §8c's block bound for fp64 vs fp32)
  C1 cover 1200x675, 100 spp, depth 50, every 32nd row (22 rows):
    the same bounds                   [7e-6, 1.1e-4, 0.030, 0.25 %, 0.009 / 0.10]

The kernel's default path draws the two samplers loop-free (MODE_MIRROR32 |
DIRECT), so after the first scatter its paths are independent of MODE_REF64's
and the two compare only statistically (oracle/pin.py BOUNDS_INDEPENDENT).
Its same-draw fp64 partner is MODE_REF64D: MODE_REF64 with the two samplers
as their definition in plain double (z = 2 xi1 - 1 or r = sqrt(xi1), the
angle 2 pi u / 2^24, libm) from the same uniforms.  It is held to the same
bounds (measured values in brackets):

  C0, MODE_MIRROR32 | DIRECT vs MODE_REF64D:
    segments/sample 1.8e-4, linear 1.29e-4, 8-bit 0.035, off by > 1 0.59 %,
    block means 0.020 / 0.21
  C1 rows, the same:
    2.7e-4, 1.09e-4, 0.029, 0.23 %, 0.0045 / 0.021
  negative control, the fp64 sphere draw's z scaled by 0.99
  (oracle.sampler_bias): linear mean |d| 1.36e-3 (C0), 8.7e-4 (C1 rows)
  > 5e-4, and off by > 1 7.7 % / 2.15 % > 2 %; the same biased C1 rows
  against MODE_REF64 pass BOUNDS_INDEPENDENT (8-bit per-pixel 2.39 <= 3.5,
  block means 0.123 / 0.50, segments/sample 3.5e-4): the hole this pin closes.
"""
import functools
import os

import numpy as np
import pytest

import oracle


from oracle.pin import BOUNDS_INDEPENDENT, compare, within  # noqa: E402  (the statistics, shared with bench.py)

KERNEL32 = oracle.MODE_MIRROR32 | oracle.DIRECT   # the kernel's default contract


@functools.lru_cache(maxsize=None)
def _render(mode, w, h, spp, rows=None, row_step=1, grid=11, zscale=1.0):
    """Each render once per session (the tests share them and leave them
    unchanged).  zscale: oracle.sampler_bias during this render only."""
    from rtclj import scenes
    sc = scenes.cover(grid)
    cam = scenes.cover_camera(w, h)
    oracle.sampler_bias(zscale)
    try:
        out, _, segs, smp = oracle.render(mode, sc.sphere.astype(np.float64), sc.kind, sc.mat.astype(np.float64),
                                          cam.as_list(), cam.defocus, w, h, spp, 50, seed=1, rows=rows,
                                          row_step=row_step, nthreads=min(16, os.cpu_count() or 1))
    finally:
        oracle.sampler_bias(1.0)
    out.setflags(write=False)
    return out, segs / smp


def test_c0_cover_mirror32_tracks_ref64():
    a, s64 = _render(oracle.MODE_REF64, 200, 112, 10)
    b, s32 = _render(oracle.MODE_MIRROR32, 200, 112, 10)
    st = compare(a, s64, b, s32, by=9)
    ok = within(st)
    assert all(ok.values()), (ok, st)
    assert 2.6 < s64 < 2.75          # SURVEY.md §3.2 probe: 2.63 segments/sample on the cover scene


def test_c1_rows_mirror32_tracks_ref64():
    a, s64 = _render(oracle.MODE_REF64, 1200, 675, 100, row_step=32)
    b, s32 = _render(oracle.MODE_MIRROR32, 1200, 675, 100, row_step=32)
    assert a.shape == (22, 1200, 3)
    st = compare(a, s64, b, s32, by=2)
    ok = within(st)
    assert all(ok.values()), (ok, st)


def test_c0_cover_direct_mirror_tracks_ref64d():
    """The default path's contract against its same-draw fp64 reference."""
    a, s64 = _render(oracle.MODE_REF64D, 200, 112, 10)
    b, s32 = _render(KERNEL32, 200, 112, 10)
    st = compare(a, s64, b, s32, by=9)
    print("C0 MIRROR32|DIRECT vs REF64D:", st)
    ok = within(st)
    assert all(ok.values()), (ok, st)
    assert 2.6 < s64 < 2.75


def test_c1_rows_direct_mirror_tracks_ref64d():
    a, s64 = _render(oracle.MODE_REF64D, 1200, 675, 100, row_step=32)
    b, s32 = _render(KERNEL32, 1200, 675, 100, row_step=32)
    assert a.shape == b.shape == (22, 1200, 3)
    st = compare(a, s64, b, s32, by=2)
    print("C1 rows MIRROR32|DIRECT vs REF64D:", st)
    ok = within(st)
    assert all(ok.values()), (ok, st)


def test_ref64d_pin_rejects_a_one_percent_sampler_bias():
    """Negative control: a 1 % squeeze of the unit-sphere draw's z in the fp64
    reference (a bias of the lambertian and metal lobes) fails the same-draw
    bounds on C0 and on the C1 rows, and the unbiased reference passes them
    (the two tests above).  The hole this closes, recorded once: the same
    biased C1 rows still pass the independent-draw bounds against MODE_REF64,
    which were the default path's only fp64 check."""
    assert oracle.sampler_bias() == 1.0
    b0, t0 = _render(KERNEL32, 200, 112, 10)
    a0, s0 = _render(oracle.MODE_REF64D, 200, 112, 10, zscale=0.99)
    b1, t1 = _render(KERNEL32, 1200, 675, 100, row_step=32)
    a1, s1 = _render(oracle.MODE_REF64D, 1200, 675, 100, row_step=32, zscale=0.99)
    assert oracle.sampler_bias() == 1.0
    for name, st in (("C0", compare(a0, s0, b0, t0, by=9)), ("C1 rows", compare(a1, s1, b1, t1, by=2))):
        print(name, "biased REF64D:", st)
        ok = within(st)
        assert not all(ok.values()) and not ok["lin_mean"], (name, ok, st)
    r, sr = _render(oracle.MODE_REF64, 1200, 675, 100, row_step=32)
    st = compare(r, sr, a1, s1, by=2)
    print("C1 rows biased REF64D vs REF64 (independent draws):", st)
    ok = within(st, BOUNDS_INDEPENDENT)
    assert all(ok.values()), (ok, st)


def test_pin_discriminates_semantics():
    """Negative control: the book's normalised-metal reflect (MODE_BOOK64) on
    the same cover frame is far outside these bounds (the cover scene's
    metal bodies carry it)."""
    a, s64 = _render(oracle.MODE_REF64, 200, 112, 10)
    c, sb = _render(oracle.MODE_BOOK64, 200, 112, 10)
    ok = within(compare(a, s64, c, sb, by=9))
    assert not all(ok.values())


def test_c4_scene_is_1000_bodies():
    from rtclj import scenes
    full, c4 = scenes.cover(16), scenes.cover_c4()
    assert len(full) == 1025 and len(c4) == 1000
    assert np.array_equal(c4.sphere[:997], full.sphere[:997]) and np.array_equal(c4.sphere[-3:], full.sphere[-3:])
    assert c4.sphere[0, 3] == 1000.0 and (c4.sphere[-3:, 3] == 1.0).all()
