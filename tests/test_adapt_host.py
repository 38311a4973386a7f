"""Adaptive sampling, the host side (no GPU needed): rt_adapt_eval_host is the
stopping rule in plain C++ -- per 8 x 8 tile, over its pixels inside the frame
and their three channels, D = sum |H0 - H1|, S = sum (H0 + H1), converged iff
D * 2^16 <= tol_q16 * S in unbounded integers -- and rt_adapt_resolve_host the
frame's conversion with each tile's own count.  The independent reference of
the rule is its restatement in Python ints (adapt_rule below, which
tests/test_gpu_adapt.py also feeds with the oracle's samples); that of the
conversion is rt_resolve_sums, tile by tile.
"""
import ctypes as C

import numpy as np
import pytest


def adapt_rule(h0, h1, tol_q16):
    """The rule in Python ints: (gy, gx) bools for (rows, width, 3) uint64 halves."""
    rows, width = h0.shape[:2]
    gy, gx = (rows + 7) // 8, (width + 7) // 8
    out = np.zeros((gy, gx), bool)
    for ty in range(gy):
        for tx in range(gx):
            a = [int(v) for v in h0[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].ravel()]
            b = [int(v) for v in h1[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].ravel()]
            d = sum(abs(x - y) for x, y in zip(a, b))
            s = sum(x + y for x, y in zip(a, b))
            out[ty, tx] = (d << 16) <= tol_q16 * s
    return out


def _eval(h0, h1, tol):
    from rtclj._lib import check, lib, u8ptr, u64ptr
    h0, h1 = np.ascontiguousarray(h0, np.uint64), np.ascontiguousarray(h1, np.uint64)
    rows, width = h0.shape[:2]
    out = np.full(((rows + 7) // 8, (width + 7) // 8), 0xa5, np.uint8)
    check(lib.rt_adapt_eval_host(u64ptr(h0), u64ptr(h1), width, rows, tol, u8ptr(out)))
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def _tile(value0, value1):
    return (np.full((8, 8, 3), value0, np.uint64), np.full((8, 8, 3), value1, np.uint64))


def test_equal_and_empty_halves_converge():
    rng = np.random.default_rng(1)
    h = rng.integers(0, 2 ** 40, (8, 8, 3), dtype=np.uint64)
    for tol in (0, 1, 4096, 65536):
        assert _eval(h, h.copy(), tol).all()
        assert _eval(*_tile(0, 0), tol).all()      # 0 <= 0
    h1 = h.copy()
    h1[3, 4, 1] += np.uint64(1)
    assert not _eval(h, h1, 0).any()                # tol 0: only identical halves
    assert _eval(h, h1, 65536).all()                # tol 1: |a - b| <= a + b always
    z = np.zeros((8, 8, 3), np.uint64)
    assert _eval(h, z, 65536).all() and not _eval(h, z, 65535).any()   # D = S


def test_the_bound_is_inclusive_and_exact():
    # S = 192 * 2^16 * 5, tol = 3: tol * S = D * 2^16 at D = 2880
    tol, s_each = 3, 5 << 16
    h0, h1 = _tile(s_each, 0)
    d_want = tol * 192 * s_each >> 16
    assert (d_want << 16) == tol * 192 * s_each
    # move D from S to exactly d_want while keeping S: h0 = a, h1 = b, a + b fixed
    h0[...] = s_each // 2
    h1[...] = s_each // 2                             # D = 0, S as before
    h0[0, 0, 0] += np.uint64(d_want // 2)
    h1[0, 0, 0] -= np.uint64(d_want // 2)             # D = d_want, S unchanged
    assert int(np.abs(h0.astype(np.int64) - h1.astype(np.int64)).sum()) == d_want
    assert adapt_rule(h0, h1, tol).all() and _eval(h0, h1, tol).all()
    h0[7, 7, 2] += np.uint64(1)                       # one unit more of D (and of S: tol * 1 < 2^16)
    assert not adapt_rule(h0, h1, tol).any() and not _eval(h0, h1, tol).any()


def test_sums_near_2_to_56_do_not_overflow():
    big = 2 ** 56 - 1
    # S = 192 * (2^56 - 1) < 2^64; D = S: converged only at tol 65536
    h0, h1 = _tile(big, 0)
    assert _eval(h0, h1, 65536).all() and not _eval(h0, h1, 65535).any()
    # halves 2^55 apart by a little: D * 2^16 needs more than 64 bits
    h0, h1 = _tile(2 ** 55 - 1, 2 ** 55 - 1 - 2 ** 40)
    for tol in (0, 1, 2, 3, 255, 256, 257, 65536):
        assert np.array_equal(_eval(h0, h1, tol), adapt_rule(h0, h1, tol)), tol
    # D / S = 2^40 / (2^56 - 2 - 2^40) per term: tol = 1 (2^-16) is just too small
    assert not _eval(h0, h1, 1).any() and _eval(h0, h1, 2).all()


def test_ragged_tiles_count_their_own_pixels():
    """60 x 36: the right column of tiles is 4 pixels wide, the bottom row 4
    rows high.  Each tile's own pixels decide, whatever the neighbours hold."""
    rng = np.random.default_rng(7)
    w, rows = 60, 36
    base = rng.integers(2 ** 20, 2 ** 24, (rows, w, 3), dtype=np.uint64)
    h0, h1 = base.copy(), base.copy()
    assert _eval(h0, h1, 0).shape == (5, 8) and _eval(h0, h1, 0).all()
    # disagreement in the last full tile column only: the ragged column (x >= 56) still converges
    h1[:, 48:56] += np.uint64(2 ** 19)
    got = _eval(h0, h1, 0)
    assert not got[:, 6].any() and got[:, 7].all() and got[:, :6].all()
    # ... in the ragged corner tile's 4 x 4 pixels only
    h1 = base.copy()
    h1[32:, 56:] += np.uint64(1)
    got = _eval(h0, h1, 0)
    assert not got[4, 7] and got.sum() == got.size - 1
    # a random frame against the Python-int rule, at a tolerance that splits the tiles
    h1 = (base.astype(np.int64) + rng.integers(-2 ** 14, 2 ** 14, base.shape)).astype(np.uint64)
    # (mean |noise| 2^13 against sums of about 1.8e7 a term: D / S is about 30 / 65536)
    mixed = 0
    for tol in (0, *range(24, 37), 65536):
        got = _eval(h0, h1, tol)
        assert np.array_equal(got, adapt_rule(h0, h1, tol)), tol
        mixed += 0 < got.sum() < got.size
    assert mixed >= 3


@pytest.mark.parametrize("flags", [0, 2])
def test_resolve_host_is_resolve_sums_per_tile(flags):
    from rtclj._lib import check, fptr, lib, u32ptr, u64ptr
    rng = np.random.default_rng(3)
    w, rows = 21, 13
    gy, gx = 2, 3
    counts = np.array([[16, 48, 3], [255, 0, 2 ** 24]], np.uint32)
    h0 = rng.integers(0, 2 ** 40, (rows, w, 3), dtype=np.uint64)
    h1 = rng.integers(0, 2 ** 40, (rows, w, 3), dtype=np.uint64)
    got = np.full((rows, w, 3), np.nan, np.float32)
    check(lib.rt_adapt_resolve_host(u64ptr(h0), u64ptr(h1), u32ptr(counts), w, rows, flags, fptr(got)))
    assert not np.isnan(got).any()
    for ty in range(gy):
        for tx in range(gx):
            tot = np.ascontiguousarray((h0 + h1)[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8])
            want = np.full(tot.shape, np.nan, np.float32)
            check(lib.rt_resolve_sums(u64ptr(tot), tot.size, int(counts[ty, tx]), flags, fptr(want)))
            assert np.array_equal(got[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8], want), (ty, tx)
    if flags == 0:   # 3 and 255 are no powers of two: realm's product is another frame there
        other = np.empty_like(got)
        check(lib.rt_adapt_resolve_host(u64ptr(h0), u64ptr(h1), u32ptr(counts), w, rows, 2, fptr(other)))
        assert not np.array_equal(other, got)


GOOD = dict(step_spp=8, min_spp=16, max_spp=64, tol_q16=4096)
BAD = [
    (dict(step_spp=0), b"step_spp"),
    (dict(step_spp=-1), b"step_spp"),
    (dict(min_spp=0), b"min_spp"),
    (dict(min_spp=8), b"min_spp"),            # a multiple of step_spp, not of 2 * step_spp
    (dict(min_spp=24), b"min_spp"),
    (dict(max_spp=0), b"max_spp"),
    (dict(max_spp=72), b"max_spp"),
    (dict(min_spp=80), b"min_spp > max_spp"),
    (dict(max_spp=(1 << 24) + 16), b"RT_MAX_SPP"),
    (dict(tol_q16=65537), b"tol_q16"),
]


@pytest.mark.parametrize("change,word", BAD)
def test_each_violated_option_rule_is_refused(change, word):
    """The options are checked before the scene: a violated rule is RT_E_ARG
    with the rule named, where the good options reach the NULL scene."""
    from rtclj._lib import lib, rt_adapt_opts, rt_params
    p = rt_params(width=16, height=9, row_begin=0, row_end=9)
    ad = C.c_void_p(1)
    o = rt_adapt_opts(**{**GOOD, **change})
    assert lib.rt_adapt_create(None, C.byref(p), C.byref(o), C.byref(ad)) == -1 and not ad.value
    assert word in lib.rt_last_error(), lib.rt_last_error()


def test_good_options_pass_the_option_check():
    from rtclj._lib import lib, rt_adapt_opts, rt_params
    p = rt_params(width=16, height=9, row_begin=0, row_end=9)
    ad = C.c_void_p()
    for change in ({}, dict(tol_q16=0), dict(tol_q16=65536), dict(min_spp=64), dict(step_spp=1, min_spp=2, max_spp=2),
                   dict(step_spp=1 << 23, min_spp=1 << 24, max_spp=1 << 24)):
        o = rt_adapt_opts(**{**GOOD, **change})
        assert lib.rt_adapt_create(None, C.byref(p), C.byref(o), C.byref(ad)) == -1
        assert b"NULL" in lib.rt_last_error(), (change, lib.rt_last_error())


def test_adaptive_entries_without_a_device():
    import rtclj
    from rtclj import raytracing as R
    from rtclj._lib import rt_adapt_opts, rt_params
    lib = rtclj.lib
    cam = R.camera(16, 9, **R.REFERENCE_CAMERA)
    p = rt_params(width=16, height=9, row_begin=0, row_end=9, max_depth=5)
    o = rt_adapt_opts(**GOOD)
    ad = C.c_void_p()
    assert lib.rt_adapt_create(None, None, C.byref(o), C.byref(ad)) == -1
    assert lib.rt_adapt_create(None, C.byref(p), None, C.byref(ad)) == -1
    assert lib.rt_adapt_step(None, C.byref(cam), C.byref(p), None, None, None) == -1
    assert lib.rt_last_error() != b""
    assert lib.rt_adapt_clear(None, None) == -1
    assert lib.rt_adapt_resolve(None, 0, None, None) == -1
    assert lib.rt_adapt_resolve_u8(None, 0, None, None) == -1
    assert lib.rt_adapt_counts(None, None, None) == -1
    assert lib.rt_adapt_read(None, None, None, None) == -1
    assert lib.rt_adapt_active(None) == 0 and lib.rt_adapt_samples(None) == 0
    assert lib.rt_adapt_free(None) == 0
    one = (C.c_uint64 * 192)()
    conv = (C.c_uint8 * 1)()
    assert lib.rt_adapt_eval_host(None, one, 8, 8, 0, conv) == -1
    assert lib.rt_adapt_eval_host(one, one, 0, 8, 0, conv) == -1
    assert lib.rt_adapt_eval_host(one, one, 8, 8, 65537, conv) == -1
    assert lib.rt_adapt_eval_host(one, one, 8, 8, 65536, conv) == 0 and conv[0] == 1
    assert lib.rt_adapt_resolve_host(one, one, None, 8, 8, 0, None) == -1
    if lib.rt_device_count() == 0:
        with pytest.raises(rtclj.RTError):
            R.Adaptive(R.hittables, cam, 16, 9)
        with pytest.raises(rtclj.RTError):
            R.render(R.hittables, cam, 16, 9, adaptive=dict(tol_q16=4096, step=8, min_spp=16, max_spp=64))
