"""Progressive rendering, the host side (no GPU needed): rt_resolve_sums is
the accumulator's conversion in plain C++ -- RN(float(sum)) * 2^-24, then
/ RN(float(n)) (realm: * (1 / RN(float(n)))) -- and shard.combine_exact adds
the ranks' integer sums before it, so that sample stripes combine to exactly
the one-launch frame where the float average does not.

The integer sums of a stripe are made from the oracle's fp32 mirror one sample
at a time: a 1-spp mirror frame is RN(float(fix24 sum)) * 2^-24 / 1 with a sum
of at most 2^24 (the reference scene's colours lie in [0, 1]), which a float
holds exactly, so frame * 2^24 is the sample's integer.  (The mirror fills its
float64 output only in the fp64 modes; its want64 array stays NaN here.)
"""
import ctypes as C

import numpy as np
import pytest

SUMS = [0, 1, 2 ** 24, 2 ** 53 + 1, 2 ** 63,
        2 ** 60 + 2 ** 36 + 1]   # (just past a float tie: rounding through a double first would go down)
COUNTS = [1, 3, 255, 256, 2 ** 24, 2 ** 24 + 1]


def _resolve(sums, n, flags=0):
    from rtclj._lib import check, fptr, lib, u64ptr
    sums = np.ascontiguousarray(sums, np.uint64)
    out = np.full(sums.shape, np.nan, np.float32)
    check(lib.rt_resolve_sums(u64ptr(sums), sums.size, n, flags, fptr(out)))
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_resolve_sums_is_the_numpy_restatement(n):
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    sums = np.array(SUMS + [2 ** 24 * n], np.uint64)
    tot = sums.astype(np.float32) * np.float32(2.0 ** -24)     # RN(float(sum)), an exact scale
    nf = np.array([n], np.uint64).astype(np.float32)[0]         # RN(float(n))
    want = tot / nf
    want_realm = tot * (np.float32(1.0) / nf)
    assert want.dtype == np.float32 and want_realm.dtype == np.float32
    got = _resolve(sums, n)
    assert np.array_equal(got, want), (n, got, want)
    assert np.array_equal(_resolve(sums, n, RT_FLAG_REALM), want_realm), n
    # the resolve reads the realm flag only
    assert np.array_equal(_resolve(sums, n, RT_FLAG_REJECTION_SAMPLERS), want), n
    if n in (3, 255):   # not a power of two: the quotient and the product differ somewhere
        many = np.arange(1, 4097, dtype=np.uint64) * np.uint64(4099)
        assert not np.array_equal(_resolve(many, n), _resolve(many, n, RT_FLAG_REALM))
    # 2^24 is colour 1: 1 / n; n samples of colour 1: 1 (for 2^24 + 1 both the
    # sum 2^48 + 2^24 and the count round to even, down)
    assert got[2] == np.float32(1.0) / nf and got[-1] == 1.0


def test_resolve_sums_edges():
    from rtclj._lib import lib
    # no samples: n = max(count, 1)
    assert np.array_equal(_resolve([0, 2 ** 24, 3 * 2 ** 23], 0), np.array([0.0, 1.0, 1.5], np.float32))
    one = (C.c_uint64 * 1)(5)
    f = (C.c_float * 1)()
    assert lib.rt_resolve_sums(None, 0, 1, 0, None) == 0
    assert lib.rt_resolve_sums(None, 1, 1, 0, f) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_resolve_sums(one, 1, 1, 0, None) == -1
    assert lib.rt_resolve_sums(one, 1, -1, 0, f) == -1
    assert lib.rt_resolve_sums(one, 1, 2 ** 32, 0, f) == -1
    assert lib.rt_resolve_sums(one, 1, 2 ** 32 - 1, 0, f) == 0
    assert lib.rt_resolve_sums(one, 1, 1, 64, f) == -1 and b"flags" in lib.rt_last_error()


@pytest.fixture(scope="module")
def stripes():
    """The reference scene at 40 x 22 through the fp32 mirror: the 8-spp
    frame, the 4-spp frames of stripes [0, 4) and [4, 8), and the stripes'
    integer sums (eight 1-spp frames x 2^24)."""
    import oracle
    from rtclj import raytracing as R
    w, h = 40, 22
    sc = R.Scene.from_bodies(R.hittables)
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    mode = oracle.MODE_MIRROR32 | oracle.DIRECT

    def mirror(spp, begin):
        return oracle.render(mode, sc.sphere.astype(np.float64), sc.kind, sc.mat.astype(np.float64), cam.as_list(),
                             cam.defocus, w, h, spp, 50, seed=9, sample_begin=begin)[0]
    ones = []
    for k in range(8):
        f = mirror(1, k).astype(np.float64) * 2.0 ** 24
        assert np.array_equal(f, np.floor(f)) and f.min() >= 0 and f.max() <= 2 ** 24   # exact integers
        ones.append(f.astype(np.uint64))
    sums = [sum(ones[:4]), sum(ones[4:])]
    return dict(full=mirror(8, 0), half=[mirror(4, 0), mirror(4, 4)], sums=sums)


def test_combine_exact_equals_the_one_launch_frame(stripes):
    from rtclj.shard import combine_exact
    full, (a, b), sums = stripes["full"], stripes["half"], stripes["sums"]
    # each stripe's integers resolve to that stripe's mirror frame
    assert np.array_equal(combine_exact([sums[0]], 4), a)
    assert np.array_equal(combine_exact([sums[1]], 4), b)
    got = combine_exact(sums, 8)
    assert got.dtype == np.float32 and np.array_equal(got, full)
    assert np.array_equal(combine_exact(sums[::-1], 8), full)
    # the float average of the stripes' frames is not that frame: close, not equal
    avg = (a + b) * np.float32(0.5)
    differ = int((avg != full).sum())
    print(f"float average: {differ} of {full.size} channels differ, max |d| {np.abs(avg - full).max():.3e}")
    assert differ > 0
    assert np.allclose(avg, full, rtol=0, atol=2e-6)


def test_combine_exact_realm_and_arguments(stripes):
    from rtclj._lib import RT_FLAG_REALM
    from rtclj.shard import combine_exact
    sums = stripes["sums"]
    total = sums[0] + sums[1]
    assert np.array_equal(combine_exact(sums, 7, realm=True), _resolve(total, 7, RT_FLAG_REALM))
    assert not np.array_equal(combine_exact(sums, 7, realm=True), combine_exact(sums, 7))
    with pytest.raises(ValueError):
        combine_exact([], 8)
    with pytest.raises(ValueError):
        combine_exact([sums[0], sums[1][:5]], 8)


def test_accumulator_entries_without_a_device():
    """As test_abi.py's neighbours: no device scene can exist here, so every
    entry that needs one refuses its NULLs (RT_E_ARG) or the device
    (RT_E_NODEV), with a message."""
    import rtclj
    from rtclj import raytracing as R
    from rtclj._lib import rt_params
    lib = rtclj.lib
    cam = R.camera(16, 9, **R.REFERENCE_CAMERA)
    p = rt_params(width=16, height=9, row_begin=0, row_end=9, spp=1, max_depth=5)
    acc = C.c_void_p()
    assert lib.rt_launch_accum(None, C.byref(cam), C.byref(p), None, None, None) in (-1, -5)
    assert lib.rt_last_error() != b""
    assert lib.rt_accum_create(None, C.byref(p), C.byref(acc)) in (-1, -5) and not acc.value
    assert lib.rt_accum_clear(None, None) == -1
    assert lib.rt_accum_resolve(None, 0, None, None) == -1
    assert lib.rt_accum_resolve_u8(None, 0, None, None) == -1
    assert lib.rt_accum_read(None, None, None) == -1
    assert lib.rt_accum_add(None, None, 1, None) == -1
    assert lib.rt_accum_samples(None) == 0
    assert lib.rt_accum_free(None) == 0
    if lib.rt_device_count() == 0:
        with pytest.raises(rtclj.RTError) as ei:
            R.Progressive(R.hittables, cam, 16, 9)
        assert ei.value.code in (-4, -5)   # (rt_scene_upload: the HIP runtime's own "no device", or NODEV)
        with pytest.raises(rtclj.RTError):
            R.render(R.hittables, cam, 16, 9, spp=4, passes=2)


def test_pass_sizes():
    from rtclj.raytracing import pass_sizes
    assert pass_sizes(100, 4) == [25, 25, 25, 25]
    assert pass_sizes(10, 4) == [3, 3, 2, 2]
    assert pass_sizes(3, 8) == [1, 1, 1]
    assert pass_sizes(5, 0) == [5] and pass_sizes(0, 3) == [0]
