"""ctypes wrapper of oracle/_build/liboracle.so — TEST INFRASTRUCTURE ONLY.

Parity status: pinned statistically against the reference's own render
(its scene.ppm -> tests/golden/scene_ppm.npz, scene_ppm_stats.json)
and by hand-derived known answers (tests/golden/kats.json).  The reference's
RNG is unseeded java.util.Random, so no bitwise reference image can exist.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
LIB = HERE / "_build" / "liboracle.so"
MODE_REF64, MODE_MIRROR32, MODE_BOOK64, MODE_REALM64, MODE_REALM32 = 0, 1, 2, 3, 4
# MODE_REF64 / MODE_REALM64 with the two samplers drawn loop-free in plain
# double from the same uniforms as the kernel's: the same-draw fp64 partners
# of MODE_MIRROR32 | DIRECT / MODE_REALM32 | DIRECT.  They take no DIRECT bits.
MODE_REF64D, MODE_REALM64D = 5, 6
MODES64 = (MODE_REF64, MODE_BOOK64, MODE_REALM64, MODE_REF64D, MODE_REALM64D)
# ored into MODE_MIRROR32 / MODE_REALM32: the kernel's loop-free samplers
# (its default, i.e. without RT_FLAG_REJECTION_SAMPLERS): the unit-sphere
# draw, the defocus disk, both
DIRECT_SPHERE, DIRECT_DISK = 0x10, 0x20
DIRECT = DIRECT_SPHERE | DIRECT_DISK

_dll = None


def build(force: bool = False) -> Path:
    if force or not LIB.exists() or LIB.stat().st_mtime < (HERE / "rt_oracle.cpp").stat().st_mtime:
        subprocess.run(["make", "-C", str(HERE)], check=True, capture_output=True)
    return LIB


def _lib():
    global _dll
    if _dll is None:
        build()
        d = C.CDLL(str(LIB))
        dp, ip, fp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        d.oracle_render.restype = C.c_int
        d.oracle_render.argtypes = [C.c_int, C.c_int, dp, ip, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, fp, dp, u64p]
        d.oracle_render_cols.restype = C.c_int
        d.oracle_render_cols.argtypes = [C.c_int, C.c_int, dp, ip, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                         C.c_int, fp, dp, u64p]
        d.oracle_features.restype = C.c_int
        d.oracle_features.argtypes = [C.c_int, C.c_int, dp, ip, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_uint32), fp, dp, C.POINTER(C.c_int32), dp, fp]
        d.oracle_sphere_hit.restype = C.c_int
        d.oracle_sphere_hit.argtypes = [dp, dp, dp, C.c_double, C.c_double, dp]
        d.oracle_reflect.argtypes = [dp, dp, dp]
        d.oracle_refract.argtypes = [dp, dp, C.c_double, dp]
        d.oracle_reflectance.restype = C.c_double
        d.oracle_reflectance.argtypes = [C.c_double, C.c_double]
        d.oracle_quantize.restype = C.c_int
        d.oracle_quantize.argtypes = [C.c_double]
        d.oracle_camera.argtypes = [C.c_int, C.c_int, C.c_double, dp, dp, dp, C.c_double, C.c_double, dp]
        d.oracle_lambertian_dir.argtypes = [dp, dp, dp]
        d.oracle_metal_dir.restype = C.c_int
        d.oracle_metal_dir.argtypes = [dp, dp, C.c_double, dp, dp]
        d.oracle_dielectric_dir.restype = C.c_int
        d.oracle_dielectric_dir.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, dp]
        d.oracle_rng_stream.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, fp]
        d.oracle_sampler_draws.restype = C.c_int
        d.oracle_sampler_draws.argtypes = [C.c_int, C.c_uint64, C.c_int, fp]
        d.oracle_turn24.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_float, fp]
        d.oracle_sampler_draws64.restype = C.c_int
        d.oracle_sampler_draws64.argtypes = [C.c_int, C.c_uint64, C.c_int, dp]
        d.oracle_direct_from_uniforms.restype = C.c_int
        d.oracle_direct_from_uniforms.argtypes = [C.c_int, C.c_int, fp, C.POINTER(C.c_uint32), fp, dp]
        d.oracle_set_sampler_bias.restype = None
        d.oracle_set_sampler_bias.argtypes = [C.c_double]
        d.oracle_get_sampler_bias.restype = C.c_double
        d.oracle_get_sampler_bias.argtypes = []
        _dll = d
    return _dll


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def render(mode, sphere, kind, mat, cam, defocus, width, height, spp, max_depth, seed=1, rows=None,
           sample_begin=0, nthreads=0, want64=False, row_step=1, cols=None):
    """Render rows r0, r0+row_step, ... < r1 (default all) -> (float32 (rows,W,3),
    float64 or None, segments, samples).  cols=(c0, c1): only those columns
    of the rows (the others NaN; samples counts the rendered pixels')."""
    r0, r1 = (0, height) if rows is None else rows
    nrows = (r1 - r0 + row_step - 1) // row_step
    sph, sp = _d(np.asarray(sphere, np.float64).reshape(-1, 4))
    mt, mp = _d(np.asarray(mat, np.float64).reshape(-1, 4))
    kd = np.ascontiguousarray(kind, np.int32).reshape(-1)
    cm, cp = _d(np.asarray(cam, np.float64).reshape(18))
    c0, c1 = (0, width) if cols is None else cols
    out = np.full((nrows, width, 3), np.nan, np.float32)
    out64 = np.full((nrows, width, 3), np.nan, np.float64) if want64 else None
    cnt = np.zeros(2, np.uint64)
    rc = _lib().oracle_render_cols(mode, len(kd), sp, kd.ctypes.data_as(C.POINTER(C.c_int)), mp, cp, int(defocus),
                                   width, height, r0, r1, row_step, c0, c1, spp, sample_begin, max_depth, seed,
                                   nthreads, out.ctypes.data_as(C.POINTER(C.c_float)),
                                   out64.ctypes.data_as(C.POINTER(C.c_double)) if want64 else None,
                                   cnt.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise ValueError(f"oracle_render rejected its arguments (rc={rc})")
    return out, out64, int(cnt[0]), int(cnt[1])


def features(mode, sphere, kind, mat, cam, defocus, width, height, spp, seed=1, rows=None, sample_begin=0,
             nthreads=0, row_step=1, want_body=False, want_t=False, want_rays=False):
    """The first-hit feature pass (include/rt.h, rt_launch_feat) of rows r0,
    r0+row_step, ... < r1 (default all), samples sample_begin ... + spp - 1 -> dict.
    MODE_MIRROR32 (| DIRECT bits), what rt_feat_read returns bit for bit:
      sums int64 (rows, W, 6), hits uint32 (rows, W), depth float32 (rows, W).
    MODE_REF64D (MODE_REF64: the rejection disk), the same draws in double:
      albedo, normal float64 (rows, W, 3) means over the samples (the sky on a
      miss, normal 0), depth float64 (min t |d|, +inf: none), hits uint32.
    want_body: body int32 (rows, W, spp), -1 a miss; want_t: t float64, the
    same shape (+inf a miss); want_rays (mirror): rays float32 (..., spp, 6), (o, d)."""
    r0, r1 = (0, height) if rows is None else rows
    nrows = (r1 - r0 + row_step - 1) // row_step
    sph, sp = _d(np.asarray(sphere, np.float64).reshape(-1, 4))
    mt, mp = _d(np.asarray(mat, np.float64).reshape(-1, 4))
    kd = np.ascontiguousarray(kind, np.int32).reshape(-1)
    cm, cp = _d(np.asarray(cam, np.float64).reshape(18))
    fp64 = (mode & 0xf) in (MODE_REF64, MODE_REF64D)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    sums = hits = depth = mean = body = t = rays = None
    if fp64:
        mean = np.full((nrows, width, 8), np.nan, np.float64)
    else:
        sums = np.full((nrows, width, 6), -1, np.int64)
        hits = np.full((nrows, width), 0xffffffff, np.uint32)
        depth = np.full((nrows, width), np.nan, np.float32)
    if want_body:
        body = np.full((nrows, width, max(spp, 0)), -2, np.int32)
    if want_t:
        t = np.full((nrows, width, max(spp, 0)), np.nan, np.float64)
    if want_rays:
        rays = np.full((nrows, width, max(spp, 0), 6), np.nan, np.float32)

    def ptr(a, ty):
        return None if a is None else a.ctypes.data_as(ty)
    rc = _lib().oracle_features(mode, len(kd), sp, kd.ctypes.data_as(C.POINTER(C.c_int)), mp, cp, int(defocus),
                                width, height, r0, r1, row_step, spp, sample_begin, seed, nthreads,
                                ptr(sums, C.POINTER(C.c_int64)), ptr(hits, C.POINTER(C.c_uint32)), ptr(depth, fp),
                                ptr(mean, dp), ptr(body, C.POINTER(C.c_int32)), ptr(t, dp), ptr(rays, fp))
    if rc != 0:
        raise ValueError(f"oracle_features rejected its arguments (rc={rc})")
    if fp64:
        out = dict(albedo=mean[..., 0:3], normal=mean[..., 3:6], depth=mean[..., 6], hits=mean[..., 7].astype(np.uint32))
    else:
        out = dict(sums=sums, hits=hits, depth=depth)
    if want_body:
        out["body"] = body
    if want_t:
        out["t"] = t
    if want_rays:
        out["rays"] = rays
    return out


def sphere_hit(sphere4, o, d, tmin, tmax):
    s, sp = _d(sphere4)
    oo, op = _d(o)
    dd, dp = _d(d)
    out, outp = _d(np.zeros(9))
    _lib().oracle_sphere_hit(sp, op, dp, tmin, tmax, outp)
    return dict(hit=bool(out[0]), t=out[1], p=out[2:5].tolist(), n=out[5:8].tolist(), front=bool(out[8]))


def reflect(v, n):
    a, ap = _d(v)
    b, bp = _d(n)
    o, op = _d(np.zeros(3))
    _lib().oracle_reflect(ap, bp, op)
    return o.tolist()


def refract(uv, n, eta):
    a, ap = _d(uv)
    b, bp = _d(n)
    o, op = _d(np.zeros(3))
    _lib().oracle_refract(ap, bp, eta, op)
    return o.tolist()


def reflectance(cosine, ri):
    return _lib().oracle_reflectance(cosine, ri)


def quantize(c):
    return _lib().oracle_quantize(c)


def camera(w, h, vfov, look_from, look_at, vup, defocus_angle, focus_dist):
    lf, lp = _d(look_from)
    la, ap = _d(look_at)
    up, upp = _d(vup)
    o, op = _d(np.zeros(18))
    _lib().oracle_camera(w, h, vfov, lp, ap, upp, defocus_angle, focus_dist, op)
    return o


def rng_stream(seed, pixel, sample, n):
    out = np.zeros(n, np.float32)
    _lib().oracle_rng_stream(seed, pixel, sample, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def lambertian_dir(unit, n):
    a, ap = _d(unit)
    b, bp = _d(n)
    o, op = _d(np.zeros(3))
    _lib().oracle_lambertian_dir(ap, bp, op)
    return o.tolist()


def metal_dir(d, n, fuzz, unit):
    a, ap = _d(d)
    b, bp = _d(n)
    u, up = _d(unit)
    o, op = _d(np.zeros(3))
    ok = _lib().oracle_metal_dir(ap, bp, fuzz, up, op)
    return bool(ok), o.tolist()


def dielectric_dir(d, n, front, eta, xi):
    a, ap = _d(d)
    b, bp = _d(n)
    o, op = _d(np.zeros(3))
    refl = _lib().oracle_dielectric_dir(ap, bp, int(front), eta, xi, op)
    return bool(refl), o.tolist()


SAMPLERS = {"sphere_rejection": 0, "sphere_direct": 1, "disk_rejection": 2, "disk_direct": 3}


def sampler_draws(which, seed, n):
    """n consecutive draws of one sampler from the keyed stream (seed, 0, 0):
    (n, 3) float32 (the disk's z = 0).  which: a SAMPLERS key."""
    out = np.zeros((n, 3), np.float32)
    if _lib().oracle_sampler_draws(SAMPLERS[which], seed, n, out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise ValueError(which)
    return out


def sampler_draws64(which, seed, n):
    """sampler_draws' stream through the fp64 loop-free samplers
    ("sphere_direct" / "disk_direct" in plain double): (n, 3) float64."""
    out = np.zeros((n, 3), np.float64)
    if _lib().oracle_sampler_draws64(SAMPLERS[which], seed, n, out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise ValueError(which)
    return out


def direct_from_uniforms(which, xi1, u):
    """One loop-free sampler in both precisions for given uniforms: xi1 (draws,
    k / 2^24, float32) and the next step's 24-bit integers u ->
    ((n, 3) float32 as the kernel computes it, (n, 3) float64 by definition)."""
    xi1 = np.ascontiguousarray(xi1, np.float32).reshape(-1)
    u = np.ascontiguousarray(u, np.uint32).reshape(-1)
    assert len(xi1) == len(u)
    o32, o64 = np.zeros((len(u), 3), np.float32), np.zeros((len(u), 3), np.float64)
    if _lib().oracle_direct_from_uniforms(SAMPLERS[which], len(u), xi1.ctypes.data_as(C.POINTER(C.c_float)),
                                          u.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          o32.ctypes.data_as(C.POINTER(C.c_float)),
                                          o64.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise ValueError(which)
    return o32, o64


def sampler_bias(zscale=1.0):
    """TEST-ONLY negative control: multiply the fp64 loop-free sphere draw's z
    (MODE_REF64D / MODE_REALM64D, sampler_draws64) by zscale before r is
    formed.  Process-wide, read at the start of a render; 1 is unbiased.
    Callers reset it in a `finally`.  Returns the previous value."""
    old = _lib().oracle_get_sampler_bias()
    _lib().oracle_set_sampler_bias(float(zscale))
    return old


def turn24(u, r=1.0):
    """The kernel's (r cos, r sin) of 2 pi u / 2^24 for 24-bit integers u: (n, 2) float32."""
    u = np.ascontiguousarray(u, np.uint32).reshape(-1)
    out = np.zeros((len(u), 2), np.float32)
    _lib().oracle_turn24(len(u), u.ctypes.data_as(C.POINTER(C.c_uint32)), r, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out
