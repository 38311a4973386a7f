"""First-hit feature buffers on the device (include/rt.h, rt_feat): albedo,
normal, depth and coverage of the first surface each camera ray meets, as
exact integer sums -- known answers, the same rays as the path kernel,
geometry in float64, order-freedom, the contract's edges and the hosts.
Every resolve goes into a NaN-filled buffer: no NaN may remain.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_MAIN = ROOT / "raytracing-clj_amd" / "lib" / "rt_main"
OCC_SHAPES = (("ref", 400, 225, 100), ("cover", 1200, 675, 100))   # tests/test_gpu_accum.py::OCC_SHAPES
ONE = 1 << 24
INF_BITS = 0x7f800000
K_BOUND = 6e-4   # bvh_pad.h: the fp32 body test's point lies within 6e-4 * (t + 3 r) of the surface (3x margin)


class Env:
    pass


def _occupancy(ds, w, h, spp):
    from rtclj._lib import check, lib, rt_params
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=50, seed=1)
    out4 = (C.c_int * 4)()
    check(lib.rt_launch_occupancy(ds, C.byref(p), out4))
    return tuple(out4)


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    from rtclj import scenes
    from rtclj._lib import check, lib
    e = Env()
    e.torch = torch
    e.sc = R.Scene.from_bodies(R.hittables)
    e.cover = scenes.cover(11)
    e.ds, e.ds_cover = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(e.sc.c), C.byref(e.ds)))
    check(lib.rt_scene_upload(0, C.byref(e.cover.c), C.byref(e.ds_cover)))
    # before the module's first feature launch
    e.occ_before = {name: _occupancy(e.ds if name == "ref" else e.ds_cover, w, h, spp)
                    for name, w, h, spp in OCC_SHAPES}
    yield e
    lib.rt_scene_free(e.ds)
    lib.rt_scene_free(e.ds_cover)


def _upload(scene):
    from rtclj._lib import check, lib
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(scene.c), C.byref(ds)))
    return ds


def _scene(bodies):
    """[(cx, cy, cz, r, kind, (a, b, c))] -> Scene."""
    from rtclj import raytracing as R
    n = len(bodies)
    sph, kind, mat = np.zeros((n, 4), np.float32), np.zeros(n, np.int32), np.zeros((n, 4), np.float32)
    for i, (x, y, z, r, k, alb) in enumerate(bodies):
        sph[i], kind[i], mat[i, :3] = (x, y, z, r), k, alb
        if k == 2:
            mat[i] = (0, 0, 0, 1.5)
    return R.Scene(sph, kind, mat)


def _cam(w, h, wide=False):
    """The reference camera (its defocus included).  Its 20 degrees see the
    ground and the bodies only; `wide` opens it to 80, which adds the sky."""
    from rtclj import raytracing as R
    return R.camera(w, h, **dict(R.REFERENCE_CAMERA, vfov=80.0 if wide else 20.0))


def _params(w, h, spp, begin=0, seed=9, flags=0, depth=1, **kw):
    from rtclj._lib import rt_params
    return rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=depth, seed=seed,
                     sample_begin=begin, flags=flags, **kw)


def _sptr(env, stream):
    s = stream or env.torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _launch(env, cam, p, ds=None):
    """rt_launch of p -> frame."""
    from rtclj._lib import lib
    torch = env.torch
    shape = (lib.rt_rows_out(C.byref(p)), p.width, 3)
    out = torch.full((int(np.prod(shape)),), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.rt_launch(ds or env.ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), None, _sptr(env, None))
    assert rc == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    frame = out.cpu().numpy().reshape(shape)
    assert not np.isnan(frame).any()
    return frame


class Feat:
    """An rt_feat and the device buffer its resolves write."""

    def __init__(self, env, p, ds=None):
        from rtclj._lib import check, lib
        self.env, self.ds = env, ds or env.ds
        self.rows, self.w = lib.rt_rows_out(C.byref(p)), p.width
        self.h = C.c_void_p()
        check(lib.rt_feat_create(self.ds, C.byref(p), C.byref(self.h)))
        self.cnt = env.torch.zeros(2, dtype=env.torch.int64, device="cuda")
        env.torch.cuda.synchronize()

    def add(self, cam, p, stream=None, counters=True):
        from rtclj._lib import lib
        rc = lib.rt_launch_feat(self.ds, C.byref(cam), C.byref(p), self.h,
                                C.c_void_p(self.cnt.data_ptr()) if counters else None, _sptr(self.env, stream))
        assert rc == 0, lib.rt_last_error()
        return self

    @property
    def samples(self):
        from rtclj._lib import lib
        return lib.rt_feat_samples(self.h)

    def counters(self):
        self.env.torch.cuda.synchronize()
        return self.cnt.cpu().numpy().tolist()

    def read(self):
        """(sums int64 (rows, w, 6), hits uint32, depth float32), after every stream's passes."""
        from rtclj._lib import check, fptr, i64ptr, lib, u32ptr
        self.env.torch.cuda.synchronize()
        sums = np.full((self.rows, self.w, 6), -1, np.int64)
        hits = np.full((self.rows, self.w), 0xffffffff, np.uint32)
        depth = np.full((self.rows, self.w), np.nan, np.float32)
        check(lib.rt_feat_read(self.h, i64ptr(sums), u32ptr(hits), fptr(depth), _sptr(self.env, None)))
        assert not np.isnan(depth).any()
        return sums, hits, depth

    def frame(self):
        """rt_feat_resolve into a NaN-filled buffer; equal to rt_feat_resolve_host of read()."""
        from rtclj._lib import check, fptr, i64ptr, lib, u32ptr
        torch = self.env.torch
        torch.cuda.synchronize()
        n = self.rows * self.w * 8
        out = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")   # 8 guard floats behind
        rc = lib.rt_feat_resolve(self.h, C.c_void_p(out.data_ptr()), _sptr(self.env, None))
        assert rc == 0, lib.rt_last_error()
        torch.cuda.synchronize()
        f = out.cpu().numpy()
        assert np.isnan(f[n:]).all()
        f = f[:n].reshape(self.rows, self.w, 8)
        assert not np.isnan(f).any()
        sums, hits, depth = self.read()
        host = np.full(f.shape, np.nan, np.float32)
        check(lib.rt_feat_resolve_host(i64ptr(sums), u32ptr(hits), fptr(depth), hits.size, self.samples, fptr(host)))
        assert np.array_equal(host.view(np.uint32), f.view(np.uint32))
        return f

    def free(self):
        from rtclj._lib import lib
        lib.rt_feat_free(self.h)
        self.h = C.c_void_p()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _with_variant(v, fn):
    from rtclj._lib import lib
    old = lib.rt_set_variant(v)
    assert old >= 0
    try:
        return fn()
    finally:
        lib.rt_set_variant(old)


def _source(ds):
    from rtclj._lib import check, lib
    out4 = (C.c_int * 4)()
    check(lib.rt_feat_occupancy(ds, out4))
    return out4[3]


def fix24(c):
    """c * 2^24 toward zero (c a float32 in [0, 256))."""
    return int(np.float32(c) * np.float32(ONE))


# ---- 1: known answers ---------------------------------------------------------------
def _fixed_cam():
    """du = dv = 0, no defocus: every sample of every pixel is the ray (0,0,0) -> (0,0,-1)."""
    from rtclj._lib import rt_camera
    cam = rt_camera()
    cam.p00[2] = -1.0
    return cam


A = (0.25, 0.5, 0.75)
SKY = (0.75, float(np.float32(0.5) * np.float32(0.7) + np.float32(0.5)), 1.0)   # uy = 0: sa = om = 0.5
KNOWN = {
    # name: (bodies, hits, depth (None: see the test), normal z, albedo)
    "sphere": ([(0, 0, -3, 1, 0, A)], 4, 2.0, 1, A),
    "metal": ([(0, 0, -3, 1, 1, A)], 4, 2.0, 1, A),
    "back_face": ([(0, 0, 0, 2, 0, A)], 4, 2.0, 1, A),
    "negative_radius": ([(0, 0, -3, -1, 0, A)], 4, 2.0, 1, A),
    "identical_first_wins": ([(0, 0, -3, 1, 0, A), (0, 0, -3, 1, 0, (1.0, 0.125, 0.0))], 4, 2.0, 1, A),
    "dielectric": ([(0, 0, -3, 1, 2, (0, 0, 0))], 4, 2.0, 1, (1.0, 1.0, 1.0)),
    "no_material": ([(0, 0, -3, 1, 3, A)], 4, 2.0, 1, (0.0, 0.0, 0.0)),
    "far_root": ([(0, 0, -1.0005, 1, 0, A)], 4, None, 1, A),
    "nearest_of_many": ([(0, 0, -9 - i, 1, 0, (1.0, 0.125, 0.0)) for i in range(9)] + [(0, 0, -3, 1, 0, A)],
                        4, 2.0, 1, A),
    "no_body": ([], 0, np.inf, 0, SKY),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(env, name):
    from rtclj._lib import lib
    bodies, hits, depth, nz, alb = KNOWN[name]
    sc = _scene(bodies)
    ds = _upload(sc)
    cam, p = _fixed_cam(), _params(8, 8, 4)
    got = {}
    try:
        for v in (0, 5, 12):
            ft = Feat(env, p, ds)
            try:
                sums, h, d = _with_variant(v, lambda: ft.add(cam, p).read())
                assert ft.samples == 4 and ft.counters() == [8 * 8 * 4] * 2
                f = ft.frame()
            finally:
                ft.free()
            got[v] = (sums, h, d)
            assert (h == hits).all()
            assert (sums[..., 0:3] == [4 * fix24(c) for c in alb]).all(), sums[0, 0]
            assert (sums[..., 3:5] == 0).all()
            if depth is None:
                # the near surface lies 5e-4 ahead, below t-min = 1e-3: the far root h + sqrt(disc), fp32
                ocz = np.float32(-1.0005)
                hh = np.float32(-1.0) * ocz
                cc = np.float32(np.float64(ocz) * np.float64(ocz) - 1.0)
                disc = np.float32(np.float64(hh) * np.float64(hh) - np.float64(cc))
                t = hh + np.sqrt(disc)
                assert hh - np.sqrt(disc) < np.float32(1e-3) < t
                ulps = np.abs(d.view(np.int32).astype(np.int64) - int(np.float32(t).view(np.int32)))
                print("far root: depth", d[0, 0], "formula", t, "ulps", ulps.max())
                assert ulps.max() <= 4
                assert (np.abs(sums[..., 5] - 4 * ONE) <= 4 * 16).all()     # z = +1 to 2^-20 per sample
                assert (np.abs(f[..., 5] - 1.0) <= 2.0 ** -20).all()
            else:
                assert (d.view(np.uint32) == np.float32(depth).view(np.uint32)).all()
                assert (sums[..., 5] == 4 * ONE * nz).all()
                assert (f[..., 3:6] == (0, 0, nz)).all() and (f[..., 7] == hits / 4).all()
                assert np.array_equal(f[..., 0:3], np.broadcast_to(np.float32(alb), f[..., 0:3].shape))
        assert _same(got[0], got[5]) and _same(got[0], got[12])
    finally:
        lib.rt_scene_free(ds)


# ---- 2: the same rays as the path kernel -------------------------------------------------
W2, H2 = 64, 40


def _variant_scene(env, kind=None, albedo=None):
    from rtclj import raytracing as R
    k = env.sc.kind.copy() if kind is None else np.full(len(env.sc), kind, np.int32)
    m = env.sc.mat.copy()
    if albedo is not None:
        m[:, :3] = albedo
    return R.Scene(env.sc.sphere.copy(), k, m)


@pytest.fixture(scope="module")
def one_spp(env):
    """The eight 1-spp, max_depth = 1 frames of the reference scene (64 x 40,
    seed 9) per camera and flag set: black on a hit, the sky on a miss.  The
    reference camera sees no sky at all; the wide one does."""
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    out = {}
    for wide in (False, True):
        cam = _cam(W2, H2, wide)
        for flags in (0, RT_FLAG_REJECTION_SAMPLERS, RT_FLAG_REALM):
            out[wide, flags] = [_launch(env, cam, _params(W2, H2, 1, begin=k, flags=flags)) for k in range(8)]
    return out


@pytest.mark.parametrize("wide", [False, True], ids=["reference", "wide"])
@pytest.mark.parametrize("flag", ["default", "rejection", "realm"])
def test_hits_are_the_path_kernels_black_pixels(env, one_spp, flag, wide):
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    flags = {"default": 0, "rejection": RT_FLAG_REJECTION_SAMPLERS, "realm": RT_FLAG_REALM}[flag]
    black = sum((~fr.any(axis=-1)).astype(np.int64) for fr in one_spp[wide, flags])
    if wide:   # part hit, part sky, and edge pixels with both
        assert 0.05 < black.mean() / 8 < 0.95 and ((black > 0) & (black < 8)).any()
    p = _params(W2, H2, 8, flags=flags)
    ft = Feat(env, p)
    try:
        sums, hits, depth = ft.add(_cam(W2, H2, wide), p).read()
    finally:
        ft.free()
    assert np.array_equal(hits.astype(np.int64), black)
    assert np.array_equal(np.isinf(depth), hits == 0)


@pytest.mark.parametrize("wide", [False, True], ids=["reference", "wide"])
@pytest.mark.parametrize("flag", ["default", "rejection"])
def test_sky_and_albedo_sums_are_the_path_kernels(env, one_spp, flag, wide):
    from rtclj._lib import RT_FLAG_REJECTION_SAMPLERS, lib
    flags = RT_FLAG_REJECTION_SAMPLERS if flag == "rejection" else 0
    cam = _cam(W2, H2, wide)
    p = _params(W2, H2, 8, flags=flags)
    # (b) no material anywhere: a hit adds nothing, a miss the sky -- rt_launch's max_depth = 1 frame
    ds = _upload(_variant_scene(env, kind=3))
    try:
        ft = Feat(env, p, ds)
        try:
            f = ft.add(cam, p).frame()
        finally:
            ft.free()
        want = _launch(env, cam, p, ds)
        assert np.array_equal(f[..., 0:3].view(np.uint32), want.view(np.uint32))
        assert want.any() == wide
    finally:
        lib.rt_scene_free(ds)
    # (c) one lambertian albedo everywhere: hits * fix24(A) + the sky's sums, which the eight
    # 1-spp frames hold exactly (at 1 spp a channel is its integer sum times 2^-24)
    sky = np.zeros((H2, W2, 3), np.int64)
    for fr in one_spp[wide, flags]:
        s = fr.astype(np.float64) * ONE
        assert np.array_equal(s, np.round(s))
        sky += s.astype(np.int64)
    ds = _upload(_variant_scene(env, kind=0, albedo=A))
    try:
        ft = Feat(env, p, ds)
        try:
            sums, hits, _ = ft.add(cam, p).read()
        finally:
            ft.free()
    finally:
        lib.rt_scene_free(ds)
    want = hits.astype(np.int64)[..., None] * np.array([fix24(c) for c in A], np.int64) + sky
    assert np.array_equal(sums[..., 0:3], want)


# ---- 3: geometry, in float64 ---------------------------------------------------------------
W3, H3 = 64, 40
# the cover scene's own camera (rtclj.scenes.COVER_CAMERA), with and without its defocus: 3 % / 5 % of
# the pixels' footprints touch a silhouette, 14 % see the sky alone (from the geometry, no GPU)
GEO_CAMERA = dict(vfov=20.0, look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), focus_dist=10.0)
GEO_DEFOCUS = 0.6


def _v(c, name):
    return np.array(list(getattr(c, name)), np.float64)


def _geo_scene():
    from rtclj import raytracing as R
    from rtclj import scenes
    sc = scenes.cover(3)
    n = len(sc)
    mat = np.zeros((n, 4), np.float32)
    i = np.arange(n)
    mat[:, 0], mat[:, 1] = (i % 250 + 1) / 256.0, (i // 250 + 1) / 256.0
    return R.Scene(sc.sphere.copy(), np.zeros(n, np.int32), mat)


def _roots(O, D, sph):
    """float64 roots of the unit-direction rays (O, D) (..., 3) against every body: (..., n) near, far (NaN: none)."""
    oc = sph[:, :3] - O[..., None, :]
    h = np.einsum("...k,...nk->...n", D, oc)
    c = np.einsum("...nk,...nk->...n", oc, oc) - sph[:, 3] ** 2
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(h * h - c)
    return h - sq, h + sq


def _lens(cam, k):
    """Probe origins: the centre, and with defocus k points on the lens disk's rim and k at half its radius."""
    O = [_v(cam, "center")]
    if cam.defocus:
        for rad in (1.0, 0.5):
            for a in np.arange(k) * 2 * np.pi / k:
                O.append(O[0] + rad * (np.cos(a) * _v(cam, "disk_u") + np.sin(a) * _v(cam, "disk_v")))
    return np.array(O)


def _silhouette_classes(cam, sph):
    """Per pixel, from the geometry alone: the share of probe rays (5 x 5 over
    the footprint x the lens probes) that hit any body."""
    p00, du, dv = _v(cam, "p00"), _v(cam, "du"), _v(cam, "dv")
    off = np.linspace(-0.5, 0.5, 5)
    O = _lens(cam, 8)
    share = np.zeros((H3, W3))
    for y in range(H3):   # (a row at a time: the arrays stay small)
        fx = np.arange(W3)[:, None, None] + off[None, :, None]
        fy = y + off[None, None, :]
        S = p00 + fx[..., None] * du + fy[..., None] * dv                # (W, 5, 5, 3)
        D = S[..., None, :] - O                                           # (W, 5, 5, L, 3)
        ln = np.linalg.norm(D, axis=-1)
        near, far = _roots(np.broadcast_to(O, D.shape), D / ln[..., None], sph)
        tmin = 1e-3 * ln[..., None]
        hit = ((near > tmin) | (far > tmin)).any(axis=-1)
        share[y] = hit.reshape(W3, -1).mean(axis=-1)
    return share


@pytest.fixture(scope="module")
def geo(env):
    """The cover scene's 1-spp feature frames under both cameras (float64), traced once."""
    from rtclj import raytracing as R
    from rtclj._lib import lib
    sc = _geo_scene()
    p = _params(W3, H3, 1, seed=5)
    ds = _upload(sc)
    out = dict(sc=sc)
    try:
        for defocus in (0.0, GEO_DEFOCUS):
            cam = R.camera(W3, H3, defocus_angle=defocus, **GEO_CAMERA)
            ft = Feat(env, p, ds)
            try:
                out[defocus] = (cam, ft.add(cam, p).frame().astype(np.float64))
            finally:
                ft.free()
    finally:
        lib.rt_scene_free(ds)
    return out


def _named_body(f, y, x):
    ir, ig = f[y, x, 0] * 256 - 1, f[y, x, 1] * 256 - 1
    assert ir == int(ir) and ig == int(ig) and f[y, x, 2] == 0
    return int(ir) + 250 * int(ig)


@pytest.mark.parametrize("defocus", [0.0, GEO_DEFOCUS])
def test_normals_are_unit_length(geo, defocus):
    """| |n| - 1 | <= 2^-20 on every hit pixel, per radius class printed.

    The path kernel's own (P - C) * (1/r) at the fp32 root would miss this by
    far for small bodies (the root's h and c are rounded at |oc|^2's
    magnitude: | |n| - 1 | up to 1.1e-3 for the r = 0.2 bodies 13 units away,
    3.9e-5 for r = 1, measured); the feature pass therefore scales each
    sample's normal by one correctly rounded 1 / |n| (first_hit.h): what is
    left is that product's rounding and the 2^-24 truncation of the sums
    (measured: 1.4e-7 at the worst pixel of either camera)."""
    sph = geo["sc"].sphere.astype(np.float64)
    f = geo[defocus][1]
    hitm = f[..., 7] == 1.0
    dev = np.abs(np.linalg.norm(f[..., 3:6], axis=-1) - 1.0)
    body = np.array([[_named_body(f, y, x) if hitm[y, x] else -1 for x in range(W3)] for y in range(H3)])
    for r in sorted(set(np.abs(sph[:, 3]).tolist())):
        m = hitm & np.isin(body, np.nonzero(np.abs(sph[:, 3]) == r)[0])
        if m.any():
            print(f"|r| = {r:g}: {m.sum()} pixels, worst | |n| - 1 | = {dev[m].max():.3e}, "
                  f"{(dev[m] > 2.0 ** -20).sum()} beyond 2^-20")
    assert dev[hitm].max() <= 2.0 ** -20, (dev[hitm].max(), np.argwhere(hitm & (dev > 2.0 ** -20))[:5])


@pytest.mark.parametrize("defocus", [0.0, GEO_DEFOCUS])
def test_geometry_in_float64(geo, defocus):
    sc = geo["sc"]
    sph = sc.sphere.astype(np.float64)
    n = len(sc)
    cam, f = geo[defocus]
    center, p00, du, dv = (_v(cam, k) for k in ("center", "p00", "du", "dv"))
    # the camera and its lens lie outside every body: each first hit is a front face (n_out = n)
    assert (np.linalg.norm(sph[:, :3] - center, axis=1) - np.abs(sph[:, 3]) > 0.5).all()
    # the CPU side: which pixels' footprints touch a silhouette, from the geometry alone
    share = _silhouette_classes(cam, sph)
    mixed = (share > 0) & (share < 1)
    print("silhouette pixels:", mixed.mean())
    assert mixed.mean() <= 0.15
    hitm = f[..., 7] == 1.0
    assert ((f[..., 7] == 0.0) | hitm).all() and 0.2 < hitm.mean() < 0.98
    nrm = np.cross(du, dv)
    # lens candidates: a 41 x 41 grid over the disk (the centre alone without defocus)
    if cam.defocus:
        g = np.linspace(-1, 1, 41)
        ab = np.array([(a, b) for a in g for b in g if a * a + b * b <= 1.0])
        cand_O = center + ab[:, :1] * _v(cam, "disk_u") + ab[:, 1:] * _v(cam, "disk_v")
    else:
        cand_O = center[None, :]
    worst = dict(len=0.0, dist=0.0)
    for y, x in zip(*np.nonzero(hitm)):
        b = _named_body(f, y, x)
        assert 0 <= b < n
        Cb, r = sph[b, :3], sph[b, 3]
        nn, t = f[y, x, 3:6], f[y, x, 6]
        worst["len"] = max(worst["len"], abs(np.linalg.norm(nn) - 1))   # (asserted in test_normals_are_unit_length)
        P = Cb + r * nn
        D = P - cand_O
        dist = np.linalg.norm(D, axis=1)
        assert (D @ nn < 0).all(), (y, x)                                  # the face rule: turned against the ray
        lam = ((p00 - cand_O) @ nrm) / (D @ nrm)
        S = cand_O + lam[:, None] * D
        fx, fy = ((S - p00) @ du) / (du @ du), ((S - p00) @ dv) / (dv @ dv)
        foot = (np.abs(fx - x) <= 0.5 + 1e-3) & (np.abs(fy - y) <= 0.5 + 1e-3)
        bound = K_BOUND * (t + 3 * abs(r))
        ok = foot & (np.abs(dist - t) <= bound)
        assert ok.any(), (y, x, b, t, dist.min(), dist.max(), foot.any())
        worst["dist"] = max(worst["dist"], float(np.abs(dist - t)[foot].min() / bound))
        # no other body nearer on that ray, for one such origin at least
        idx = np.nonzero(ok)[0]
        idx = idx[np.linspace(0, len(idx) - 1, min(len(idx), 16)).astype(int)]
        near, far = _roots(cand_O[idx], D[idx] / dist[idx, None], sph)
        tmin = 1e-3 * (lam[idx] * dist[idx])[:, None]
        lim = t - K_BOUND * (t + 3 * np.abs(sph[:, 3]))
        occl = ((near > tmin) & (near < lim)) | ((far > tmin) & (far < lim))
        occl[:, b] = False
        assert (~occl.any(axis=1)).any(), (y, x, b)
    print("worst | |n| - 1 |:", worst["len"], " worst | |P - O| - t | / bound:", worst["dist"])
    # misses: a pixel every probe ray of which hits a body cannot be one; the pixels whose
    # footprint touches a silhouette are not asserted (their share is capped above)
    miss = ~hitm
    assert not (miss & (share == 1.0)).any(), np.argwhere(miss & (share == 1.0))[:5]
    assert not (hitm & (share == 0.0) & ~_dilate(share > 0)).any()


def _dilate(m):
    """m or any of its 8 neighbours."""
    out = m.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = np.zeros_like(m)
            ys = slice(max(dy, 0), m.shape[0] + min(dy, 0))
            yd = slice(max(-dy, 0), m.shape[0] + min(-dy, 0))
            xs = slice(max(dx, 0), m.shape[1] + min(dx, 0))
            xd = slice(max(-dx, 0), m.shape[1] + min(-dx, 0))
            sh[yd, xd] = m[ys, xs]
            out |= sh
    return out


# ---- 4: order-free ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(env):
    """The reference scene under the wide camera, 64 x 40, seed 9, 8 spp in one pass."""
    cam, p = _cam(W2, H2, True), _params(W2, H2, 8)
    ft = Feat(env, p)
    try:
        raw = ft.add(cam, p).read()
        assert ft.counters() == [W2 * H2 * 8] * 2 and ft.samples == 8
        f = ft.frame()
    finally:
        ft.free()
    assert 0 < raw[1].sum() < 8 * W2 * H2
    return dict(cam=cam, p=p, raw=raw, frame=f)


@pytest.mark.parametrize("order", ["3+5", "5+3 reversed", "two streams", "1 x 8"])
def test_passes_in_any_order(env, whole, order):
    torch = env.torch
    cam = whole["cam"]
    ft = Feat(env, whole["p"])
    try:
        if order == "3+5":
            ft.add(cam, _params(W2, H2, 3, begin=0)).add(cam, _params(W2, H2, 5, begin=3))
        elif order == "5+3 reversed":
            ft.add(cam, _params(W2, H2, 3, begin=5)).add(cam, _params(W2, H2, 5, begin=0))
        elif order == "two streams":
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            ft.add(cam, _params(W2, H2, 4, begin=0), stream=s1)
            ft.add(cam, _params(W2, H2, 4, begin=4), stream=s2)   # (both enqueued before either is waited for)
        else:
            for k in range(8):
                ft.add(cam, _params(W2, H2, 1, begin=7 - k))
        assert ft.samples == 8
        assert _same(ft.read(), whole["raw"])
        assert ft.counters() == [W2 * H2 * 8] * 2
        assert np.array_equal(ft.frame().view(np.uint32), whole["frame"].view(np.uint32))
    finally:
        ft.free()


def test_interleaved_shards(env, whole):
    from rtclj.shard import shard_rows
    seen = np.zeros(H2, bool)
    for first in range(4):
        p = _params(W2, H2, 8, row_tile=8, tile_first=first, tile_step=4)
        rows = shard_rows(H2, 8, first, 4)
        ft = Feat(env, p)
        try:
            raw = ft.add(whole["cam"], p).read()
            assert ft.counters() == [len(rows) * W2 * 8] * 2
        finally:
            ft.free()
        assert raw[1].shape == (len(rows), W2)
        assert _same(raw, tuple(a[rows] for a in whole["raw"])), first
        seen[rows] = True
    assert seen.all()


def test_sources_agree(env, whole):
    """The tree in LDS, the tree in global memory and the linear scan: identical arrays."""
    got = {}
    for v in (0, 5, 12):
        ft = Feat(env, whole["p"])
        try:
            got[v] = _with_variant(v, lambda: (_source(env.ds), ft.add(whole["cam"], whole["p"]).read()))
        finally:
            ft.free()
    assert [got[v][0] for v in (0, 5, 12)] == [0, 2, 1]
    for v in (0, 5, 12):
        assert _same(got[v][1], whole["raw"]), v


def test_cover_scene_sources_agree(env):
    """484 bodies, big bodies outside the tree, a deeper stack: the three sources again."""
    from rtclj import scenes
    cam, p = scenes.cover_camera(W2, H2), _params(W2, H2, 4)
    got = {}
    for v in (0, 5, 12):
        ft = Feat(env, p, env.ds_cover)
        try:
            got[v] = _with_variant(v, lambda: (_source(env.ds_cover), ft.add(cam, p).read()))
        finally:
            ft.free()
    assert [got[v][0] for v in (0, 5, 12)] == [0, 2, 1]
    assert _same(got[0][1], got[5][1]) and _same(got[0][1], got[12][1])
    assert 0 < got[0][1][1].sum() < 4 * W2 * H2


def test_partial_tiles(env):
    """13 x 11: a partial tile in both directions.  A pixel's RNG key holds the
    frame's width (j * width + i), so no 16 x 16 frame shares these rays: the
    three sources against each other, into NaN-filled buffers, and the rows
    against a row range of the same frame."""
    w, h = 13, 11
    cam, p = _cam(w, h, True), _params(w, h, 8)
    got = {}
    for v in (0, 5, 12):
        ft = Feat(env, p)
        try:
            raw = _with_variant(v, lambda: ft.add(cam, p).read())
            got[v] = raw + (ft.frame(),)
            assert ft.counters() == [w * h * 8] * 2
        finally:
            ft.free()
    assert _same(got[0], got[5]) and _same(got[0], got[12])
    assert 0 < got[0][1].sum() < 8 * w * h
    from rtclj._lib import rt_params
    q = rt_params(width=w, height=h, row_begin=3, row_end=10, spp=8, max_depth=1, seed=9)
    ft = Feat(env, q)
    try:
        assert _same(ft.add(cam, q).read(), tuple(a[3:10] for a in got[0][:3]))
    finally:
        ft.free()


# ---- 5: contract edges -----------------------------------------------------------------------------
def test_errors_leave_the_object_unchanged(env, whole):
    from rtclj._lib import fptr, i64ptr, lib, rt_params, u32ptr
    cam, p = whole["cam"], whole["p"]
    ft = Feat(env, p)
    sp = _sptr(env, None)

    def refused(rc):
        return rc == -1 and lib.rt_last_error() != b""
    try:
        ft.add(cam, p)
        for q in (_params(W2 + 1, H2, 2), _params(W2, H2 + 1, 2),
                  _params(W2, H2, 2, row_tile=4, tile_first=0, tile_step=2),
                  rt_params(width=W2, height=H2, row_begin=1, row_end=H2, spp=2, max_depth=1, seed=9),
                  _params(W2, H2, 2, flags=64), _params(W2, H2, -1)):
            assert refused(lib.rt_launch_feat(env.ds, C.byref(cam), C.byref(q), ft.h, None, sp))
            assert lib.rt_last_error().startswith(b"rt_launch_feat: ")
        if lib.rt_device_count() > 1:
            other = C.c_void_p()
            assert lib.rt_scene_upload(1, C.byref(env.sc.c), C.byref(other)) == 0
            assert refused(lib.rt_launch_feat(other, C.byref(cam), C.byref(p), ft.h, None, None))
            assert b"device" in lib.rt_last_error()
            lib.rt_scene_free(other)
        bad = C.c_void_p()
        assert refused(lib.rt_feat_create(env.ds, C.byref(_params(0, H2, 1)), C.byref(bad))) and not bad.value
        assert refused(lib.rt_feat_create(env.ds, C.byref(rt_params(width=4, height=4, row_begin=3, row_end=2)),
                                          C.byref(bad)))
        assert ft.samples == 8 and _same(ft.read(), whole["raw"])
        # the count's limit, 2^32 - 1, reached without rendering
        zs, zh = np.zeros((H2, W2, 6), np.int64), np.zeros((H2, W2), np.uint32)
        zd = np.full((H2, W2), np.inf, np.float32)
        assert lib.rt_feat_add(ft.h, i64ptr(zs), u32ptr(zh), fptr(zd), 2 ** 32 - 1 - 8 - 2, sp) == 0
        assert ft.samples == 2 ** 32 - 3
        assert refused(lib.rt_launch_feat(env.ds, C.byref(cam), C.byref(_params(W2, H2, 3)), ft.h, None, sp))
        assert b"2^32" in lib.rt_last_error()
        assert refused(lib.rt_feat_add(ft.h, i64ptr(zs), u32ptr(zh), fptr(zd), 3, sp))
        assert refused(lib.rt_feat_add(ft.h, i64ptr(zs), u32ptr(zh), fptr(np.zeros_like(zd)), 1, sp))
        assert ft.samples == 2 ** 32 - 3 and _same(ft.read(), whole["raw"])
        assert ft.counters() == [W2 * H2 * 8] * 2
        # ... and still usable
        assert lib.rt_launch_feat(env.ds, C.byref(cam), C.byref(_params(W2, H2, 2, begin=8)), ft.h, None, sp) == 0
        assert ft.samples == 2 ** 32 - 1
        ft.frame()
    finally:
        ft.free()


def test_clear_and_merge(env, whole):
    from rtclj._lib import check, fptr, i64ptr, lib, u32ptr
    cam = whole["cam"]
    a, b = Feat(env, whole["p"]), Feat(env, whole["p"])
    try:
        a.add(cam, _params(W2, H2, 3, begin=0))
        b.add(cam, _params(W2, H2, 5, begin=3))
        ra, rb = a.read(), b.read()
        check(lib.rt_feat_clear(a.h, _sptr(env, None)))
        assert a.samples == 0
        s, h, d = a.read()
        assert not s.any() and not h.any() and (d.view(np.uint32) == INF_BITS).all()
        f = a.frame()
        assert not f[..., :6].any() and np.isinf(f[..., 6]).all() and not f[..., 7].any()
        # two stripes merged through the host: sums and hits add, the depth is the minimum
        for r, n in ((rb, 5), (ra, 3)):
            check(lib.rt_feat_add(a.h, i64ptr(r[0]), u32ptr(r[1]), fptr(r[2]), n, _sptr(env, None)))
        assert a.samples == 8 and _same(a.read(), whole["raw"])
        assert np.array_equal(whole["raw"][2], np.minimum(ra[2], rb[2]))
    finally:
        a.free()
        b.free()


# ---- 6: hosts ---------------------------------------------------------------------------------------------
def test_python_features(env, whole):
    from rtclj import raytracing as R
    from rtclj._lib import fptr, i64ptr, lib, u32ptr
    torch = env.torch
    with R.Features(env.sc, whole["cam"], W2, H2, seed=9) as ft:
        assert ft.samples == 0 and ft.shape == (H2, W2, 8)
        assert ft.add(3) == 3 and ft.add(5) == 8
        raw = ft.raw()
        assert _same(raw, whole["raw"])
        f = ft.frame()
        host = np.full(f.shape, np.nan, np.float32)
        assert lib.rt_feat_resolve_host(i64ptr(raw[0]), u32ptr(raw[1]), fptr(raw[2]), raw[1].size, 8, fptr(host)) == 0
        assert np.array_equal(f.view(np.uint32), host.view(np.uint32))
        assert np.array_equal(f.view(np.uint32), whole["frame"].view(np.uint32))
        d = torch.full((H2 * W2 * 8,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ft.resolve_into(d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy().reshape(f.shape).view(np.uint32), f.view(np.uint32))
        ft.clear()
        assert ft.samples == 0 and not ft.raw()[1].any()
        assert ft.add_raw(*raw, 8) == 8 and _same(ft.raw(), whole["raw"])
        ft.clear()
        ft.add(8)
        assert _same(ft.raw(), whole["raw"])


def test_rt_main_features(gpu_lib, tmp_path):
    from rtclj import raytracing as R
    import pngdec
    assert RT_MAIN.exists(), "lib/rt_main is not built (make -C raytracing-clj_amd)"
    child = dict(os.environ)
    child.pop("RTCLJ_LIBRARY", None)
    r = subprocess.run([str(RT_MAIN), "4", "5", "--width", "64", "--gpus", "1", "--no-png", "--seed", "3",
                        "--features", "ft"], cwd=tmp_path, capture_output=True, text=True, timeout=120, env=child)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    w, h = 64, 36
    with R.Features(R.hittables, _cam(w, h), w, h, seed=3) as ft:
        ft.add(4)
        f = ft.frame()
    assert (tmp_path / "ft.feat.f32").read_bytes() == f.tobytes()
    alb, info = pngdec.decode((tmp_path / "ft.albedo.png").read_bytes())
    assert alb.shape == (h, w, 3) and np.array_equal(alb, R.write_color(np.ascontiguousarray(f[..., 0:3])))
    nrm, info = pngdec.decode((tmp_path / "ft.normal.png").read_bytes())
    v = np.clip(0.5 * f[..., 3:6].astype(np.float64) + 0.5, 0.0, 1.0)
    assert np.array_equal(nrm, np.floor(v * 255.0 + 0.5).astype(np.uint8))
    assert nrm.min() < 100 and nrm.max() > 156 and (nrm == 128).any()


# ---- the path kernel's launches are untouched (after the tests above) ---------------------------------
def test_occupancy_is_untouched_by_the_feature_launches(env):
    for name, ww, hh, spp in OCC_SHAPES:
        assert _occupancy(env.ds if name == "ref" else env.ds_cover, ww, hh, spp) == env.occ_before[name], name
    assert env.occ_before["ref"][3] == 22
