"""Specular-chain features on the host (include/rt.h: rt_feat_chain_host; no GPU
needed): presence and argument errors, the two properties rt.h states -- with no
bounce the chain is the first-hit pass bit for bit, on smooth bodies alone it is
the path the trace kernel follows under RT_FLAG_REALM -- an independent
restatement in NumPy (fp64, its primitives held to oracle.sphere_hit / reflect /
refract) with its negative controls, the Python hosts, the stand-alone sanitizer
program, and the denoiser's quality with chain guides against first-hit guides.
tests/test_gpu_chain.py holds the device to the records below.
"""
import ctypes as C
import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edge_scenes as E
import feat_oracle as FO
import oracle

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "chain_check"
F = np.float32
CHAIN_FUNCS = ("rt_launch_feat_chain", "rt_feat_chain_host", "rt_feat_chain_occupancy")
EDGE_NAMES = ("fuzz_0",) + tuple(f"eta_{k}" for k in E.ETAS) + ("ties_big", "camera_inside_glass",
                                                                 "bubble_negative_radius", "nonfinite_65")


# ---- scenes -----------------------------------------------------------------------------
def _scene(rows):
    from rtclj import raytracing as R
    a = np.array([r[:4] for r in rows], np.float32)
    k = np.array([r[4] for r in rows], np.int32)
    m = np.array([r[5:9] for r in rows], np.float32)
    return R.Scene(a, k, m)


@functools.lru_cache(maxsize=None)
def mixed_scene():
    """12 bodies: a lambertian ground, a hollow glass ball (negative-radius
    bubble), fuzz-0 and fuzz-0.3 metal, lambertian, RT_NONE."""
    L, M, G, N = E.LAMB, E.METAL, E.GLASS, E.NONE
    return _scene([
        (0.0, -100.5, -1.0, 100.0, L, 0.8, 0.8, 0.0, 0.0),
        (-1.0, 0.0, -1.0, 0.5, G, 0.0, 0.0, 0.0, 1.5),
        (-1.0, 0.0, -1.0, -0.4, G, 0.0, 0.0, 0.0, 1.5),
        (1.0, 0.0, -1.0, 0.5, M, 0.8, 0.6, 0.2, 0.0),
        (0.0, 0.0, -1.2, 0.5, M, 0.7, 0.7, 0.9, 0.3),
        (0.0, -0.3, 0.0, 0.2, L, 0.1, 0.2, 0.5, 0.0),
        (-0.6, -0.35, -0.1, 0.15, N, 0.0, 0.0, 0.0, 0.0),
        (0.5, -0.3, -0.2, 0.2, M, 0.9, 0.9, 0.9, 0.0),
        (-0.2, -0.35, 0.4, 0.15, G, 0.0, 0.0, 0.0, 1.5),
        (0.9, -0.38, 0.3, 0.12, L, 0.9, 0.1, 0.1, 0.0),
        (-1.5, -0.3, 0.2, 0.2, M, 0.5, 0.9, 0.5, 0.5),
        (0.1, 0.9, -1.0, 0.3, L, 0.3, 0.8, 0.3, 0.0),
    ])


@functools.lru_cache(maxsize=None)
def smooth_scene():
    """Smooth bodies only: a fuzz-0 metal ground of r = 100, a glass ball, a
    hollow glass ball (negative-radius bubble), two fuzz-0 metal spheres."""
    M, G = E.METAL, E.GLASS
    return _scene([
        (0.0, -100.5, -1.0, 100.0, M, 0.8, 0.8, 0.8, 0.0),
        (-1.0, 0.0, -1.0, 0.5, G, 0.0, 0.0, 0.0, 1.5),
        (0.0, 0.0, -1.2, 0.5, G, 0.0, 0.0, 0.0, 1.5),
        (0.0, 0.0, -1.2, -0.4, G, 0.0, 0.0, 0.0, 1.5),
        (1.0, 0.0, -1.0, 0.5, M, 0.8, 0.6, 0.2, 0.0),
        (0.2, -0.3, 0.0, 0.2, M, 0.9, 0.5, 0.5, 0.0),
    ])


@functools.lru_cache(maxsize=None)
def closed_mirror():
    """The camera inside a closed fuzz-0 sphere."""
    from rtclj import raytracing as R
    sc = _scene([(0.0, 0.0, 0.0, 5.0, E.METAL, 0.9, 0.8, 0.7, 0.0)])
    cam = R.camera(8, 8, vfov=40.0, look_from=(0.5, 0.3, 1.0), look_at=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0),
                   defocus_angle=2.0, focus_dist=2.0)
    return sc, cam


def reference_scene():
    from rtclj import raytracing as R
    return R.Scene.from_bodies(R.hittables)


def ref_camera(w, h):
    from rtclj import raytracing as R
    return R.camera(w, h, **R.REFERENCE_CAMERA)


# ---- records -> what rt_feat_read returns -------------------------------------------------
def fix24s(c):
    """fix24's signed twin: c * 2^24 toward zero as int64, NaN gives 0."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(c, np.float32) * np.float32(FO.ONE)
        return np.where(np.isnan(v), 0, np.trunc(v)).astype(np.int64)


def records_sum(rec):
    """rt_feat_chain_host's records (rows, width, spp) summed as a pass sums
    them -> dict(sums int64, hits uint32, depth float32)."""
    hit = rec["body"] >= 0
    sums = np.zeros(rec.shape[:2] + (6,), np.int64)
    sums[..., 0:3] = FO.fix24(rec["albedo"]).sum(axis=2).astype(np.uint64).view(np.int64)
    sums[..., 3:6] = np.where(hit[..., None], fix24s(rec["normal"]), 0).sum(axis=2)
    depth = np.where(hit, rec["length"], np.float32(np.inf)).min(axis=2).astype(np.float32)
    return dict(sums=sums, hits=hit.sum(axis=2).astype(np.uint32), depth=depth)


def host(sc, rays, **opts):
    from rtclj import raytracing as R
    return R.feat_chain_host(sc, rays, **opts)


def same_raw(a, b):
    return (np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["hits"], b["hits"]) and
            np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32)))


# ---- 1. presence, signatures, argument errors ------------------------------------------------
@pytest.mark.parametrize("which", ["product", "diag"])
def test_symbols_and_signatures(which):
    import rtclj
    from rtclj import _lib
    dll = C.CDLL(str(rtclj.library_path if which == "product" else _lib.diag_library_path))
    hdr = (ROOT / "include" / "rt.h").read_text()
    for name in CHAIN_FUNCS:
        assert hasattr(dll, name), name
        assert name in _lib.SIGNATURES and name in _lib.ADDITIVE
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    assert re.search(r"typedef struct rt_feat_chain_opts\s*\{\s*int max_bounces;[^}]*float fuzz_max;", hdr)
    assert re.search(r"typedef struct rt_chain_sample\s*\{\s*int32_t body, bounces;\s*float length, albedo\[3\], normal\[3\];",
                     hdr)
    assert C.sizeof(_lib.rt_feat_chain_opts) == 8 and C.sizeof(_lib.rt_chain_sample) == 36
    assert np.dtype(_lib.CHAIN_SAMPLE_DTYPE).itemsize == 36
    assert len(_lib.SIGNATURES["rt_launch_feat_chain"][1]) == 7 and len(_lib.SIGNATURES["rt_feat_chain_host"][1]) == 5
    assert _lib.CHAIN_DEFAULTS == dict(max_bounces=8, fuzz_max=0.0)
    # what a user must know stands in the header
    for word in ("VIRTUAL distance", "not mirrored", "refraction branch only", "fuzz above fuzz_max is rough",
                 "never be given to rt_temporal_step"):
        assert word in hdr, word


def test_argument_errors():
    from rtclj import RTError
    from rtclj import raytracing as R
    from rtclj._lib import fptr, lib, rt_chain_sample, rt_feat_chain_opts
    sc = reference_scene()
    rays = np.array([[0, 0, 1, 0, 0, -1]], np.float32)
    out = (rt_chain_sample * 1)()
    assert lib.rt_feat_chain_host(C.byref(sc.c), None, fptr(rays), 1, out) == 0
    assert (out[0].body, out[0].bounces) == (1, 0)
    for bad in ((-1, 0.0), (65, 0.0), (8, -0.5), (8, float("nan")), (8, float("inf"))):
        o = rt_feat_chain_opts(*bad)
        assert lib.rt_feat_chain_host(C.byref(sc.c), C.byref(o), fptr(rays), 1, out) == -1, bad
        assert b"max_bounces" in lib.rt_last_error() or b"fuzz_max" in lib.rt_last_error()
    for o in ((0, 0.0), (64, 3e38)):
        assert lib.rt_feat_chain_host(C.byref(sc.c), C.byref(rt_feat_chain_opts(*o)), fptr(rays), 1, out) == 0
    assert lib.rt_feat_chain_host(None, None, fptr(rays), 1, out) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_feat_chain_host(C.byref(sc.c), None, None, 1, out) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_feat_chain_host(C.byref(sc.c), None, fptr(rays), 1, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_feat_chain_host(C.byref(sc.c), None, None, 0, None) == 0   # n = 0
    bad_kind = R.Scene(sc.sphere, np.full(len(sc), 7, np.int32), sc.mat)
    assert lib.rt_feat_chain_host(C.byref(bad_kind.c), None, fptr(rays), 1, out) == -2   # RT_E_MATERIAL
    assert b"material kind" in lib.rt_last_error()
    # the device entries refuse NULL handles before any device call
    assert lib.rt_launch_feat_chain(None, None, None, None, None, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_feat_chain_occupancy(None, None) == -1 and b"NULL" in lib.rt_last_error()
    with pytest.raises(TypeError):
        R.feat_chain_host(sc, rays, bounces=3)
    with pytest.raises(ValueError):
        R.feat_chain_host(sc, rays[:, :5])
    with pytest.raises(RTError):
        R.feat_chain_host(sc, rays, max_bounces=65)
    assert R.feat_chain_host(sc, np.zeros((0, 6), np.float32)).shape == (0,)


# ---- 2. property 1: no bounce is the first-hit pass ----------------------------------------
def _detail_cases():
    from rtclj import scenes
    yield "reference", reference_scene, lambda: ref_camera(E.W, E.H), 4, 5
    yield "cover_2", lambda: scenes.cover(2), lambda: scenes.cover_camera(E.W, E.H), 4, 6
    for name in EDGE_NAMES:
        yield name, None, None, None, None


@functools.lru_cache(maxsize=None)
def detail(name):
    """(scene, camera, the feature mirror with body, t and rays, spp, seed, sample_begin) of a property-1 case, 64 x 36."""
    for n, mk_sc, mk_cam, spp, seed in _detail_cases():
        if n != name:
            continue
        if mk_sc is None:
            sc, cam, meta = E.case(name)
            p = E.params(meta)
            return sc, cam, FO.edge_mirror(name, detail=True), E.SPP, p["seed"], p["sample_begin"]
        sc, cam = mk_sc(), mk_cam()
        return sc, cam, FO.mirror(sc, cam, E.W, E.H, spp, seed, want_rays=True, want_body=True, want_t=True), spp, seed, 0
    raise KeyError(name)


PROPERTY1_NAMES = ("reference", "cover_2") + EDGE_NAMES


@pytest.mark.parametrize("name", PROPERTY1_NAMES)
def test_no_bounce_is_the_first_hit_pass(name):
    sc, _, m, spp, _, _ = detail(name)
    rec = host(sc, m["rays"], max_bounces=0)
    assert rec.shape == (E.H, E.W, spp)
    assert np.array_equal(rec["body"], m["body"])
    assert (rec["bounces"] == 0).all()
    with np.errstate(over="ignore"):
        assert np.array_equal(rec["length"].view(np.uint32), m["t"].astype(np.float32).view(np.uint32))
    assert same_raw(records_sum(rec), m)


@pytest.mark.parametrize("name", ("ties_big", "nonfinite_65"))
def test_any_bounces_on_rough_bodies_only(name):
    """A scene whose smooth bodies are made lambertian: max_bounces changes nothing."""
    from rtclj import raytracing as R
    sc, _, m, _, _, _ = detail(name)
    kind = np.where((sc.kind == E.GLASS) | (sc.kind == E.METAL), E.LAMB, sc.kind).astype(np.int32)
    rough = R.Scene(sc.sphere, kind, sc.mat)
    a, b = host(rough, m["rays"], max_bounces=0), host(rough, m["rays"], max_bounces=8, fuzz_max=10.0)
    assert a.tobytes() == b.tobytes()


# ---- 3. property 2: on smooth bodies the chain is the realm path ----------------------------
P2_W, P2_H, P2_BOUNCES, P2_SEED = 32, 18, 8, 3


@functools.lru_cache(maxsize=None)
def property2():
    """The smooth scene's camera, rays (one a pixel), the host's records and the
    pixels whose chain ends in the sky."""
    sc, cam = smooth_scene(), ref_camera(P2_W, P2_H)
    m = FO.mirror(sc, cam, P2_W, P2_H, 1, P2_SEED, want_rays=True)
    rec = host(sc, m["rays"], max_bounces=P2_BOUNCES)
    return sc, cam, rec, (rec["body"] < 0)[..., 0]


def chain_albedo_frame(rec, samples):
    raw = records_sum(rec)
    return FO.resolve_np(raw["sums"], raw["hits"], raw["depth"], samples)[..., 0:3]


def test_smooth_bodies_give_the_realm_path():
    sc, cam, rec, sky = property2()
    share = float(sky.mean())
    print(f"pixels whose chain ends in the sky: {share:.3f}")
    assert share >= 0.5, share
    img = oracle.render(oracle.MODE_REALM32 | oracle.DIRECT, *FO.scene_args(sc, cam), P2_W, P2_H, 1, P2_BOUNCES + 2,
                        seed=P2_SEED, nthreads=E.NT)[0]
    got = chain_albedo_frame(rec, 1)
    assert rec["bounces"][sky].max() >= 3      # chains through the glass among them
    assert np.array_equal(got[sky].view(np.uint32), img[sky].view(np.uint32)), \
        f"{int((got[sky] != img[sky]).any(axis=-1).sum())} of {int(sky.sum())} pixels differ"


# ---- 4. an independent restatement in double ----------------------------------------------------
def reflect_np(v, n):
    return v - 2.0 * (v * n).sum(-1, keepdims=True) * n


def refract_np(u, n, eta):
    c = np.minimum(-(u * n).sum(-1, keepdims=True), 1.0)
    perp = (u + n * c) * eta
    return perp - n * np.sqrt(np.abs(1.0 - (perp * perp).sum(-1, keepdims=True)))


def chain_np(sc, rays, max_bounces=8, fuzz_max=0.0, dtype=np.float64, guard=True, metal_unit=False):
    """rt.h's chain restated over arrays of rays: the reference's sphere test
    (hittable.clj:9-31) on the unit direction, reflect and refract as the oracle
    has them.  guard=False: the body a ray leaves is tested like any other.
    metal_unit: the metal reflects the unit direction (the same direction)."""
    T = dtype
    sph, mat, kind = sc.sphere.astype(T), sc.mat.astype(T), sc.kind
    flat = np.asarray(rays, np.float32).reshape(-1, 6).astype(T)
    n = len(flat)
    o, d = flat[:, :3].copy(), flat[:, 3:].copy()
    thr, L = np.ones((n, 3), T), np.zeros(n, T)
    last, b = np.full(n, -1), np.zeros(n, np.int32)
    out = np.zeros(n, [("body", "i4"), ("bounces", "i4"), ("length", "f8"), ("albedo", "f8", (3,)), ("normal", "f8", (3,))])
    act = np.arange(n)
    ids = np.arange(len(kind))
    with np.errstate(all="ignore"):
        while len(act):
            oo, dd = o[act], d[act]
            ln = np.sqrt((dd * dd).sum(-1))
            u = dd / ln[:, None]
            tmin = T(1e-3) * ln
            oc = sph[None, :, :3] - oo[:, None, :]
            h = (u[:, None, :] * oc).sum(-1)
            cc = (oc * oc).sum(-1) - sph[None, :, 3] ** 2
            disc = h * h - cc
            sq = np.sqrt(disc)
            if guard:
                sq = np.where(ids[None, :] == last[act][:, None], np.abs(h), sq)
            t = h - sq
            t = np.where(t > tmin[:, None], t, h + sq)
            t = np.where((t > tmin[:, None]) & np.isfinite(t), t, np.inf)
            body = t.argmin(axis=1)            # the first of equal roots: array order
            tb = t[np.arange(len(act)), body]
            miss = ~np.isfinite(tb)
            # the sky
            sa = 0.5 * (u[:, 1] + 1.0)
            sky = (1.0 - sa)[:, None] + sa[:, None] * np.array([0.5, 0.7, 1.0], T)
            # the hit record
            P = oo + u * tb[:, None]
            nrm = (P - sph[body, :3]) / sph[body, 3:4]
            front = (dd * nrm).sum(-1) < 0
            nrm = np.where(front[:, None], nrm, -nrm)
            k, m = kind[body], mat[body]
            smooth = (k == E.GLASS) | ((k == E.METAL) & (m[:, 3] <= fuzz_max))
            go = ~miss & smooth & (b[act] < max_bounces)
            rdir = reflect_np(u * ln[:, None] if not metal_unit else u, nrm)
            metal_on = (rdir * nrm).sum(-1) > 0
            ri = np.where(front, 1.0 / m[:, 3], m[:, 3])
            cosv = np.minimum(-(u * nrm).sum(-1), 1.0)
            tir = ~(ri * np.sqrt(1.0 - cosv * cosv) <= 1.0)
            gdir = np.where(tir[:, None], reflect_np(u, nrm), refract_np(u, nrm, ri[:, None]))
            is_metal = k == E.METAL
            go &= ~is_metal | metal_on
            Lnew = L[act] + tb
            # the chains that end here
            end = ~go
            e = act[end]
            att = np.where((k == E.GLASS)[:, None], 1.0, np.where((k == E.NONE)[:, None], 0.0, m[:, :3]))
            out["body"][e] = np.where(miss, -1, body)[end]
            out["bounces"][e] = b[act][end]
            out["length"][e] = np.where(miss, np.inf, Lnew)[end]
            out["albedo"][e] = (thr[act] * np.where(miss[:, None], sky, att))[end]
            nlen = np.sqrt((nrm * nrm).sum(-1, keepdims=True))
            out["normal"][e] = np.where(miss[:, None], 0.0, nrm / nlen)[end]
            # the chains that go on
            g = act[go]
            thr[g] = (thr[act] * np.where(is_metal[:, None], m[:, :3], 1.0))[go]
            d[g] = np.where(is_metal[:, None], rdir, gdir)[go]
            o[g] = P[go]
            L[g] = Lnew[go]
            last[g] = body[go]
            b[g] += 1
            act = g
    return out.reshape(np.asarray(rays).shape[:-1])


def test_the_restatements_primitives_are_the_oracles():
    rng = np.random.default_rng(5)
    for _ in range(40):
        v, n = rng.normal(size=3), rng.normal(size=3)
        n /= np.linalg.norm(n)
        u = v / np.linalg.norm(v)
        assert np.allclose(reflect_np(v, n), oracle.reflect(v, n), rtol=0, atol=1e-14)
        eta = float(rng.choice([1.5, 1 / 1.5]))
        assert np.allclose(refract_np(u, n, eta), oracle.refract(u, n, eta), rtol=0, atol=1e-14)
    # the sphere test: the first segment of camera rays against oracle.sphere_hit on the body found
    sc = reference_scene()
    rays = FO.mirror(sc, ref_camera(16, 9), 16, 9, 1, 2, want_rays=True)["rays"].reshape(-1, 6)
    rec = chain_np(sc, rays, max_bounces=0)
    for r, c in zip(rays, rec):
        if c["body"] < 0:
            assert not any(oracle.sphere_hit(s, r[:3], r[3:], 1e-3, np.inf)["hit"] for s in sc.sphere.astype(np.float64))
            continue
        hit = oracle.sphere_hit(sc.sphere[c["body"]].astype(np.float64), r[:3], r[3:], 1e-3, np.inf)
        assert hit["hit"] and abs(hit["t"] * np.linalg.norm(r[3:].astype(np.float64)) - c["length"]) < 1e-12
        assert np.allclose(hit["n"], c["normal"], rtol=0, atol=1e-12)


def compare(rec, ref):
    """(share of samples whose body or bounce count differ, then the largest
    deviation of L (relative), albedo and normal (absolute) over the others)."""
    same = (rec["body"] == ref["body"]) & (rec["bounces"] == ref["bounces"])
    hit = same & (rec["body"] >= 0)
    with np.errstate(invalid="ignore"):
        dl = np.abs(rec["length"][hit].astype(np.float64) - ref["length"][hit]) / ref["length"][hit]
    da = np.abs(rec["albedo"][same].astype(np.float64) - ref["albedo"][same])
    dn = np.abs(rec["normal"][same].astype(np.float64) - ref["normal"][same])
    return 1.0 - float(same.mean()), float(dl.max(initial=0)), float(da.max(initial=0)), float(dn.max(initial=0))


@functools.lru_cache(maxsize=None)
def fp64_case(which):
    from rtclj import scenes
    w, h, spp = 80, 45, 2
    if which == "reference":
        sc, cam = reference_scene(), ref_camera(w, h)
    else:
        sc, cam = scenes.cover(3), scenes.cover_camera(w, h)
    rays = FO.mirror(sc, cam, w, h, spp, 4, want_rays=True)["rays"]
    return sc, rays, host(sc, rays)


# the largest deviations measured (L relative, albedo, normal; see the docstring
# below): the test holds the host to four times these
MEASURED = {"reference": (1.596e-4, 1.385e-6, 1.608e-4), "cover_3": (3.527e-3, 2.061e-4, 6.425e-3)}


@pytest.mark.parametrize("which", ("reference", "cover_3"))
def test_against_the_fp64_restatement(which):
    """80 x 45, 2 spp, max_bounces 8.  Measured (share of samples whose final
    body or bounce count differ; largest deviations on the others):
      reference scene  0 of 7200 differ; L 1.596e-4 (relative), albedo 1.385e-6, normal 1.608e-4
      cover grid 3     0 of 7200 differ; L 3.527e-3 (relative), albedo 2.061e-4, normal 6.425e-3
    (the largest ones belong to grazing hits on the r = 0.2 bodies and to chains
    through two glass surfaces, where the fp32 root's error is bent twice).
    The deviations are bounded in principle by bvh_pad.h's 6e-4 (t + 3 r) per
    segment; the bounds asserted are four times the measured ones."""
    sc, rays, rec = fp64_case(which)
    ref = chain_np(sc, rays)
    share, dl, da, dn = compare(rec, ref)
    print(f"{which}: differing {share:.5f}, L rel {dl:.3e}, albedo {da:.3e}, normal {dn:.3e}; "
          f"bounces up to {int(rec['bounces'].max())}")
    if which == "reference":
        assert rec["bounces"].max() >= 4      # through the hollow glass: four surfaces
    assert share < 0.0025, share
    tl, ta, tn = (4 * v for v in MEASURED[which])
    assert dl <= tl and da <= ta and dn <= tn, (dl, da, dn)


# ---- 5. negative controls ---------------------------------------------------------------------
def test_negative_controls():
    """The restatement with the metal reflecting the unit direction u instead
    of d still agrees (the direction is the same): 0 of 7200 samples differ on
    the reference scene, 2 of 7200 on the smooth scene.
    The restatement without the self-hit guard does NOT leave the 1 % cap on the
    hollow-glass (reference) scene, in double or in float32: 0 of 7200 differ.
    There the body a ray leaves has |oc|^2 - r^2 = 0 within 1e-7, the stray root
    lies at 1e-7 / (2 h), far below t-min, and the ordinary test drops it as the
    guard does; in double that holds for every scene.  The guard earns its keep
    on a large smooth body in fp32: with the smooth scene's mirror ground at
    r = 10^4 (|oc|^2 - r^2 is 10^8's rounding error, about 8) the float32
    restatement differs from the host on 0.14 % of the samples with the guard
    and on 3.7 % without it.  That scene and precision are asserted here."""
    from rtclj import raytracing as R
    sc, rays, rec = fp64_case("reference")
    share_u = compare(rec, chain_np(sc, rays, metal_unit=True))[0]
    share_ng = max(compare(rec, chain_np(sc, rays, guard=False, dtype=t))[0] for t in (np.float64, np.float32))
    print(f"reference scene: metal reflecting u {share_u:.5f}, without the guard {share_ng:.5f}")
    assert share_u < 0.0025
    s = smooth_scene()
    rays_s = FO.mirror(s, ref_camera(80, 45), 80, 45, 2, 4, want_rays=True)["rays"]
    share_us = compare(host(s, rays_s), chain_np(s, rays_s, metal_unit=True))[0]
    print(f"smooth scene: metal reflecting u {share_us:.5f}")
    assert share_us < 0.0025
    sph = s.sphere.copy()
    sph[0] = (0.0, -1e4 - 0.5, -1.0, 1e4)
    big = R.Scene(sph, s.kind, s.mat)
    rays_b = FO.mirror(big, ref_camera(80, 45), 80, 45, 2, 4, want_rays=True)["rays"]
    rec_b = host(big, rays_b)
    with_guard = compare(rec_b, chain_np(big, rays_b, dtype=np.float32))[0]
    without = compare(rec_b, chain_np(big, rays_b, dtype=np.float32, guard=False))[0]
    print(f"mirror ground of r = 1e4, float32 restatement: with the guard {with_guard:.5f}, without {without:.5f}")
    assert with_guard < 0.0025 and without > 0.01, (with_guard, without)


# ---- 6. the Python hosts, the sanitizer program ----------------------------------------------------
def test_python_hosts_expose_the_chain():
    import inspect
    from rtclj import raytracing as R
    assert "feat_chain_host" in R.__all__ and hasattr(R, "feat_chain_host")
    for fn in (R.Features.__init__, R.render_denoised, R.render_upscaled, R.render_animation):
        par = inspect.signature(fn).parameters
        assert "chain" in par and par["chain"].default is None, fn
    o = R._chain_opts(5)
    assert (o.max_bounces, o.fuzz_max) == (5, 0.0)
    o = R._chain_opts(True)
    assert (o.max_bounces, o.fuzz_max) == (8, 0.0)
    o = R._chain_opts(dict(fuzz_max=0.5))
    assert (o.max_bounces, o.fuzz_max) == (8, 0.5)
    assert R._chain_opts(None) is None and R._chain_opts(False) is None
    with pytest.raises(TypeError):
        R._chain_opts(dict(bounces=2))
    main = (ROOT / "raytracing-clj_amd" / "csrc" / "rt_main.cpp").read_text()
    assert "--chain" in main and "rt_launch_feat_chain" in main


def test_sanitizer_program():
    """tools/chain_check.cpp: spec_chain.h's host pass under ASan and UBSan over
    hostile rays, bodies and materials, and the closed mirror at 64 bounces."""
    assert TOOL.exists(), f"{TOOL} is missing: make -C raytracing-clj_amd"
    run = subprocess.run([str(TOOL)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    rep = json.loads(run.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["bad_status"] == 0 and rep["bad_record"] == 0 and rep["closed_bad"] == 0
    assert rep["closed_max_bounces"] == 64 and rep["bad_args"] == 0 and rep["records"] > 10000
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_closed_mirror_returns_after_64_bounces():
    sc, cam = closed_mirror()
    rays = FO.mirror(sc, cam, 8, 8, 4, 1, want_rays=True)["rays"]
    rec = host(sc, rays, max_bounces=64)
    assert (rec["body"] == 0).all() and (rec["bounces"] == 64).all() and np.isfinite(rec["length"]).all()


# ---- 7. quality: the denoiser guided by chain features against first-hit features ------------------
QW, QH, Q_HALF, Q_FEAT_SPP, Q_REF_SPP, Q_REF_SEED = 160, 90, 4, 16, 1024, 77
Q_ALTERNATIVES = (("defaults", {}), ("normal_pow2=2", dict(normal_pow2=2)), ("normal_pow2=8", dict(normal_pow2=8)),
                  ("sigma_z=0.01", dict(sigma_z=0.01)), ("sigma_z=0.2", dict(sigma_z=0.2)))


class OracleFrames:
    """The frames from the oracle alone: the path kernel's fp32 mirror, the
    feature mirror, and rt_feat_chain_host over the feature mirror's rays."""

    def render(self, sc, cam, spp, seed, begin=0):
        return oracle.render(oracle.MODE_MIRROR32 | oracle.DIRECT, *FO.scene_args(sc, cam), QW, QH, spp, 50, seed=seed,
                             sample_begin=begin, nthreads=E.NT)[0]

    def features(self, sc, cam, spp, seed, chain):
        m = FO.mirror(sc, cam, QW, QH, spp, seed, want_rays=chain)
        if chain:
            m = records_sum(host(sc, m["rays"]))
        return FO.resolve_np(m["sums"], m["hits"], m["depth"], spp)


def quality_scene(which):
    from rtclj import raytracing as R
    from rtclj import scenes
    if which == "cover_3":
        return scenes.cover(3), R.camera(QW, QH, **scenes.COVER_CAMERA)
    return reference_scene(), ref_camera(QW, QH)


def quality_table(which, source):
    """Per seed 1-3 and option set of the chain-guided filter: (RMSE over M,
    RMSE over the frame), each divided by the first-hit-guided filter's at its
    defaults.  M: the pixels whose body (rt_ids_host) is glass or fuzz-0 metal."""
    from rtclj import raytracing as R
    sc, cam = quality_scene(which)
    ref = source.render(sc, cam, Q_REF_SPP, Q_REF_SEED).astype(np.float64)
    ids = R.ids_host(sc, cam, QW, QH)
    smooth = (sc.kind == E.GLASS) | ((sc.kind == E.METAL) & (sc.mat[:, 3] <= 0))
    M = (ids >= 0) & smooth[np.clip(ids, 0, None)]
    assert 0.05 < M.mean() < 0.5

    def rmse(img, mask=None):
        d = ((img.astype(np.float64) - ref) ** 2).mean(axis=-1)
        return float(np.sqrt(d[mask].mean() if mask is not None else d.mean()))

    table = {}
    for seed in (1, 2, 3):
        h0 = source.render(sc, cam, Q_HALF, seed)
        h1 = source.render(sc, cam, Q_HALF, seed, begin=Q_HALF)
        first = R.denoise_host(h0, h1, source.features(sc, cam, Q_FEAT_SPP, seed, False))
        chained = source.features(sc, cam, Q_FEAT_SPP, seed, True)
        for tag, o in Q_ALTERNATIVES:
            out = R.denoise_host(h0, h1, chained, **o)
            assert np.isfinite(out).all()
            table[seed, tag] = (rmse(out, M) / rmse(first, M), rmse(out) / rmse(first))
    return table


def check_quality(which, table):
    """Measured, CPU and device alike (RMSE with chain guides / RMSE with
    first-hit guides; over M, over the frame; seeds 1, 2, 3):
      cover grid 3, defaults       M 1.082 1.068 1.002   frame 0.983 0.971 0.961
      cover grid 3, normal_pow2=2  M 1.054 0.999 0.933   frame 0.939 0.915 0.902
      reference,    defaults       M 2.297 2.321 2.507   frame 1.704 1.731 1.799
      reference,    normal_pow2=8  M 1.682 1.725 1.710   frame 1.374 1.372 1.370
    At 4 + 4 samples a pixel the ratio over M is NOT below 1 on either scene, so
    nothing is asserted over M: what the first-hit guides smear across a mirror
    or a glass ball is mostly noise at this sample count, and an RMSE rewards
    the smear.  On the reference scene the chain's albedo is the larger loss:
    the ground seen through the glass has a blue albedo of 0, while the glass's
    own Schlick reflection of the sky, which the chain does not follow, is blue.
    Over the frame the cover scene measures below 1 (mean 0.972) and is held
    below 1.05; the reference scene measures above 1 and is printed only.
    `chain=` therefore stays off by default in every host."""
    for tag, _ in Q_ALTERNATIVES:
        print(which, tag, "M", ["%.3f" % table[s, tag][0] for s in (1, 2, 3)],
              "frame", ["%.3f" % table[s, tag][1] for s in (1, 2, 3)])
    if which == "cover_3":
        assert all(table[s, "defaults"][1] < 1.05 for s in (1, 2, 3))


@pytest.mark.parametrize("which", ("cover_3", "reference"))
def test_quality(which):
    check_quality(which, quality_table(which, OracleFrames()))
