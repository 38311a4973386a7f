"""rt_feat against the oracle's same-ray mirror (oracle.features,
MODE_MIRROR32): rt_feat_read's sums, hit counts and depth bits equal the
mirror's bit for bit -- on the reference scene, on the geo scene of
tests/test_gpu_feat.py and on every edge input of tests/edge_scenes.py, with
the bodies read from the tree in LDS, from the tree in global memory and by
the linear scan -- and rt_feat_resolve equals a NumPy restatement of the
resolve.  The mirror itself is held to known answers, to the path mirror and
to fp64 on the CPU (tests/test_oracle_features.py).

What the earlier feature tests could not see shows here: a wrong face flip or
a normal scaled by the wrong length changes the normal sums, a depth minimum
that orders bits wrongly the depth, a wave taking another wave's sample the
sums of a pass that starts at sample_begin = 5.
"""
import ctypes as C

import numpy as np
import pytest

import edge_scenes as E
import feat_oracle as F
from test_gpu_feat import GEO_CAMERA, GEO_DEFOCUS, Env, Feat, _cam, _geo_scene, _params, _source, _upload, _with_variant

pytestmark = pytest.mark.gpu

VARIANTS = ((0, 0), (5, 2), (12, 1))     # rt_set_variant -> the source rt_feat_occupancy reports
CASES = [(n, "direct") for n in E.NAMES] + [(n, "rejection") for n in E.REJECTION_NAMES]


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    e = Env()
    e.torch = torch
    e.ds = None
    return e


def _bits(a):
    return a.view(np.uint32)


def _check(env, sc, cam, w, h, passes, seed, flags=0, begin=0, rejection=False, label="", variants=VARIANTS, **sel):
    """Every variant's rt_feat after `passes` (sample counts, consecutive from
    `begin`) against the mirror's passes added up -> the mirror's arrays.
    variants: (selector, the source rt_feat_occupancy must report) pairs; the
    default is a small scene's, whose tree fits the LDS budget."""
    from rtclj._lib import lib
    want = None
    b = begin
    for n in passes:
        m = F.mirror(sc, cam, w, h, n, seed, b, rejection, **sel.get("mirror", {}))
        want = m if want is None else F.add(want, m)
        b += n
    total = sum(passes)
    want_frame = F.resolve_np(want["sums"], want["hits"], want["depth"], total)
    ds = _upload(sc)
    try:
        for v, source in variants:
            def run():
                assert _source(ds) == source, (label, v)
                p0 = _params(w, h, total, seed=seed, flags=flags, **sel.get("params", {}))
                ft = Feat(env, p0, ds)
                try:
                    b = begin
                    for n in passes:
                        ft.add(cam, _params(w, h, n, begin=b, seed=seed, flags=flags, **sel.get("params", {})))
                        b += n
                    assert ft.samples == total
                    got = ft.read()
                    rows = got[1].shape[0]
                    assert ft.counters() == [rows * w * total] * 2
                    return got, ft.frame()        # resolved into a NaN-filled buffer; equal to the host's
                finally:
                    ft.free()
            (sums, hits, depth), frame = _with_variant(v, run)
            assert sums.shape == want["sums"].shape, (label, v)
            assert np.array_equal(hits, want["hits"]), (label, v, int((hits != want["hits"]).sum()))
            assert np.array_equal(_bits(depth), _bits(want["depth"])), (label, v)
            bad = (sums != want["sums"]).any(axis=-1)
            assert not bad.any(), (label, v, int(bad.sum()), np.argwhere(bad)[:3].tolist())
            assert np.array_equal(_bits(frame), _bits(want_frame)), (label, v)
    finally:
        lib.rt_scene_free(ds)
    return want


# ---- the reference scene and the geo scene --------------------------------------------------------
W2, H2 = 64, 40


@pytest.mark.parametrize("wide", [False, True], ids=["reference", "wide"])
@pytest.mark.parametrize("flag", ["default", "rejection", "realm"])
def test_reference_scene(env, flag, wide):
    from rtclj import raytracing as R
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    flags = {"default": 0, "rejection": RT_FLAG_REJECTION_SAMPLERS, "realm": RT_FLAG_REALM}[flag]
    sc = R.Scene.from_bodies(R.hittables)
    m = _check(env, sc, _cam(W2, H2, wide), W2, H2, (3, 5), 9, flags=flags, rejection=flag == "rejection",
               label=f"reference {flag} wide={wide}")
    assert (0 < m["hits"].mean() < 8) == wide and m["sums"][..., 3:6].any()


@pytest.mark.parametrize("defocus", [0.0, GEO_DEFOCUS])
def test_geo_scene(env, defocus):
    from rtclj import raytracing as R
    cam = R.camera(W2, H2, defocus_angle=defocus, **GEO_CAMERA)
    m = _check(env, _geo_scene(), cam, W2, H2, (1, 3), 5, label=f"geo defocus={defocus}")
    assert 0.2 < (m["hits"] == 4).mean() < 0.98 and (m["hits"] == 0).any()


def test_interleaved_rows(env):
    """60 x 36 (a partial tile across), row tiles of one row, every second of
    them from the second on: the mirror's rows 1, 3, ..."""
    from rtclj import raytracing as R
    sc = R.Scene.from_bodies(R.hittables)
    m = _check(env, sc, _cam(60, 36, True), 60, 36, (3, 5), 9, label="interleaved",
               mirror=dict(rows=(1, 36), row_step=2), params=dict(row_tile=1, tile_first=1, tile_step=2))
    assert m["hits"].shape == (18, 60) and 0 < m["hits"].mean() < 8


def test_albedo_clamp(env):
    """fix24's ends on an albedo: 256 and above add 2^32 - 1 per sample, a
    negative channel and a NaN nothing (edge_scenes' albedo_saturating stops at
    40, which a first hit adds unclamped)."""
    from test_gpu_feat import _fixed_cam, _scene
    sc = _scene([(0, 0, -3, 1, 0, (300.0, -1.0, float("nan")))])
    m = _check(env, sc, _fixed_cam(), 8, 8, (5, 11), 9, label="clamp")
    assert (m["hits"] == 16).all() and (m["sums"][..., 0:3] == (16 * 0xffffffff, 0, 0)).all()


# ---- the edge inputs ------------------------------------------------------------------------------------
def _non_vacuous(name, sc, cam, m):
    """What the case is about shows in the mirror's own arrays (16 spp)."""
    body, rays = m["body"], m["rays"].astype(np.float64)
    hit = body >= 0
    if name == "scale_2^63":
        assert not hit.any() and not m["sums"][..., 3:6].any()
        return
    assert hit.any()
    if name in ("camera_inside_glass", "neg_radius_field"):
        # the stored normal is turned against the ray: where it points along (P - C) / r's opposite,
        # the face was a back face (camera_inside_glass) or the radius negative (inward normals)
        o, d, t = rays[..., 0:3], rays[..., 3:6], m["t"]
        with np.errstate(invalid="ignore"):
            u = d / np.linalg.norm(d, axis=-1, keepdims=True)
            p = o + u * np.where(hit, t, 0.0)[..., None]
        sph = sc.sphere.astype(np.float64)[np.where(hit, body, 0)]
        outward = (p - sph[..., :3]) / np.abs(sph[..., 3:4])        # geometric, whatever r's sign
        back = hit & ((outward * d).sum(-1) > 0)                    # n . d sign: leaving the body
        if name == "camera_inside_glass":
            assert back.mean() > 0.2
        else:
            neg = hit & (sph[..., 3] < 0)
            assert neg.sum() > 100
            # (P - C) / r points inward there and is flipped like a back face: the sums still oppose d
        single = (body == body[..., :1]).all(-1) & hit.all(-1)
        n = m["sums"][..., 3:6] / F.ONE / body.shape[-1]
        assert ((n[single] * d[single].mean(axis=1)).sum(-1) < 0).all()
    if name == "ties":
        meta = E.case(name)[2]
        group = np.asarray(meta["group"])
        first = {g: int(np.nonzero(group == g)[0][0]) for g in set(group.tolist()) if g >= 0}
        hit_groups = group[body[hit]]
        assert (hit_groups >= 0).sum() > 1000
        twins = body[hit][hit_groups >= 0]
        assert all(b == first[g] for b, g in zip(twins[:4000].tolist(), hit_groups[hit_groups >= 0][:4000].tolist()))
        # and the albedo sums hold that twin's fix24, exactly
        per_body = F.body_albedo_fix24(sc)
        whole = hit.all(-1)
        assert np.array_equal(m["sums"][..., 0:3][whole], per_body[body].sum(-2).astype(np.int64)[whole])
    if name == "albedo_saturating":
        # A first hit adds the albedo itself, 40: far above a colour's [0, 1], yet below fix24's
        # clamp at 256, which only a path's product of albedos reaches (test_albedo_clamp holds it).
        n = body.shape[-1]
        assert (m["sums"][..., 0:3] == n * (40 << 24)).all(-1).any()
        assert (F.resolve_np(m["sums"], m["hits"], m["depth"], n)[..., 0:3] == 40.0).any()


@pytest.mark.parametrize("name,samplers", CASES)
def test_edge_inputs(env, name, samplers):
    from rtclj._lib import RT_FLAG_REJECTION_SAMPLERS
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    rejection = samplers == "rejection"
    want = _check(env, sc, cam, E.W, E.H, (5, 11), p["seed"], begin=p["sample_begin"], rejection=rejection,
                  flags=RT_FLAG_REJECTION_SAMPLERS if rejection else 0, label=f"{name} {samplers}")
    whole = F.edge_mirror(name, rejection=rejection, detail=True)
    for k in ("sums", "hits", "depth"):      # 5 + 11 added up is the mirror's 16 in one pass
        assert want[k].tobytes() == whole[k].tobytes(), k
    _non_vacuous(name, sc, cam, whole)
