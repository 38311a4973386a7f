"""oracle.features (oracle/rt_oracle.cpp, oracle_features) -- the feature pass's
fp32 mirror and its same-draw fp64 partner -- checked on the CPU before any
device is held to them (tests/test_gpu_feat_oracle.py):

  1. the ten known answers of tests/test_gpu_feat.py from the mirror alone;
  2. on the reference scene the mirror's hits are the black pixels of the path
     mirror's 1-spp max_depth = 1 frames, and without materials its resolved
     albedo is that frame (the GPU identity of
     test_hits_are_the_path_kernels_black_pixels, on the CPU): the new code is
     tied to the already pinned MODE_MIRROR32;
  3. mirror against fp64 on the pixels whose per-sample bodies agree.

Measured over the reference scene (both cameras, both samplers), the geo scene
(with and without defocus) and FP64_CASES (64 x 36, 16 spp; with the rejection
disk too where edge_scenes.REJECTION_NAMES says so):
  sky, |fp32 fma chain - fp64| per miss sample: 6.06e-8 at the most (ties_big;
    the 2^-24 truncation of fix24 is 5.96e-8 of it) -> SKY_MEASURED;
  pixels whose per-sample `body` arrays disagree: none, in every case (the
    condition is at most 5 %): no case had to leave the list;
  depth and normal differences: at most 0.086 and 0.25 of their bounds.
"""
import numpy as np
import pytest

import edge_scenes as E
import feat_oracle as F
import oracle
from test_gpu_feat import GEO_CAMERA, GEO_DEFOCUS, K_BOUND, KNOWN, ONE, _cam, _fixed_cam, _geo_scene, _scene, fix24

# The largest |sky32 - sky64| per miss sample over every listed case (2^-24
# units of truncation included), as measured; the bound is 4 x this.
SKY_MEASURED = 6.06e-8
SKY_BOUND = 4 * SKY_MEASURED
MAX_DISAGREE = 0.05
# name: the measured share of pixels whose per-sample bodies differ between the
# mirror and fp64 (a silhouette or t-min decision that flips in fp32)
FP64_CASES = [n for n in E.FP64_NAMES if n != "max_depth_-1"]   # rt_feat does not read max_depth
REMOVED = {}   # name: reason (a case over MAX_DISAGREE; three at most) -- none


def _ref_scene():
    from rtclj import raytracing as R
    return R.Scene.from_bodies(R.hittables)


# ---- 1: known answers -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    bodies, hits, depth, nz, alb = KNOWN[name]
    m = F.mirror(_scene(bodies), _fixed_cam(), 8, 8, 4, seed=9, want_body=True)
    assert (m["hits"] == hits).all()
    assert (m["sums"][..., 0:3] == [4 * fix24(c) for c in alb]).all(), m["sums"][0, 0]
    assert (m["sums"][..., 3:5] == 0).all()
    if depth is None:    # far_root: the device test's formula and tolerances
        ocz = np.float32(-1.0005)
        hh = np.float32(-1.0) * ocz
        cc = np.float32(np.float64(ocz) * np.float64(ocz) - 1.0)
        disc = np.float32(np.float64(hh) * np.float64(hh) - np.float64(cc))
        t = hh + np.sqrt(disc)
        ulps = np.abs(m["depth"].view(np.int32).astype(np.int64) - int(np.float32(t).view(np.int32)))
        assert ulps.max() <= 4
        assert (np.abs(m["sums"][..., 5] - 4 * ONE) <= 4 * 16).all()
    else:
        assert (m["depth"].view(np.uint32) == np.float32(depth).view(np.uint32)).all()
        assert (m["sums"][..., 5] == 4 * ONE * nz).all()
    want_body = -1 if not bodies else (9 if name == "nearest_of_many" else 0)
    assert (m["body"] == want_body).all()
    f = F.resolve_np(m["sums"], m["hits"], m["depth"], 4)
    assert np.array_equal(f[..., 0:3], np.broadcast_to(np.float32(alb), f[..., 0:3].shape))
    assert (f[..., 7] == hits / 4).all()


# ---- 2: the path mirror's black pixels ------------------------------------------------------------
W2, H2 = 64, 40


@pytest.mark.parametrize("wide", [False, True], ids=["reference", "wide"])
@pytest.mark.parametrize("rejection", [False, True], ids=["default", "rejection"])
def test_hits_are_the_path_mirrors_black_pixels(rejection, wide):
    from rtclj import raytracing as R
    sc, cam = _ref_scene(), _cam(W2, H2, wide)
    mode = oracle.MODE_MIRROR32 | (0 if rejection else oracle.DIRECT)
    black = np.zeros((H2, W2), np.int64)
    for k in range(8):
        fr = oracle.render(mode, *F.scene_args(sc, cam), W2, H2, 1, 1, seed=9, sample_begin=k, nthreads=E.NT)[0]
        black += ~fr.any(axis=-1)
    if wide:
        assert 0.05 < black.mean() / 8 < 0.95 and ((black > 0) & (black < 8)).any()
    m = F.mirror(sc, cam, W2, H2, 8, 9, rejection=rejection)
    assert np.array_equal(m["hits"].astype(np.int64), black)
    assert np.array_equal(np.isinf(m["depth"]), m["hits"] == 0)
    # no material anywhere: a hit adds nothing, a miss the sky -- the path mirror's max_depth = 1 frame
    none = R.Scene(sc.sphere.copy(), np.full(len(sc), E.NONE, np.int32), sc.mat.copy())
    n = F.mirror(none, cam, W2, H2, 8, 9, rejection=rejection)
    want = oracle.render(mode, *F.scene_args(none, cam), W2, H2, 8, 1, seed=9, nthreads=E.NT)[0]
    got = F.resolve_np(n["sums"], n["hits"], n["depth"], 8)[..., 0:3]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want.any() == wide
    assert np.array_equal(n["sums"][..., 3:6], m["sums"][..., 3:6]) and np.array_equal(n["hits"], m["hits"])


# ---- 3: mirror against fp64 -----------------------------------------------------------------------
def compare(sc, m, r):
    """The mirror's features `m` against fp64's `r` (both with body and t) on
    the pixels whose per-sample bodies agree -> (share of pixels that disagree,
    the largest sky difference per miss sample, the worst depth and normal
    differences as shares of their bounds).  Asserts the rest."""
    spp = m["body"].shape[-1]
    agree = (m["body"] == r["body"]).all(axis=-1)
    body = m["body"]
    hit = body >= 0
    nh = hit.sum(axis=-1)
    # hits
    assert np.array_equal(m["hits"], nh.astype(np.uint32)) and np.array_equal(r["hits"][agree], m["hits"][agree])
    assert np.array_equal(m["depth"] == np.inf, nh == 0) and np.array_equal(r["depth"] == np.inf, r["hits"] == 0)
    # per sample: the body's |r|, fp64's distance
    absr = np.abs(sc.sphere[:, 3].astype(np.float64))
    rk = np.where(hit, absr[np.where(hit, body, 0)], 0.0)
    tk = np.where(hit, r["t"], 0.0)
    some = agree & (nh > 0)
    # depth: the nearest surface, within the fp32 body test's displacement bound
    with np.errstate(invalid="ignore"):
        dd = np.abs(m["depth"].astype(np.float64) - r["depth"])
    bound_d = K_BOUND * (r["depth"] + 3 * rk.max(axis=-1))
    assert (dd[some] <= bound_d[some]).all(), (dd[some] / bound_d[some]).max()
    # normals: the displacement bound as an angle, the mean over the samples, plus the truncation
    with np.errstate(invalid="ignore", divide="ignore"):
        ang = np.where(hit, K_BOUND * (tk + 3 * rk) / rk, 0.0).sum(axis=-1) / spp + 2.0 ** -23
    n32 = m["sums"][..., 3:6].astype(np.float64) / ONE / spp
    dn = np.abs(n32 - r["normal"]).max(axis=-1)
    assert (dn[some] <= ang[some]).all(), (dn[some] / ang[some]).max()
    # albedo of the hit samples: exactly fix24 of the same float; what is left is the sky's
    per_body = F.body_albedo_fix24(sc)
    hit_sum = per_body[body].sum(axis=-2).astype(np.int64)
    sky32 = m["sums"][..., 0:3] - hit_sum
    assert (sky32 >= 0).all() and not sky32[nh == spp].any()
    assert (sky32[nh < spp] > 0).all()
    kinds = np.append(sc.kind, -1)[body]
    mat64 = np.vstack([sc.mat[:, :3].astype(np.float64), np.zeros((1, 3))])[body]
    alb64 = np.where(((kinds == E.LAMB) | (kinds == E.METAL))[..., None], mat64,
                     np.where((kinds == E.GLASS)[..., None], 1.0, 0.0)).sum(axis=-2)
    sky64 = r["albedo"] * spp - alb64
    miss = agree & (nh < spp)
    sky = 0.0
    if miss.any():
        d = np.abs(sky32 / ONE - sky64).max(axis=-1) / np.maximum(spp - nh, 1)
        sky = float(d[miss].max())
    worst = (float((dd[some] / bound_d[some]).max()), float((dn[some] / ang[some]).max())) if some.any() else (0.0, 0.0)
    return float(1.0 - agree.mean()), sky, worst


def _pair(sc, cam, w, h, spp, seed, rejection=False):
    kw = dict(want_body=True, want_t=True)
    return (F.mirror(sc, cam, w, h, spp, seed, rejection=rejection, **kw),
            F.ref64(sc, cam, w, h, spp, seed, rejection=rejection, **kw))


def _check(label, sc, m, r):
    share, sky, worst = compare(sc, m, r)
    print(f"{label}: bodies disagree on {share:.4%} of the pixels, sky |d| per miss sample {sky:.3e}, "
          f"hit share {(m['body'] >= 0).mean():.3f}, worst depth / bound {worst[0]:.3g}, normal / bound {worst[1]:.3g}")
    assert share <= MAX_DISAGREE, share
    assert sky <= SKY_BOUND, sky
    return share, sky


@pytest.mark.parametrize("wide", [False, True], ids=["reference", "wide"])
@pytest.mark.parametrize("rejection", [False, True], ids=["default", "rejection"])
def test_reference_scene_against_fp64(rejection, wide):
    sc = _ref_scene()
    m, r = _pair(sc, _cam(W2, H2, wide), W2, H2, 8, 9, rejection)
    _check(f"reference scene (wide {wide}, rejection {rejection})", sc, m, r)
    assert (0 < m["hits"].mean() < 8) == wide


@pytest.mark.parametrize("defocus", [0.0, GEO_DEFOCUS])
def test_geo_scene_against_fp64(defocus):
    from rtclj import raytracing as R
    sc = _geo_scene()
    cam = R.camera(W2, H2, defocus_angle=defocus, **GEO_CAMERA)
    m, r = _pair(sc, cam, W2, H2, 4, 5)
    _check(f"geo scene (defocus {defocus})", sc, m, r)
    assert 0.2 < (m["hits"] == 4).mean() < 0.98


@pytest.mark.parametrize("defocus", [0.0, GEO_DEFOCUS])
def test_normals_are_unit_length(defocus):
    """At 1 spp a hit pixel's sums are one sample's normal: | |n| - 1 | <= 2^-20,
    the bound tests/test_gpu_feat.py holds the device to (the product's
    rounding and the 2^-24 truncation; the fp64 bound above, a displacement,
    would let a length error of 1e-3 through)."""
    from rtclj import raytracing as R
    cam = R.camera(W2, H2, defocus_angle=defocus, **GEO_CAMERA)
    m = F.mirror(_geo_scene(), cam, W2, H2, 1, 5)
    hit = m["hits"] == 1
    dev = np.abs(np.linalg.norm(m["sums"][..., 3:6] / ONE, axis=-1) - 1.0)
    assert hit.mean() > 0.2 and dev[hit].max() <= 2.0 ** -20, dev[hit].max()


@pytest.mark.parametrize("name", FP64_CASES)
def test_edge_cases_against_fp64(name):
    sc, cam, meta = E.case(name)
    m, r = F.edge_mirror(name, detail=True), F.edge_ref64(name)
    _check(name, sc, m, r)
    if name in E.REJECTION_NAMES:
        _check(name + " (rejection)", sc, F.edge_mirror(name, rejection=True, detail=True),
               F.edge_ref64(name, rejection=True))


def test_the_case_list():
    assert len(REMOVED) <= 3 and not set(REMOVED) - set(E.FP64_NAMES)
    assert set(FP64_CASES) | set(REMOVED) | {"max_depth_-1"} >= set(E.FP64_NAMES)


def test_rays_and_row_selection():
    """The returned (o, d) are the rays the bodies were found with (the known
    camera), and a row_step selection is the rows of the whole frame."""
    sc, cam = _ref_scene(), _cam(60, 36, True)
    whole = F.mirror(sc, cam, 60, 36, 4, 9, want_body=True, want_rays=True)
    part = F.mirror(sc, cam, 60, 36, 4, 9, rows=(1, 36), row_step=2, want_body=True)
    for k in ("sums", "hits", "depth", "body"):
        assert part[k].shape[0] == 18 and np.array_equal(part[k], whole[k][1::2]), k
    o, d = whole["rays"][..., 0:3].astype(np.float64), whole["rays"][..., 3:6].astype(np.float64)
    assert np.isfinite(whole["rays"]).all()
    # every origin lies on the lens disk, every o + d on the pixel's footprint in the focus plane
    c, p00, du, dv = (np.array(list(getattr(cam, f)), np.float64) for f in ("center", "p00", "du", "dv"))
    lens = np.array([list(cam.disk_u), list(cam.disk_v)], np.float64)
    q = (o - c) @ np.linalg.pinv(lens)
    assert ((q * q).sum(-1) <= 1 + 1e-5).all() and (q * q).sum(-1).max() > 0.8
    s = o + d - p00
    fx, fy = s @ du / (du @ du), s @ dv / (dv @ dv)
    jj, ii = np.meshgrid(np.arange(36), np.arange(60), indexing="ij")
    assert (np.abs(fx - ii[..., None]) <= 0.5 + 1e-3).all() and (np.abs(fy - jj[..., None]) <= 0.5 + 1e-3).all()
