"""Named scenes, cameras and parameters at the edges of what rt_scene,
rt_camera and rt_params accept, shared by tests/test_oracle_input_edges.py
(CPU: the fp32 mirror against the fp64 reference semantics) and
tests/test_gpu_input_edges.py (GPU: the kernel against the mirror).

case(name) -> (Scene, rt_camera, meta).  Every frame is W x H = 64 x 36 at 16
spp, depth 12, seed 1 unless meta["params"] says otherwise; at most 120
bodies.  The base scene is the reference's five bodies (rtclj.raytracing
.hittables: 0 ground, 1 centre, 2 left glass, 3 bubble, 4 right metal) under
the reference camera; scenes that need a real tree add a seeded field of small
bodies, so that 4- and 8-body leaves, several tree levels and the big-body
list all exist.

meta keys:
  fp64       the mirror stays within oracle.pin.BOUNDS of MODE_REF64D (the
             same-draw fp64 reference): the GPU frame is held to it too.
             False: the input leaves the bounds for a reason that belongs to
             the fp32 contract (include/rt.h, rt_scene) and is compared with
             the mirror only.
  rejection  also rendered with RT_FLAG_REJECTION_SAMPLERS
  realm      also MODE_REALM32 | DIRECT against MODE_REALM64D on the CPU
  unit       every lambertian / metal albedo within [-1, 1]: the default
             launch is the compact variant 22, else 16 (u64 sums)
  params     rt_params overrides: seed, sample_begin, max_depth

rtclj is imported inside the functions: the GPU tests load torch first
(tests/conftest.py gpu_lib).
"""
import functools
import os

import numpy as np

import oracle

W, H, SPP, DEPTH, SEED = 64, 36, 16, 12, 1
BY = 9                      # oracle.pin.compare's block rows (4 x 4-pixel blocks)
NT = min(16, os.cpu_count() or 1)
LAMB, METAL, GLASS, NONE = 0, 1, 2, 3
GROUND, CENTRE, LEFT, BUBBLE, RIGHT = range(5)

SCALES = (-62, -55, -40, 20, 40, 62, 63)
ETAS = {"1": 1.0, "0.3": 0.3, "4": 4.0, "-1.5": -1.5, "0": 0.0, "inf": float("inf")}
FUZZES = {"2.5": 2.5, "-0.5": -0.5, "0": 0.0}
SEEDS = {"seed_1+2^32": 1 + 2**32, "seed_2^63+1": 2**63 + 1, "seed_2^64-1": 2**64 - 1}
# rt_params.sample_begin is an int: 2^32 - 8 does not fit it as a value.  The
# kernel keys sample k by uint32(sample_begin + k), so the int -8 carries the
# same 32 bits, and its 16 samples run over the uint32 wrap (2^32 - 8 ... 7).
SAMPLE_BEGINS = {"sample_begin_2^24-8": 2**24 - 8, "sample_begin_2^31-8": 2**31 - 8, "sample_begin_2^32-8": -8}


# ---- building blocks ---------------------------------------------------------

def _base():
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten(R.hittables)
    return sph.astype(np.float64), kind.copy(), mat.astype(np.float64)


def _ref_camera():
    from rtclj import raytracing as R
    return R.camera(W, H, **R.REFERENCE_CAMERA)


def _scene(sph, kind, mat):
    from rtclj import raytracing as R
    with np.errstate(over="ignore"):
        return R.Scene(np.asarray(sph, np.float32), np.asarray(kind, np.int32), np.asarray(mat, np.float32))


def _field(rng, n, kinds=(LAMB, METAL, GLASS)):
    """n small bodies in the reference camera's view, mixed materials."""
    sph = np.column_stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-0.4, 0.8, n), rng.uniform(-3.0, 0.0, n),
                           rng.uniform(0.04, 0.15, n)])
    kind = rng.choice(kinds, n)
    mat = np.column_stack([rng.uniform(0.2, 1.0, (n, 3)),
                           np.where(kind == GLASS, 1.5, np.where(kind == METAL, rng.uniform(0, 0.5, n), 0.0))])
    return sph, kind, mat


def _with_field(seed, n=40, kinds=(LAMB, METAL, GLASS)):
    sph, kind, mat = _base()
    f = _field(np.random.default_rng(seed), n, kinds)
    return np.vstack([sph, f[0]]), np.concatenate([kind, f[1]]), np.vstack([mat, f[2]])


def _scaled_camera(cam, k):
    """cam with every length times 2^k (exact in float32 while in range)."""
    from rtclj._lib import rt_camera
    out = rt_camera()
    s = np.float32(2.0) ** np.float32(k)
    for f in ("center", "p00", "du", "dv", "disk_u", "disk_v"):
        v = np.asarray(list(getattr(cam, f)), np.float32) * s
        assert np.isfinite(v).all() and ((v == 0) | (np.abs(v) >= 2.0 ** -126)).all(), (f, k)
        setattr(out, f, (type(getattr(out, f)))(*v.tolist()))
    out.defocus = cam.defocus
    return out


def primary_len2(cam):
    """float32 |d|^2 of the primary rays through every pixel's four corners
    (the jitter's range), from the camera centre: (min, max), and the largest
    |d|^2 the defocus disk could add, as float64."""
    c, p00, du, dv = (np.asarray(list(getattr(cam, f)), np.float64) for f in ("center", "p00", "du", "dv"))
    fx, fy = np.meshgrid(np.arange(W + 1) - 0.5, np.arange(H + 1) - 0.5)
    d = p00 + fx[..., None] * du + fy[..., None] * dv - c
    with np.errstate(over="ignore"):
        l2 = (d * d).sum(-1).astype(np.float32)
    disk = sum(np.abs(np.asarray(list(getattr(cam, f)), np.float64)).sum() for f in ("disk_u", "disk_v"))
    return float(l2.min()), float(l2.max()), float(disk) if cam.defocus else 0.0


# ---- the cases -----------------------------------------------------------------

def _materials(name):
    sph, kind, mat = _base()
    meta = dict(fp64=True, unit=True)
    if name == "albedo_gt1":
        mat[CENTRE, :3] = (3.0, 1.5, 0.5)
        mat[GROUND, :3] = (0.8, 0.8, 1.2)
        mat[RIGHT] = (1.5, 1.2, 0.9, 0.2)
        # the three together reach 29 per channel, and BOUNDS' lin_mean is
        # absolute: mirror vs MODE_REF64D 0.0104 (> 5e-4) with every other
        # statistic inside (px8_mean 0.0025, block_max 0.63).  Each of the
        # three alone (albedo_gt1_*) stays within BOUNDS.
        meta.update(fp64=False, unit=False, rejection=True)
    elif name == "albedo_gt1_centre":
        mat[CENTRE, :3] = (3.0, 1.5, 0.5)
        meta.update(unit=False, rejection=True)
    elif name == "albedo_gt1_ground":
        mat[GROUND, :3] = (0.8, 0.8, 1.2)
        meta.update(unit=False, rejection=True)
    elif name == "albedo_gt1_metal":
        mat[RIGHT] = (1.5, 1.2, 0.9, 0.2)
        meta.update(unit=False, rejection=True)
    elif name == "albedo_negative":
        mat[GROUND, :3] = (0.8, -0.5, 0.0)
        meta.update(fp64=False)
    elif name == "albedo_saturating":
        mat[GROUND, :3] = 40.0
        mat[CENTRE, :3] = 40.0
        meta.update(fp64=False, unit=False)
    elif name.startswith("fuzz_"):
        mat[RIGHT, 3] = FUZZES[name[5:]]
    elif name.startswith("eta_"):
        mat[LEFT, 3] = ETAS[name[4:]]
        meta.update(rejection=True, realm=True)
    elif name == "bubble_negative_radius":
        sph[BUBBLE, 3] = -0.4
        mat[BUBBLE, 3] = 1.5
        meta.update(rejection=True, realm=True)
    else:
        raise KeyError(name)
    return _scene(sph, kind, mat), _ref_camera(), meta


def _neg_radius_field():
    sph, kind, mat = _with_field(101, 40, (LAMB, METAL, GLASS, NONE))
    sph[5::3, 3] *= -1.0           # a third of the field's radii
    assert (sph[:, 3] < 0).sum() == 14
    return _scene(sph, kind, mat), _ref_camera(), dict(fp64=True, unit=True)


TIE_MATERIALS = ((LAMB, (1.0, 0.0, 0.0, 0.0)), (NONE, (0.0, 0.0, 0.0, 0.0)), (METAL, (0.9, 0.9, 0.9, 0.0)))


def _ties():
    """12 positions x 3 identical spheres (one lambertian red, one without a
    material, one metal) and a ground, the 37 indices permuted: which copy
    comes first, and where the copies fall in the trees' leaves, varies
    (tests/test_oracle_input_edges.py looks at the trees)."""
    rng = np.random.default_rng(202)
    # clusters of five, four and three overlapping positions: inside a
    # cluster every cut costs the surface-area split about the same area, so
    # the cuts fall where they save a leaf -- 15 bodies into 8-body leaves
    # only as 7 + 8 or 8 + 7, 12 into 4-body leaves at 4 and 8: inside triples
    pos = np.array([(cx + 0.125 * i, 0.25 + 0.0625 * (i % 2), -1.5 - 0.125 * i)
                    for cx, m in ((-1.5, 5), (-0.125, 4), (1.0, 3)) for i in range(m)])
    sph = [(0.0, -100.5, -1.0, 100.0)]
    kind = [LAMB]
    mat = [(0.5, 0.5, 0.5, 0.0)]
    group = [-1]
    for g, p in enumerate(pos):
        for k, m in TIE_MATERIALS:
            sph.append((*p, 0.375))
            kind.append(k)
            mat.append(m)
            group.append(g)
    perm = rng.permutation(len(sph))
    sph, kind, mat, group = (np.asarray(a)[perm] for a in (sph, kind, mat, group))
    from rtclj import raytracing as R
    cam = R.camera(W, H, 40.0, (0.0, 0.5, 3.0), (0.0, 0.25, -1.5), (0.0, 1.0, 0.0), 0.0, 4.5)
    return _scene(sph, kind, mat), cam, dict(fp64=True, unit=True, rejection=True, realm=True, group=group)


def ties_keep_one(sc, group, last=False):
    """The ties scene with the material of every twin but the first (last:
    but the last) of its group replaced by RT_NONE, and the groups whose
    kept twin is lambertian."""
    kind = sc.kind.copy()
    seen = set()
    kept_lamb = []
    order = range(len(group) - 1, -1, -1) if last else range(len(group))
    for i in order:
        g = group[i]
        if g < 0:
            continue
        if g in seen:
            kind[i] = NONE
        else:
            seen.add(g)
            if kind[i] == LAMB:
                kept_lamb.append(g)
    return _scene(sc.sphere, kind, sc.mat), kept_lamb


def _ties_big(glass):
    """Ten identical-in-pairs r = 1 spheres among 40 r = 0.1 bodies: the
    eight of lowest index leave the tree for the big-body list, two stay, and
    the twin pairs (6, 8) and (7, 9) of the ten straddle that boundary.
    glass: the first twin of the middle pair is a dielectric.  A path inside
    it leaves through the body it entered, whose root is 2 |h| under the
    kernel's self-hit guard (sq = |h|), while its lambertian twin's is h +
    sqrt(disc): the two differ by a rounding and either may win, where the
    fp64 path (no guard, exactly equal roots) always takes the first.  That
    case is therefore outside BOUNDS (mirror vs MODE_REF64D: seg_rel 0.10)
    and compared with the mirror only."""
    rng = np.random.default_rng(303)
    n_small = 40
    small = np.column_stack([rng.uniform(-5, 5, n_small), rng.uniform(-0.9, 1.5, n_small),
                             rng.uniform(-5.0, -1.0, n_small), np.full(n_small, 0.1)])
    skind = rng.choice((LAMB, METAL, GLASS), n_small)
    smat = np.column_stack([rng.uniform(0.2, 1.0, (n_small, 3)), np.where(skind == GLASS, 1.5, 0.1)])
    centres = [(-4.5, 0.0, -6.0), (-2.25, 0.0, -6.5), (0.0, 0.0, -6.0), (2.25, 0.0, -6.5), (4.5, 0.0, -6.0)]
    pair_of = (0, 0, 1, 1, 2, 2, 3, 4, 3, 4)     # the ten big bodies in index order -> position
    bkinds = (LAMB, METAL, METAL, LAMB, GLASS if glass else METAL, LAMB, LAMB, NONE, METAL, LAMB)
    slots = np.sort(rng.choice(n_small + 10, 10, replace=False))
    sph, kind, mat = [], [], []
    b = s = 0
    for i in range(n_small + 10):
        if b < 10 and i == slots[b]:
            sph.append((*centres[pair_of[b]], 1.0))
            kind.append(bkinds[b])
            mat.append((0.9, 0.3 + 0.06 * b, 0.2, 1.5 if bkinds[b] == GLASS else 0.0))
            b += 1
        else:
            sph.append(tuple(small[s]))
            kind.append(skind[s])
            mat.append(tuple(smat[s]))
            s += 1
    from rtclj import raytracing as R
    cam = R.camera(W, H, 28.0, (0.0, 1.0, 5.0), (0.0, 0.0, -6.0), (0.0, 1.0, 0.0), 0.0, 11.0)
    sc = _scene(np.array(sph), np.array(kind), np.array(mat))
    big = np.nonzero(sc.sphere[:, 3] == 1.0)[0]
    assert len(big) == 10 and all((sc.sphere[big[a]] == sc.sphere[big[b]]).all() for a, b in ((6, 8), (7, 9)))
    return sc, cam, dict(fp64=not glass, unit=True, rejection=True)


NAN, INF = float("nan"), float("inf")
NONFINITE_FEW = [(NAN, 0.0, -1.0, 0.5), (0.0, INF, -1.0, 0.5), (0.0, 0.0, -INF, 0.5),   # centres
                 (0.0, 0.5, -1.0, NAN), (0.0, 0.0, -1.0, INF),                            # radii
                 (0.3, 0.1, -0.7, 0.0), (-0.4, 0.3, -0.9, 0.0), (0.0, 0.0, -1.0, 1e30)]
# the interleaved ones of nonfinite_{64, 65, 80}: none of them finite
NONFINITE_KINDS = [(NAN, 0.0, -1.0, 0.5), (0.0, INF, -1.0, 0.5), (0.0, 0.0, -INF, 0.5), (0.0, 0.5, -1.0, NAN),
                   (0.0, 0.0, -1.0, INF), (0.5, 0.0, -1.0, -INF), (INF, -INF, NAN, 0.25)]


def _nonfinite_few():
    sph, kind, mat = _base()
    n = len(NONFINITE_FEW)
    sph = np.vstack([sph, np.array(NONFINITE_FEW)])
    kind = np.concatenate([kind, np.array([LAMB, METAL, GLASS, LAMB, LAMB, LAMB, METAL, LAMB])])
    extra = np.tile((0.9, 0.1, 0.9, 0.0), (n, 1))
    extra[2, 3] = 1.5
    return _scene(sph, kind, np.vstack([mat, extra])), _ref_camera(), dict(fp64=False, unit=True, n_base=5)


def without_bodies(sc, keep):
    return _scene(sc.sphere[keep], sc.kind[keep], sc.mat[keep])


def _nonfinite_many(m):
    """40 finite bodies (the base five and a field of 35) interleaved with m
    non-finite ones: bvh.cpp's former limit of 64 bodies without a box lies
    between nonfinite_64 and nonfinite_65."""
    fs, fk, fm = _with_field(404, 35)
    n = len(fk) + m
    bad = np.zeros(n, bool)
    bad[np.round(np.linspace(0, n - 1, m)).astype(int)] = True
    assert bad.sum() == m
    sph, kind, mat = np.zeros((n, 4)), np.zeros(n, np.int32), np.zeros((n, 4))
    sph[~bad], kind[~bad], mat[~bad] = fs, fk, fm
    sph[bad] = [NONFINITE_KINDS[i % len(NONFINITE_KINDS)] for i in range(m)]
    kind[bad] = [(LAMB, METAL, GLASS)[i % 3] for i in range(m)]
    mat[bad] = (0.9, 0.1, 0.9, 1.5)
    return _scene(sph, kind, mat), _ref_camera(), dict(fp64=False, unit=True, finite=~bad)


def _origin_on_surface():
    """No defocus, the camera centre at the origin: a glass sphere through it
    (centre (0, 0, -1), r = 1: c = |oc|^2 - r^2 = +0 exactly for every primary
    ray), a glass sphere around it (centre = camera: oc = 0, h = +-0 by the
    direction's signs, c = -r^2), eight small bodies behind.  Coordinates are
    powers of two and their small sums, so the zeros are exact in float32."""
    from rtclj import raytracing as R
    sph = [(0.0, 0.0, -1.0, 1.0), (0.0, 0.0, 0.0, 0.5)]
    kind = [GLASS, GLASS]
    mat = [(0.0, 0.0, 0.0, 1.5), (0.0, 0.0, 0.0, 1.5)]
    for i, x in enumerate((-1.0, -0.5, 0.5, 1.0)):
        for j, y in enumerate((-0.25, 0.25)):
            sph.append((x, y, -4.0, 0.125))
            kind.append(METAL if (i + j) % 2 else LAMB)
            mat.append((0.75, 0.5, 0.25, 0.0))
    sc = _scene(np.array(sph), np.array(kind), np.array(mat))
    cam = R.camera(W, H, 40.0, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.0, 1.0)
    # the zeros, in the kernel's own float32 ops (fma as the exactly rounded
    # double sum: every term here is exact)
    f = np.float32
    o = np.asarray(list(cam.center), f)
    assert (o == 0).all() and not cam.defocus
    oc = sc.sphere[0, :3] - o
    w = -(sc.sphere[0, 3] * sc.sphere[0, 3])
    c = f(f(f(oc[1] * oc[1] + w) + oc[2] * oc[2]) + oc[0] * oc[0])
    assert c == 0.0 and not np.signbit(c)
    assert ((sc.sphere[1, :3] - o) == 0).all() and -(sc.sphere[1, 3] ** 2) == f(-0.25)
    return sc, cam, dict(fp64=True, unit=True)


def _camera_inside_glass():
    from rtclj import raytracing as R
    sph, kind, mat = _base()
    # between the bubble (r = 0.4) and the glass surface (r = 0.5) around (-1, 0, -1)
    cam = R.camera(W, H, 60.0, (-1.0, 0.0, -0.55), (0.0, 0.0, -1.2), (0.0, 1.0, 0.0), 0.0, 1.0)
    d = np.linalg.norm(np.asarray(list(cam.center)) - sph[LEFT, :3])
    assert 0.4 < d < 0.5
    return _scene(sph, kind, mat), cam, dict(fp64=True, unit=True)


def _scale(k):
    """Scene and camera times 2^k.  Non-vacuity, in float32: k = -55, -62 put
    every primary ray's |d|^2 below 2^-96 (trace_kernel.h's cold length
    branch); at k = -62 the smallest body's r * r is denormal (< 2^-126); at
    k = 63 every primary ray's |d|^2 overflows (the same branch from above).
    At k = 62 it does not: |d|^2 <= 13.1 x 2^124 < 2^128, the top of the hot
    branch's range, while the ground's r * r overflows."""
    sph, kind, mat = _base()
    sc = _scene(np.ldexp(sph, k), kind, mat)
    cam = _scaled_camera(_ref_camera(), k)
    assert np.array_equal(sc.sphere.astype(np.float64), np.ldexp(sph.astype(np.float32).astype(np.float64), k))
    lo, hi, disk = primary_len2(cam)
    f = np.float32
    with np.errstate(over="ignore", under="ignore"):
        rr = sc.sphere[:, 3] * sc.sphere[:, 3]
    if k in (-55, -62):
        assert (np.sqrt(hi) + disk) ** 2 < 2.0 ** -96 and lo > 0
    if k == -62:
        assert 0 < rr.min() < f(2.0 ** -126)
    if k == -40 or k == 20 or k == 40:
        assert 2.0 ** -96 <= lo and hi < 2.0 ** 127
    if k == 62:
        assert 2.0 ** 127 < lo and np.isfinite(hi) and np.isinf(rr.max())
    if k == 63:
        assert np.isinf(lo) and (3.3 * 2.0 ** 63 - disk) ** 2 > 2.0 ** 128
    return sc, cam, dict(fp64=k in (-62, -55, -40, 20), unit=True, rejection=True, scale=k)


def _rng_case(name):
    sph, kind, mat = _base()
    if name in SEEDS:
        params = dict(seed=SEEDS[name])
    elif name in SAMPLE_BEGINS:
        params = dict(sample_begin=SAMPLE_BEGINS[name])
    else:
        params = dict(max_depth=-1)
    return _scene(sph, kind, mat), _ref_camera(), dict(fp64=True, unit=True, params=params)


NAMES = (["albedo_gt1", "albedo_gt1_centre", "albedo_gt1_ground", "albedo_gt1_metal", "albedo_negative", "albedo_saturating"] + [f"fuzz_{k}" for k in FUZZES] +
         [f"eta_{k}" for k in ETAS] +
         ["bubble_negative_radius", "neg_radius_field", "ties", "ties_big", "ties_big_glass", "nonfinite_few", "nonfinite_64",
          "nonfinite_65", "nonfinite_80", "origin_on_surface", "camera_inside_glass"] +
         [f"scale_2^{k}" for k in SCALES] + list(SEEDS) + list(SAMPLE_BEGINS) + ["max_depth_-1"])


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "neg_radius_field":
        out = _neg_radius_field()
    elif name == "ties":
        out = _ties()
    elif name in ("ties_big", "ties_big_glass"):
        out = _ties_big(name == "ties_big_glass")
    elif name == "nonfinite_few":
        out = _nonfinite_few()
    elif name.startswith("nonfinite_"):
        out = _nonfinite_many(int(name[10:]))
    elif name == "origin_on_surface":
        out = _origin_on_surface()
    elif name == "camera_inside_glass":
        out = _camera_inside_glass()
    elif name.startswith("scale_2^"):
        out = _scale(int(name[8:]))
    elif name in SEEDS or name in SAMPLE_BEGINS or name == "max_depth_-1":
        out = _rng_case(name)
    else:
        out = _materials(name)
    sc, cam, meta = out
    assert len(sc) <= 120 and meta["fp64"] == (name in FP64_NAMES), name
    meta.setdefault("rejection", False)
    meta.setdefault("realm", False)
    meta.setdefault("params", {})
    return sc, cam, meta


# which cases the fp64 bounds apply to is a property of the input, not of a
# render: written out so that collecting the tests builds no scene
FP64_NAMES = tuple(n for n in NAMES if n not in (
    "albedo_gt1", "ties_big_glass", "albedo_negative", "albedo_saturating", "nonfinite_few", "nonfinite_64", "nonfinite_65", "nonfinite_80",
    "scale_2^40", "scale_2^62", "scale_2^63"))
REJECTION_NAMES = tuple(n for n in NAMES if n.startswith("albedo_gt1") or n.startswith("eta_") or n.startswith("scale_2^") or
                        n in ("bubble_negative_radius", "ties", "ties_big", "ties_big_glass"))
REALM_NAMES = tuple(n for n in NAMES if n.startswith("eta_") or n in ("bubble_negative_radius", "ties"))


def params(meta, **over):
    p = dict(spp=SPP, max_depth=DEPTH, seed=SEED, sample_begin=0)
    p.update(meta["params"])
    p.update(over)
    return p


def _key(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def _oracle_cached(mode, name, over):
    sc, cam, meta = case(name)
    return oracle_render(mode, sc, cam, **params(meta, **dict(over)))


def oracle_render(mode, sc, cam, spp=SPP, max_depth=DEPTH, seed=SEED, sample_begin=0):
    """-> (float32 frame, segments, samples); treat the frame as read-only."""
    img, _, segs, smp = oracle.render(mode, sc.sphere.astype(np.float64), sc.kind, sc.mat.astype(np.float64),
                                      cam.as_list(), cam.defocus, W, H, spp, max_depth, seed=seed,
                                      sample_begin=sample_begin, nthreads=NT)
    img.setflags(write=False)
    return img, segs, smp


def mirror(name, rejection=False, realm=False, **over):
    """The fp32 kernel mirror's render of a case (computed once per process)."""
    base = oracle.MODE_REALM32 if realm else oracle.MODE_MIRROR32
    return _oracle_cached(base | (0 if rejection else oracle.DIRECT), name, _key(over))


def ref64(name, realm=False, **over):
    """The same-draw fp64 reference's render of a case (MODE_REF64D /
    MODE_REALM64D; computed once per process)."""
    return _oracle_cached(oracle.MODE_REALM64D if realm else oracle.MODE_REF64D, name, _key(over))
