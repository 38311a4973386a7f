"""The BVH walk's box padding (raytracing-clj_amd/csrc/bvh_pad.h) on the GPU:
every BVH variant against the brute-force scan (variant 5), bit for bit, on
small scenes each aimed at one way a padding that follows the hit distance
(2e-3 * (t + c0) per axis; the ray-wide 2e-3 * D for a ray with a direction
component at or under the limit, or a body as large as its tree) could cull a
hit the scan reports:

  * near-axis rays: a narrow field of view straight down each axis, so the
    two minor direction components run over about +-7e-3 and +-4e-3 and
    straddle k = 2e-3 and the limit 3e-3 on both sides (the
    existing axis test covers exactly-zero components only);
  * tangency from far away: a row of equal small spheres seen edge-on from
    1000 units, where 6e-4 * |oc| far exceeds r;
  * mixed radii: one r = 5 body in the tree among r = 0.05 ones (c0 follows
    the largest), and r = 1e-3 bodies, where the rounding term of c0 decides;
  * origins inside boxes: chains through glass spheres (the self-hit guard,
    far-root exits) and mirrors touching each other.

The boxes only cull, so the frames and the segment counts must be equal.
Frames are 64 x 36 at 16 spp, depth 8, at most 33 bodies.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BVH_VARIANTS = (11, 12, 16, 18, 22, 24, 26)
PRODUCT_VARIANTS = (0, 5, 12, 16, 18, 22, 24, 26, 28)
W, H, SPP, DEPTH = 64, 36, 16, 8
LAMBERT, METAL, GLASS = 0, 1, 2


def _scene(sph, kind, param, seed):
    from rtclj import raytracing as R
    rng = np.random.default_rng(seed)
    n = len(sph)
    mat = np.column_stack([rng.uniform(0.3, 1.0, (n, 3)), np.asarray(param, np.float64)]).astype(np.float32)
    return R.Scene(np.asarray(sph, np.float32), np.asarray(kind, np.int32), mat)


def _mixed_kinds(rng, n):
    kind = rng.integers(0, 3, n)
    return kind, np.where(kind == GLASS, 1.5, np.where(kind == METAL, 0.0, 0.3))


def _render_all(sc, cam, flags):
    """Frame and segment count per variant (the scan first)."""
    from rtclj import raytracing as R
    from rtclj._lib import diag_lib, lib
    out = {}
    for v in (5,) + BVH_VARIANTS:
        dll = lib if v in PRODUCT_VARIANTS else diag_lib()
        old = dll.rt_set_variant(v)
        assert old >= 0, dll.rt_last_error()
        try:
            st = {}
            img = R.render(sc, cam, W, H, spp=SPP, max_depth=DEPTH, seed=7, stats=st, flags=flags, library=dll)
        finally:
            dll.rt_set_variant(old)
        out[v] = (img, st["segments"])
    return out


def _assert_bvh_equals_scan(sc, cam, samplers=("direct", "rejection"), min_hit=0.05):
    from rtclj._lib import RT_FLAG_REJECTION_SAMPLERS
    for s in samplers:
        out = _render_all(sc, cam, RT_FLAG_REJECTION_SAMPLERS if s == "rejection" else 0)
        ref, segs = out[5]
        # the case is about hits: a share of the paths must meet a body
        # (every sample is at least one segment; a hit adds more)
        assert segs >= (1.0 + min_hit) * W * H * SPP, (s, segs)
        for v in BVH_VARIANTS:
            img, sg = out[v]
            assert np.array_equal(ref, img), (s, v, int((ref != img).any(axis=-1).sum()))
            assert sg == segs, (s, v, sg, segs)


# ---- near-axis rays ---------------------------------------------------------

@pytest.mark.parametrize("axis,sign", [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)])
def test_near_axis_rays(gpu_lib, axis, sign):
    from rtclj import raytracing as R
    rng = np.random.default_rng(10 + axis)
    n = 33
    # the view from 100 units is 1.42 x 0.8 wide; the bodies fill it, 6 deep
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    sph = np.zeros((n, 4))
    sph[:, a] = rng.uniform(-3, 3, n)
    sph[:, b] = rng.uniform(-0.7, 0.7, n)
    sph[:, c] = rng.uniform(-0.7, 0.7, n)
    sph[:, 3] = rng.uniform(0.05, 0.2, n)
    kind, param = _mixed_kinds(rng, n)
    sc = _scene(sph, kind, param, axis)
    frm = [0.0, 0.0, 0.0]
    frm[a] = -100.0 * sign
    vup = [0.0, 0.0, 0.0]
    vup[b] = 1.0
    vfov = float(np.degrees(2 * np.arctan(4e-3)))   # minor components within +-4e-3 (x 16/9 across)
    cam = R.camera(W, H, vfov, tuple(frm), (0.0, 0.0, 0.0), tuple(vup), 0.0, 100.0)
    _assert_bvh_equals_scan(sc, cam)


# ---- tangency from far away -------------------------------------------------

def test_far_tangency(gpu_lib):
    from rtclj import raytracing as R
    n = 24
    sph = np.zeros((n, 4))
    sph[:, 0] = 0.5 * np.arange(n)
    sph[:, 3] = 0.2
    rng = np.random.default_rng(3)
    kind, param = _mixed_kinds(rng, n)
    sc = _scene(sph, kind, param, 3)
    # edge-on along the row: the frame is 0.53 x 0.3 at the first sphere, so
    # its rim (r = 0.2) runs through the frame
    vfov = float(np.degrees(2 * np.arctan(0.15 / 1000.0)))
    cam = R.camera(W, H, vfov, (-1000.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 1000.0)
    _assert_bvh_equals_scan(sc, cam)
    # and slightly off the axis, so no component is near zero
    cam = R.camera(W, H, vfov, (-1000.0, 30.0, 20.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 1000.0)
    _assert_bvh_equals_scan(sc, cam, samplers=("direct",))


# ---- mixed radii ------------------------------------------------------------

@pytest.mark.parametrize("n_big", [1, 9])
def test_large_body_in_tree(gpu_lib, n_big):
    """r = 5 in the tree among r = 0.05: with 8 bodies no body leaves the tree
    (bvh.cpp keeps every body of a scene of at most 8); with nine r = 5
    bodies the eight first leave and the ninth stays."""
    from rtclj import raytracing as R
    rng = np.random.default_rng(20 + n_big)
    n = 8 if n_big == 1 else 33
    sph = np.zeros((n, 4))
    sph[:, 0] = rng.uniform(-3, 3, n)
    sph[:, 1] = rng.uniform(0, 1.5, n)
    sph[:, 2] = rng.uniform(-6, -1, n)
    sph[:, 3] = 0.05
    for i in range(n_big):
        sph[i] = (rng.uniform(-20, 20), -5.2 - 11.0 * (i % 3), -12.0 - 11.0 * (i // 3), 5.0)
    sph[0] = (0.0, -5.0, -3.0, 5.0)   # under the small ones
    kind, param = _mixed_kinds(rng, n)
    sc = _scene(sph, kind, param, n_big)
    cam = R.camera(W, H, 40.0, (0.0, 1.5, 3.0), (0.0, 0.3, -3.0), (0.0, 1.0, 0.0), 0.0, 6.0)
    _assert_bvh_equals_scan(sc, cam)


@pytest.mark.parametrize("dist", [0.5, 300.0])
def test_tiny_bodies(gpu_lib, dist):
    """r = 1e-3 bodies: 3 r_max is 3e-3, and from 300 units the slab
    arithmetic's rounding (~1e-7 * D per plane) is a hundredth of a radius."""
    from rtclj import raytracing as R
    rng = np.random.default_rng(31)
    n = 33
    sph = np.zeros((n, 4))
    sph[:, :3] = rng.uniform(-0.012, 0.012, (n, 3)) + (2.0, 1.0, -3.0)
    sph[:, 3] = 1e-3
    kind, param = _mixed_kinds(rng, n)
    sc = _scene(sph, kind, param, 31)
    at = np.array((2.0, 1.0, -3.0))
    frm = at + dist * np.array((0.48, 0.6, 0.64))
    vfov = float(np.degrees(2 * np.arctan(0.009 / dist)))
    cam = R.camera(W, H, vfov, tuple(frm), tuple(at), (0.0, 1.0, 0.0), 0.0, dist)
    _assert_bvh_equals_scan(sc, cam)


# ---- origins inside boxes ---------------------------------------------------

def test_glass_chain(gpu_lib):
    """A line of touching glass spheres along the view: paths enter and leave
    body after body (the self-hit guard's far root, origins on and inside
    the boxes), a few lambertian bodies behind."""
    from rtclj import raytracing as R
    n = 20
    sph = np.zeros((n, 4))
    r = np.where(np.arange(n) % 2 == 0, 0.3, 0.15)
    z = -1.0 - np.concatenate([[0.0], np.cumsum(r[:-1] + r[1:])])
    sph[:, 2] = z
    sph[:, 3] = r
    kind = np.full(n, GLASS)
    kind[-4:] = LAMBERT
    param = np.where(kind == GLASS, 1.5, 0.0)
    sc = _scene(sph, kind, param, 41)
    cam = R.camera(W, H, 12.0, (0.1, 0.05, 3.0), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), 0.0, 4.0)
    _assert_bvh_equals_scan(sc, cam, min_hit=0.5)


def test_touching_mirrors(gpu_lib):
    """Polished metal spheres packed in contact: inter-reflection between
    bodies whose boxes overlap, from origins on their surfaces."""
    from rtclj import raytracing as R
    r = 0.25
    pts = [(2 * r * (i + 0.5 * (j % 2)), 2 * r * 0.8660254 * j, -2.0 - 0.3 * ((i + j) % 2))
           for j in range(5) for i in range(6)]
    n = len(pts)
    sph = np.zeros((n, 4))
    sph[:, :3] = np.array(pts) - (1.4, 0.9, 0.0)
    sph[:, 3] = r
    kind = np.full(n, METAL)
    sc = _scene(sph, kind, np.zeros(n), 43)
    cam = R.camera(W, H, 50.0, (0.0, 0.0, 0.6), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), 0.0, 2.6)
    _assert_bvh_equals_scan(sc, cam, min_hit=0.5)
