"""Rays for the ray-query tests (include/rt.h: rt_launch_rays, rt_rays_host and
their occlusion twins), shared by tests/test_rays_host.py (CPU) and
tests/test_gpu_rays.py (GPU), and the fp64 reading of hittable.clj:7-31 and
raytracing.clj:33-43 they are held to.  Everything is seeded, computed once per
process and read-only.

rtclj is imported inside the functions: the GPU tests load torch first
(tests/conftest.py gpu_lib).
"""
import functools

import numpy as np

F = np.float32
INF = F(np.inf)
N_QUERY = 4096
SEED = 20260
OFFSET = 1.5


def ray_dtype():
    from rtclj._lib import RAY_DTYPE
    return np.dtype(RAY_DTYPE)


def make_rays(o, t_min, d, t_max):
    o = np.asarray(o, F)
    rays = np.zeros(o.shape[:-1], ray_dtype())
    rays["o"], rays["d"] = o, np.asarray(d, F)
    rays["t_min"], rays["t_max"] = np.asarray(t_min, F), np.asarray(t_max, F)
    return rays


@functools.lru_cache(maxsize=None)
def scene(name):
    """reference: the five bodies; cover: C1's 484; large: cover(16), 1025
    bodies, whose tree leaves LDS."""
    from rtclj import raytracing as R, scenes
    if name == "reference":
        return R.Scene.from_bodies(R.hittables)
    return scenes.cover(11) if name == "cover" else scenes.cover(16)


def scene_box(sph):
    """The box of a scene's finite bodies without its grounds (r > 50: they
    would make every origin a far one); all finite bodies if nothing is left."""
    sph = np.asarray(sph, np.float64)
    ok = np.isfinite(sph).all(axis=1)
    small = ok & (np.abs(sph[:, 3]) <= 50.0)
    use = small if small.any() else ok
    lo = (sph[use, :3] - np.abs(sph[use, 3:4])).min(axis=0)
    hi = (sph[use, :3] + np.abs(sph[use, 3:4])).max(axis=0)
    return np.flatnonzero(use), lo, hi


@functools.lru_cache(maxsize=None)
def query_rays(name, n=N_QUERY, seed=SEED, offset=OFFSET):
    """The fp64 test's rays on scene `name`: origins uniform in the scene's box
    grown twofold, each aimed at a random body's centre plus a uniform offset in
    +-1.5 r per axis, |d| log-uniform in 2^-6 .. 2^6, t_min 0 or 1e-3, t_max
    infinite for half the rays and 0.5 .. 1.5 times the target's parameter for
    the rest."""
    sph = scene(name).sphere.astype(np.float64)
    rng = np.random.default_rng(seed)
    bodies, lo, hi = scene_box(sph)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * 2.0
    o = (c + h * rng.uniform(-1.0, 1.0, (n, 3))).astype(F)
    b = bodies[rng.integers(0, len(bodies), n)]
    aim = sph[b, :3] + offset * np.abs(sph[b, 3:4]) * rng.uniform(-1.0, 1.0, (n, 3))
    to = aim - o.astype(np.float64)
    dist = np.linalg.norm(to, axis=1)
    length = np.exp2(rng.uniform(-6.0, 6.0, n))
    d = (to / dist[:, None] * length[:, None]).astype(F)
    t_min = np.where(rng.random(n) < 0.5, F(0.0), F(1e-3)).astype(F)
    t_max = np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.5, 1.5, n) * dist / length).astype(F)
    rays = make_rays(o, t_min, d, t_max)
    rays.setflags(write=False)
    return rays


def ref64(sph, rays, rel=1e-4, graze=1e-6):
    """hittable.clj:7-31 and raytracing.clj:33-43 in float64, in d units: per
    body a = d.d, h = d.oc, c = oc.oc - r^2, the roots (h -+ sqrt(disc)) / a,
    the first of them inside (t_min, t_max); the smallest over the bodies, the
    lowest index on ties.  Returns a dict: body, t, normal, front, len (|d|),
    reach (|oc| + |r| of the hit body) and marginal -- the rays whose answer in
    float64 is itself a close call: the two smallest roots within `rel`
    relative, a root within `rel` relative of t_min or t_max, or a body with
    |disc| < graze (h^2 + |a c|) whose chord lies where it could change the
    answer (it reaches above t_min and starts below the closest root and t_max).

    The grazing band is narrower than the 1e-4 (h^2 + |a c|) a test of this
    kind may leave out, and only bodies that matter count.  Among 484 small
    bodies the wide band is wider than a far body itself (for an impact
    parameter b it reads |r^2 - b^2| < 2e-4 |oc|^2: every b below r once
    |oc| > 70 r), and nine rays in ten pass one somewhere along their line.
    What the band has to cover is the fp32 test's error in disc: oc takes one
    rounding of 2^-24 per component, u = d / |d| about 1.5, h three more, c
    four, each relative to |oc| or |oc|^2 -- |d(disc)| <= about 1e-6 |oc|^2,
    which is 5e-7 (h^2 + |a c|) for a far body (h^2 + |a c| ~ 2 a |oc|^2), and
    a fifth of that when the roundings do not all pull one way.  graze = 1e-6
    is twice the bound, ten times the usual error; at 2e-6 the cover scene's
    rays no longer stay under the 2 % such a test may leave out (3.1 %)."""
    sph = np.asarray(sph, np.float64)
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    t_min, t_max = rays["t_min"].astype(np.float64)[:, None], rays["t_max"].astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        oc = sph[None, :, :3] - o[:, None, :]                      # (n, bodies, 3)
        a = (d * d).sum(axis=1)[:, None]
        h = (oc * d[:, None, :]).sum(axis=2)
        c = (oc * oc).sum(axis=2) - sph[None, :, 3] ** 2
        disc = h * h - a * c
        sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
        near, far = (h - sq) / a, (h + sq) / a

        def inside(t):
            return (t > t_min) & (t < t_max)

        root = np.where(inside(near), near, np.where(inside(far), far, np.inf))
        root = np.where(np.isnan(root), np.inf, root)
        body = root.argmin(axis=1)
        t = root[np.arange(len(rays)), body]
        hit = np.isfinite(t)
        body = np.where(hit, body, -1)
        # the close calls
        two = np.sort(root, axis=1)[:, :2] if root.shape[1] > 1 else np.concatenate([root, root + np.inf], axis=1)
        close_roots = np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] <= rel * np.abs(two[:, 1]))

        def near_bound(t, bound):
            return np.isfinite(t) & np.isfinite(bound) & (np.abs(t - bound) <= rel * np.maximum(np.abs(t), np.abs(bound)))

        at_bound = (near_bound(near, t_min) | near_bound(near, t_max) | near_bound(far, t_min) |
                    near_bound(far, t_max)).any(axis=1)
        reach_t = np.minimum(t[:, None], t_max)
        mid, half = h / a, np.sqrt(np.abs(disc)) / a
        matters = (mid + half > t_min) & (mid - half <= reach_t + rel * np.abs(reach_t))
        grazing = ((np.abs(disc) < graze * (h * h + np.abs(a * c))) & matters).any(axis=1)
        marginal = close_roots | at_bound | grazing
        # the record
        k = np.maximum(body, 0)
        centre, radius = sph[k, :3], sph[k, 3]
        p = o + t[:, None] * d
        normal = (p - centre) / radius[:, None]
        front = (d * normal).sum(axis=1) < 0
        normal = np.where(front[:, None], normal, -normal)
        reach = np.linalg.norm(centre - o, axis=1) + np.abs(radius)
    return dict(body=body, t=t, normal=normal, front=front, len=np.sqrt(a[:, 0]), reach=reach, marginal=marginal)


def inactive_rays():
    """One ray per inactive class of rt.h's step 2 (each would hit the
    reference scene's centre body from (0, 0, 1) along -z if it were active),
    with the class's name."""
    z = (0.0, 0.0, 1.0)
    dn = (0.0, 0.0, -1.0)
    nan = float("nan")
    inf = float("inf")
    cls = [("origin NaN", (nan, 0, 1), 0, dn, inf), ("origin +inf", (0, inf, 1), 0, dn, inf),
           ("origin -inf", (0, 0, -inf), 0, dn, inf), ("d zero", z, 0, (0, 0, 0), inf),
           ("d minus zero", z, 0, (-0.0, 0.0, -0.0), inf), ("d squared underflows", z, 0, (1e-30, 0, -1e-30), inf),
           ("d NaN", z, 0, (0, nan, -1), inf), ("d infinite", z, 0, (0, 0, -inf), inf),
           ("d squared overflows", z, 0, (0, 0, -3e19), inf), ("t_min NaN", z, nan, dn, inf),
           ("t_min negative", z, -1e-3, dn, inf), ("t_max NaN", z, 0, dn, nan), ("t_max == t_min", z, 1.0, dn, 1.0),
           ("t_max < t_min", z, 2.5, dn, 2.25), ("t_min infinite", z, inf, dn, inf), ("t_max zero", z, 0, dn, 0),
           ("t_max negative", z, 0, dn, -1.0)]
    with np.errstate(over="ignore", under="ignore"):
        rays = make_rays([c[1] for c in cls], [c[2] for c in cls], [c[3] for c in cls], [c[4] for c in cls])
    return [c[0] for c in cls], rays


def none_records(shape):
    from rtclj._lib import RAY_HIT_DTYPE
    out = np.zeros(shape, np.dtype(RAY_HIT_DTYPE))
    out["body"], out["t"], out["dist"] = -1, INF, INF
    return out


@functools.lru_cache(maxsize=None)
def guarded_rays(n=96, seed=7):
    """Rays that leave the reference scene's centre body (index 1, r = 0.5) from
    points float32 puts on its surface: even rays inward (a tilted -n), odd
    rays outward (+n), t_min = 0.  Returns (rays, last) with last = 1."""
    rng = np.random.default_rng(seed)
    sph = scene("reference").sphere.astype(np.float64)[1]
    v = rng.normal(size=(n, 3))
    nrm = v / np.linalg.norm(v, axis=1, keepdims=True)
    p = (sph[:3] + sph[3] * nrm).astype(F)
    inward = -nrm + 0.2 * np.roll(nrm, 1, axis=1)
    d = np.where((np.arange(n) % 2 == 0)[:, None], inward, nrm) * rng.uniform(0.5, 2.0, (n, 1))
    rays = make_rays(p, np.zeros(n), d, np.full(n, np.inf))
    last = np.ones(n, np.int32)
    rays.setflags(write=False)
    last.setflags(write=False)
    return rays, last


def words(a):
    """A record array (or any array) as its 32-bit words, one row per element."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.size, a.dtype.itemsize // 4)
