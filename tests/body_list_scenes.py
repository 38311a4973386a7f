"""Scenes for the camera prelude's body list (tests/test_gpu_body_list.py,
tests/test_tile_bodies_host.py, tests/test_gpu_list_modes.py): frames of a few
8 x 8 tiles in which tile t's list holds t bodies, as rt_tile_bodies_host
(include/rt.h) counts them.

A ground and a mirror ball (the big bodies: the walk's first leaves) under a
pinhole camera pitched up, so that the top row of tiles sees the sky alone;
then per tile as many small spheres as it lacks to t, set along the camera rays
through the tile's middle pixels, each about a pixel across at its depth.  The
first two of a tile coincide (one centre, one radius, two materials: a tie that
the lower index wins, and the list pass's repeated slot in earnest).

compact: a tile's spheres lie one behind the other in a short stretch of depth,
the same for every tile, so the tree's leaves gather a tile's own spheres (a
list out of one record, or two).  scattered: they are spread over the whole
depth, so a leaf gathers neighbouring tiles' spheres of one depth (a list out
of five records and more).
"""
import ctypes as C

import numpy as np


def camera(w, h, defocus_angle=0.0):
    from rtclj import raytracing as R
    return R.camera(w, h, 20.0, (13.0, 2.0, 3.0), (0.0, 2.6, 0.0), (0.0, 1.0, 0.0), defocus_angle, 10.0)


def params(w, h, **kw):
    from rtclj._lib import rt_params
    kw.setdefault("spp", 1)
    kw.setdefault("max_depth", 6)
    return rt_params(width=w, height=h, row_begin=0, row_end=h, seed=1, **kw)


def tile_lists(sc, cam, p, rows=None):
    """[(bodies, slots)] per 8 x 8 tile of the launch (rt_tile_bodies_host)."""
    from rtclj import raytracing as R
    rows = p.height if rows is None else rows
    n = ((p.width + 7) // 8) * ((rows + 7) // 8)
    return [R.tile_bodies_host(sc, cam, p, t) for t in range(n)]


def _big():
    from rtclj import raytracing as R
    return ([(0.0, -1000.0, 0.0, 1000.0), (0.0, 1.0, 0.0, 1.0)], [R.RT_LAMBERTIAN, R.RT_METAL],
            [(0.5, 0.5, 0.5, 0.0), (0.7, 0.6, 0.5, 0.0)])


def _scene(sph, kind, mat):
    from rtclj import raytracing as R
    return R.Scene(np.array(sph, np.float32), np.array(kind, np.int32), np.array(mat, np.float32))


def staircase(w, h, scattered=False, first=0, aims=None):
    """-> (scene, camera): tile t aims at first + t listed bodies, or at aims[t]."""
    from rtclj import raytracing as R
    cam = camera(w, h)
    sph, kind, mat = _big()
    have = [len(b) for b, _ in tile_lists(_scene(sph, kind, mat), cam, params(w, h))]
    c, p00, du, dv = (np.array(v[:], np.float64) for v in (cam.center, cam.p00, cam.du, cam.dv))
    px = float(np.linalg.norm(du))   # a pixel's width on the focus plane (s = 1)
    tiles_x = (w + 7) // 8
    stair = [(-1, 0.0, 0.0, 0.0)] * len(sph)   # per body: its tile (-1: a big body), fx, fy, s
    for t, b in enumerate(have):
        x0, y0 = 8 * (t % tiles_x), 8 * (t // tiles_x)
        vw, vh = min(8, w - x0), min(8, h - y0)
        for k in range(max(0, (first + t if aims is None else aims[t]) - b)):
            kk = 0 if k == 1 else k   # (the second coincides with the first)
            fx = x0 + (vw - 1) / 2 + ((kk % 4) - 1.5) * min(1.0, (vw - 1) / 6)
            fy = y0 + (vh - 1) / 2 + (((kk // 4) % 4) - 1.5) * min(1.0, (vh - 1) / 6)
            s = (0.08 + 0.8 * ((kk * 7 + 3 * t) % 16) / 16) if scattered else 0.30 + 0.01 * kk
            pt = c + s * (p00 + fx * du + fy * dv - c)
            sph.append((pt[0], pt[1], pt[2], 0.45 * px * s))
            kind.append((R.RT_LAMBERTIAN, R.RT_METAL, R.RT_DIELECTRIC)[k % 3])
            mat.append(((0.8, 0.3, 0.3, 0.0), (0.7, 0.7, 0.9, 0.1), (0.0, 0.0, 0.0, 1.5))[k % 3])
            stair.append((t, fx, fy, s))
    sc = _scene(sph, kind, mat)
    sc.stair = dict(w=w, h=h, body=np.array(stair, np.float64))   # (what moved() needs)
    return sc, cam


# the frames of the GPU cases: 40 x 24 (15 whole tiles), 44 x 27 (24 tiles, the
# last column 4 pixels wide, the last row 3 high)
FRAMES = {"40x24": (40, 24, False, 0), "44x27": (44, 27, True, 0)}


# The launch-mode cases (tests/test_gpu_list_modes.py) want nearly every tile of
# a frame with partial tiles listed.  In "44x27" the spheres of a partial tile
# stand within three pixels of the neighbouring whole tile and enter its list
# too, so only ten of its tiles list 1 .. 14 bodies.  "44x27m" is the same frame
# with an aim per tile: small lists in the partial tiles (last column, last
# row), the exact lengths 0, 1, 2, 5, 9, 11, 13, 14 in the whole tiles that touch
# no partial one, and the overflow in the third row and the last row's end.
MODE_AIMS = {"44x27m": (44, 27, True, (0, 1, 2, 5, 3, 1,
                                      9, 11, 13, 14, 6, 2,
                                      20, 20, 20, 20, 20, 8,
                                      3, 4, 7, 16, 16, 16))}
MODE_FRAMES = ("40x24", "44x27m")


def frame(name):
    if name in MODE_AIMS:
        w, h, scattered, aims = MODE_AIMS[name]
        sc, cam = staircase(w, h, scattered, aims=aims)
        return sc, cam, w, h
    w, h, scattered, first = FRAMES[name]
    sc, cam = staircase(w, h, scattered, first)
    return sc, cam, w, h


def listed_tiles(sc, cam, p):
    """The tiles of the launch whose camera segments take the list: at most 14 bodies."""
    return [t for t, (b, _) in enumerate(tile_lists(sc, cam, p)) if len(b) <= 14]


def moved_tiles(sc, k):
    """The tiles whose small spheres moved(sc, k) displaces: every third, from k % 3."""
    tiles = sorted({int(t) for t in sc.stair["body"][:, 0] if t >= 0})
    return [t for t in tiles if t % 3 == k % 3]


def moved(sc, k):
    """A copy of a staircase scene in which the small spheres of every third
    tile (t % 3 == k % 3) stand 8 pixels' width farther along their tile's row,
    at their own depth: staircase's point with fx + 8 for fx.  They leave their
    tile's list and enter the next one's (from a row's last tile they leave the
    frame).  The big bodies stay, and so do radii, kinds and materials:
    rt_scene_update's condition."""
    w, h = sc.stair["w"], sc.stair["h"]
    cam = camera(w, h)
    c, p00, du, dv = (np.array(v[:], np.float64) for v in (cam.center, cam.p00, cam.du, cam.dv))
    sph = sc.sphere.copy()
    for i, (t, fx, fy, s) in enumerate(sc.stair["body"]):
        if t >= 0 and int(t) % 3 == k % 3:
            pt = c + s * (p00 + (fx + 8.0) * du + fy * dv - c)
            sph[i, :3] = pt
    out = _scene(sph, sc.kind, sc.mat)
    out.stair = sc.stair
    return out


def describe(lists):
    """What the tiles' lists hold, for the coverage assertions: the counts that
    occur; whether some listed tile (2 .. 14 bodies) has them all in one
    record, in two records at differing slots, in five records or more."""
    counts = sorted({len(b) for b, _ in lists})
    recs = [(len(b), sorted({int(s) >> 2 for s in sl}), sorted({int(s) & 3 for s in sl})) for b, sl in lists]
    listed = [r for r in recs if 2 <= r[0] <= 14]
    return {"counts": counts,
            "one_record": any(len(r[1]) == 1 for r in listed),
            "two_records": any(len(r[1]) == 2 and len(r[2]) >= 2 for r in listed),
            "five_records": any(len(r[1]) >= 5 for r in listed),
            "overflow": any(r[0] >= 15 for r in recs)}
