#!/usr/bin/env python3
"""What the ray queries (include/rt.h: rt_launch_rays, rt_launch_occluded;
DESIGN.md §3.16, §8.1) cost on C1's frame (cover scene grid 11, 1200 x 675 =
810,000 rays), beside the body-id pass they were derived from, in one process.
HIP events on one stream, the legs alternated within every round, medians over
the rounds; every leg is a batch of --batch calls between two events, so that
the window is not a single launch:

  ids            rt_launch_ids: the same walk, the ray made in registers, 4
                 bytes a pixel written
  rays           rt_launch_rays on rt_launch_ids' rays (pinhole_rays) in pixel
                 order: 32 bytes read and 32 written a ray
  rays_perm      the same rays in a fixed random permutation: neighbouring
                 lanes walk unrelated parts of the tree
  occ            rt_launch_occluded on the pixel-order rays, t_max = inf
  occ_perm       ... on the permuted rays
  occ_half       ... with t_max = half of each ray's own hit parameter (rays
                 that hit nothing keep inf): nearly every ray unoccluded, the
                 cull interval short
  occ_half_perm  ... permuted
  copy64         a device-to-device copy of 64 bytes a ray: the closest-hit
                 kernel's traffic

The expectation this checks: rays <= 1.5 x (ids + copy64).  Beside the times:
VGPRs, LDS and workgroups per CU of the closest-hit kernel per source
(rt_rays_occupancy).

  python tools/rays_time.py [--rounds 9] [--batch 50] [--json out.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-clj_amd"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rtclj import raytracing as R, scenes  # noqa: E402
from rtclj._lib import RAY_HIT_DTYPE, check, lib  # noqa: E402

SOURCES = {0: "tree in LDS", 1: "tree in global memory", 2: "linear scan"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    n = w * h
    sc = scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()

    rays = R.pinhole_rays(cam, w, h).reshape(-1)
    perm = np.random.default_rng(1).permutation(n)
    d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    d_occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_ids = torch.empty(n, dtype=torch.int32, device="cuda")
    d_rays = dev(rays)
    # each ray's own hit parameter, from the device (checked against the id pass below)
    check(lib.rt_launch_rays(ds, ptr(d_rays), None, n, ptr(d_hits), sp))
    check(lib.rt_launch_ids(ds, C.byref(cam), w, h, 0, ptr(d_ids), sp))
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy().view(np.dtype(RAY_HIT_DTYPE))
    assert np.array_equal(hits["body"], d_ids.cpu().numpy())
    half = rays.copy()
    half["t_max"] = np.where(hits["body"] >= 0, hits["t"] * np.float32(0.5), np.float32(np.inf))
    sets = {"order": d_rays, "perm": dev(rays[perm]), "half": dev(half), "half_perm": dev(half[perm])}
    copy_src = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for _ in range(a.batch):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def copy64():
        with torch.cuda.stream(s):
            copy_dst.copy_(copy_src, non_blocking=True)

    legs = {
        "ids": lambda: check(lib.rt_launch_ids(ds, C.byref(cam), w, h, 0, ptr(d_ids), sp)),
        "rays": lambda: check(lib.rt_launch_rays(ds, ptr(sets["order"]), None, n, ptr(d_hits), sp)),
        "rays_perm": lambda: check(lib.rt_launch_rays(ds, ptr(sets["perm"]), None, n, ptr(d_hits), sp)),
        "occ": lambda: check(lib.rt_launch_occluded(ds, ptr(sets["order"]), None, n, ptr(d_occ), sp)),
        "occ_perm": lambda: check(lib.rt_launch_occluded(ds, ptr(sets["perm"]), None, n, ptr(d_occ), sp)),
        "occ_half": lambda: check(lib.rt_launch_occluded(ds, ptr(sets["half"]), None, n, ptr(d_occ), sp)),
        "occ_half_perm": lambda: check(lib.rt_launch_occluded(ds, ptr(sets["half_perm"]), None, n, ptr(d_occ), sp)),
        "copy64": copy64,
    }
    for fn in legs.values():   # warm-up: the code objects
        timed(fn)
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(timed(legs[k]))
    # what the last legs left behind: the half-interval rays are nearly all unoccluded
    check(lib.rt_launch_occluded(ds, ptr(sets["half"]), None, n, ptr(d_occ), sp))
    torch.cuda.synchronize()
    occluded_half = float(d_occ.cpu().numpy().mean())
    occluded_inf = float((hits["body"] >= 0).mean())

    def stat(v):
        return {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}

    res = {"frame": [w, h], "rays": n, "bodies": len(sc), "rounds": a.rounds, "batch": a.batch,
           "occluded_share": {"t_max_inf": round(occluded_inf, 4), "t_max_half": round(occluded_half, 4)}, "kernels": {}}
    for k in legs:
        res[k] = stat(got[k])
    yard = res["ids"]["ms"] + res["copy64"]["ms"]
    res["rays"]["over_ids_plus_copy"] = round(res["rays"]["ms"] / yard, 4)
    res["rays"]["within_1.5x"] = bool(res["rays"]["ms"] <= 1.5 * yard)
    res["rays_perm"]["over_rays"] = round(res["rays_perm"]["ms"] / res["rays"]["ms"], 4)
    for k in ("occ", "occ_perm", "occ_half", "occ_half_perm"):
        res[k]["over_rays"] = round(res[k]["ms"] / res["rays_perm" if k.endswith("perm") else "rays"]["ms"], 4)
    res["copy64"]["gb_per_s"] = round(2 * 64 * n / (res["copy64"]["ms"] * 1e-3) / 1e9, 1)
    out4 = (C.c_int * 4)()
    for name, variant in (("default", 0), ("global", 12), ("scan", 5)):
        old = lib.rt_set_variant(variant)
        check(lib.rt_rays_occupancy(ds, out4))
        lib.rt_set_variant(old)
        res["kernels"][name] = {"workgroups_per_cu": out4[0], "vgprs": out4[1], "lds_bytes": out4[2],
                                "source": SOURCES[out4[3]]}
    us = lambda k: f"{res[k]['ms'] * 1e3:.1f}"   # noqa: E731
    print(f"{n} rays on {len(sc)} bodies: rt_launch_ids {us('ids')} us, copy of 64 B a ray {us('copy64')} us, "
          f"rt_launch_rays {us('rays')} us in pixel order ({res['rays']['over_ids_plus_copy']} x ids + copy), "
          f"{us('rays_perm')} us permuted ({res['rays_perm']['over_rays']} x)")
    print(f"rt_launch_occluded: t_max inf {us('occ')} us ({res['occ']['over_rays']} x rays), permuted {us('occ_perm')} us; "
          f"t_max half {us('occ_half')} us ({res['occ_half']['over_rays']} x), permuted {us('occ_half_perm')} us; "
          f"occluded {occluded_inf:.1%} / {occluded_half:.1%}")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
