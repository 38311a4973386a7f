#!/usr/bin/env python3
"""What rt_scene_update (include/rt.h) costs beside the
fresh upload it replaces, and what a refitted tree costs the trace kernel as it
loosens, in one process.  The legs are alternated within every round, medians
over the rounds with their ranges.

1. The update, for C1's 484-body scene (cover grid 11) and cover(16)'s 1025:

  update_host    the host time of one rt_scene_update call (the checks, the
                 tree centre and radius, the copy to the staging, two enqueues),
                 the stream idle before every call
  update_stream  a batch of --batch updates between two HIP events on one
                 stream: the copy to the device and the refit kernel, per
                 update (the host keeps four in flight, so this is the device's
                 time unless the host is slower: then it is an upper bound)
  upload_free    rt_scene_upload + rt_scene_free of the same spheres on the host
                 clock: three tree builds, seven allocations, synchronous copies
                 -- what a frame of an animation paid before

2. The loosened tree, on C1's frame (1200 x 675, --spp samples): the small
   spheres scattered in x and z by a uniform draw of growing amplitude; the
   frame traced on the refitted scene and on a scene freshly uploaded from the
   same spheres (bit-equal: checked), beside the 4-body tree's
   rt_tree_cost_host now / at the upload.  Where refit / rebuilt crosses
   1 + upload_free / trace is where a fresh upload pays.

  python tools/refit_time.py [--rounds 9] [--batch 50] [--json out.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-clj_amd"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rtclj import raytracing as R, scenes  # noqa: E402
from rtclj._lib import check, fptr, lib, rt_params  # noqa: E402

AMPLITUDES = (0.0, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2)


def stat(v):
    return {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def scattered(sc, amp, seed=1):
    """The small spheres (radius 0.2) moved in x and z by up to +-amp."""
    sph = sc.sphere.copy()
    small = sph[:, 3] < 0.5
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, (int(small.sum()), 2)).astype(np.float32) * np.float32(amp)
    sph[small, 0] += d[:, 0]
    sph[small, 2] += d[:, 1]
    return sph


def update_cost(sc, a, s):
    sp = C.c_void_p(s.cuda_stream)
    moved = [scattered(sc, 0.1, seed) for seed in (1, 2)]

    def host_leg():
        total = 0.0
        with R.DeviceScene(sc) as d:
            check(lib.rt_scene_update(d.handle, fptr(moved[0]), sp))   # (the first update's allocations)
            for i in range(a.batch):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                check(lib.rt_scene_update(d.handle, fptr(moved[i & 1]), sp))
                total += time.perf_counter() - t0
            torch.cuda.synchronize()
        return total * 1e3 / a.batch

    def stream_leg():
        with R.DeviceScene(sc) as d:
            check(lib.rt_scene_update(d.handle, fptr(moved[0]), sp))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(s)
            for i in range(a.batch):
                check(lib.rt_scene_update(d.handle, fptr(moved[i & 1]), sp))
            e1.record(s)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.batch

    def upload_leg():
        total = 0.0
        n = max(a.batch // 5, 5)
        for i in range(n):
            sc2 = R.Scene(moved[i & 1], sc.kind, sc.mat)
            d2 = C.c_void_p()
            t0 = time.perf_counter()
            check(lib.rt_scene_upload(0, C.byref(sc2.c), C.byref(d2)))
            check(lib.rt_scene_free(d2))
            total += time.perf_counter() - t0
        return total * 1e3 / n

    legs = {"update_host": host_leg, "update_stream": stream_leg, "upload_free": upload_leg}
    for fn in legs.values():
        fn()
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            got[k].append(legs[k]())
    res = {k: stat(v) for k, v in got.items()}
    res["bodies"] = len(sc)
    res["nodes"] = [R.tree_build_host(sc, k)[0].n_nodes for k in range(3)]
    res["upload_over_update"] = round(res["upload_free"]["ms"] / max(res["update_host"]["ms"], res["update_stream"]["ms"]), 2)
    return res


def loosened(sc, a, s):
    w = a.width
    h = R.image_height(w)
    cam = scenes.cover_camera(w, h)
    sp = C.c_void_p(s.cuda_stream)
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=a.spp, max_depth=50, seed=1)
    out = [torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    info0, blob0 = R.tree_build_host(sc, 1)
    cost0 = R.tree_cost(info0, blob0)
    rows = []
    batch = max(a.batch // 5, 5)
    for amp in AMPLITUDES:
        sph = scattered(sc, amp)
        with R.DeviceScene(sc) as refit, R.DeviceScene(R.Scene(sph, sc.kind, sc.mat)) as fresh:
            refit.update(sph, stream=s.cuda_stream)
            cost = R.tree_cost(*refit.tree(1, stream=s.cuda_stream))
            handles = (refit.handle, fresh.handle)

            def leg(k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s)
                for _ in range(batch):
                    check(lib.rt_launch(handles[k], C.byref(cam), C.byref(p), C.c_void_p(out[k].data_ptr()), None, sp))
                e1.record(s)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / batch

            leg(0), leg(1)   # warm-up: the adaptive order of either scene
            assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), amp
            got = ([], [])
            for r in range(a.rounds):
                for k in ((0, 1) if r % 2 == 0 else (1, 0)):
                    got[k].append(leg(k))
        row = {"amplitude": amp, "cost_ratio": round(cost / cost0, 4), "refit": stat(got[0]), "rebuilt": stat(got[1])}
        row["refit_over_rebuilt"] = round(row["refit"]["ms"] / row["rebuilt"]["ms"], 4)
        rows.append(row)
    return {"frame": [w, h], "spp": a.spp, "tree": "4-body", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    s = torch.cuda.Stream()
    res = {"rounds": a.rounds, "batch": a.batch, "update": {}}
    for name, sc in (("c1_cover11", scenes.cover(11, 42)), ("cover16", scenes.cover(16, 42))):
        res["update"][name] = u = update_cost(sc, a, s)
        print(f"{name} ({u['bodies']} bodies): rt_scene_update host {u['update_host']['ms'] * 1e3:.1f} us "
              f"[{u['update_host']['min'] * 1e3:.1f}, {u['update_host']['max'] * 1e3:.1f}], on the stream "
              f"{u['update_stream']['ms'] * 1e3:.1f} us [{u['update_stream']['min'] * 1e3:.1f}, "
              f"{u['update_stream']['max'] * 1e3:.1f}]; upload + free {u['upload_free']['ms']:.3f} ms "
              f"[{u['upload_free']['min']:.3f}, {u['upload_free']['max']:.3f}]: x{u['upload_over_update']}")
    res["loosened"] = lo = loosened(scenes.cover(11, 42), a, s)
    for row in lo["rows"]:
        print(f"amplitude {row['amplitude']:<5} cost x{row['cost_ratio']:<8} refit {row['refit']['ms']:.4f} ms "
              f"[{row['refit']['min']:.4f}, {row['refit']['max']:.4f}]  rebuilt {row['rebuilt']['ms']:.4f} ms "
              f"[{row['rebuilt']['min']:.4f}, {row['rebuilt']['max']:.4f}]  ratio {row['refit_over_rebuilt']}")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
