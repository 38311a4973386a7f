#!/usr/bin/env python3
"""What the colour clamp adds to a step of temporal accumulation (include/rt.h,
rt_temporal_step_clamp) on C1's frame (cover scene grid
11, 1200 x 675, depth 50, seed 1): the clamped step -- the box kernel and the
step kernel -- beside rt_temporal_step_motion on the same inputs, in one
process.

The box kernel reads 40 bytes a pixel (two halves, four guide floats; the halo
again from the caches) and writes 32; the clamped step kernel reads those 32
on top of the motion step's 180.  HIP events on one stream, the legs alternated
within every round, medians over the rounds; every leg is a batch of --batch
calls between two events, so that the window is not a single launch.  The
camera alternates between two cameras a few pixels apart (every step
reprojects; the inputs are each camera's own); the ids are each camera's, the
displacement table is zero (the scene is still):

  motion    rt_temporal_step_motion
  clamp1    rt_temporal_step_clamp with the ids, radius 1 (3 x 3 window)
  clamp2    ... radius 2 (5 x 5, the default)
  clamp3    ... radius 3 (7 x 7)

  python tools/clamp_time.py [--rounds 9] [--batch 200] [--json out.json]
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

import torch  # noqa: E402

from rtclj import raytracing as R, scenes  # noqa: E402
from rtclj._lib import check, lib, rt_params, rt_temporal_clamp_opts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    n_px = w * h
    sc = scenes.cover(11, 42)
    cams = [scenes.cover_camera(w, h)]
    moved = R.rt_camera.from_buffer_copy(cams[0])
    for c in range(3):   # a few pixels sideways and a little forward
        moved.center[c] += 3.3 * cams[0].du[c] + 0.002 * (cams[0].p00[c] - cams[0].center[c])
        moved.p00[c] += 3.3 * cams[0].du[c] + 0.002 * (cams[0].p00[c] - cams[0].center[c])
    cams.append(moved)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ds, ft = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    shape = rt_params(width=w, height=h, row_begin=0, row_end=h)
    check(lib.rt_feat_create(ds, C.byref(shape), C.byref(ft)))
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    # the inputs of either camera: two 4-spp halves of the frame's rays, the features of all 8, the ids
    half = [[torch.empty(n_px * 3, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in cams]
    feat = [torch.empty(n_px * 8, dtype=torch.float32, device="cuda") for _ in cams]
    ids = [torch.empty(n_px, dtype=torch.int32, device="cuda") for _ in cams]
    motion = torch.zeros(len(sc) * 4, dtype=torch.float32, device="cuda")
    for k, cam in enumerate(cams):
        for j in range(2):
            p4 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=4, max_depth=50, seed=1,
                           sample_begin=8 * k + 4 * j)
            check(lib.rt_launch(ds, C.byref(cam), C.byref(p4), ptr(half[k][j]), None, sp))
        p8 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=8, max_depth=50, seed=1, sample_begin=8 * k)
        check(lib.rt_feat_clear(ft, sp))
        check(lib.rt_launch_feat(ds, C.byref(cam), C.byref(p8), ft, None, sp))
        check(lib.rt_feat_resolve(ft, ptr(feat[k]), sp))
        check(lib.rt_launch_ids(ds, C.byref(cam), w, h, 0, ptr(ids[k]), sp))
    out = [torch.full((n_px * 3,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    tp = C.c_void_p()
    check(lib.rt_temporal_create(0, w, h, 0, C.byref(tp)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for i in range(a.batch):
            fn(i)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def motion_step(k):
        check(lib.rt_temporal_step_motion(tp, None, C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]), ptr(feat[k]),
                                          ptr(ids[k]), ptr(motion), len(sc), ptr(out[0]), ptr(out[1]), sp))

    def clamp_step(radius):
        ko = rt_temporal_clamp_opts(radius=radius, gamma=a.gamma)

        def run(k):
            check(lib.rt_temporal_step_clamp(tp, None, C.byref(ko), C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]),
                                             ptr(feat[k]), ptr(ids[k]), ptr(motion), len(sc), ptr(out[0]), ptr(out[1]), sp))
        return run

    legs = {"motion": lambda: timed(lambda i: motion_step(i & 1))}
    for radius in (1, 2, 3):
        legs[f"clamp{radius}"] = (lambda run: lambda: timed(lambda i: run(i & 1)))(clamp_step(radius))
    for fn in legs.values():   # warm-up: the code object, the box scratch, a built-up history
        fn()
        fn()
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(legs[k]())
    # how much history the clamped steps found: the lengths after the last batch
    length = (C.c_float * n_px)()
    check(lib.rt_temporal_read(tp, None, None, None, length, sp))
    accepted = sum(1 for v in length if v > 1.0) / n_px

    def stat(v):
        return {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}

    res = {"frame": [w, h], "bodies": len(sc), "rounds": a.rounds, "batch": a.batch, "gamma": a.gamma,
           "accepted": round(accepted, 4)}
    for k in legs:
        res[k] = stat(got[k])
    for radius in (1, 2, 3):
        res[f"clamp{radius}"]["over_motion"] = round(res[f"clamp{radius}"]["ms"] / res["motion"]["ms"], 3)
    print(f"on {w} x {h}: rt_temporal_step_motion {res['motion']['ms'] * 1e3:.1f} us; rt_temporal_step_clamp (box + step) "
          + ", ".join(f"radius {r} {res[f'clamp{r}']['ms'] * 1e3:.1f} us" for r in (1, 2, 3))
          + f"; history accepted on {accepted:.1%} of the pixels")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    lib.rt_temporal_free(tp)
    lib.rt_feat_free(ft)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
