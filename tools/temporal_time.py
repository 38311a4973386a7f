#!/usr/bin/env python3
"""What a step of temporal accumulation (include/rt.h, rt_temporal_step;
DESIGN.md §3.9, §8) costs on C1's frame (cover scene grid 11, 1200 x 675,
depth 50, seed 1), beside device-to-device copies of the bytes it moves, in
one process.

The step reads 56 bytes a pixel (two halves, the features), gathers up to
48 x 4 (three 16-byte history words a tap; neighbouring pixels share them, so
about 48 from memory) and writes 72 (three history words, two outputs): 176
bytes a pixel.  HIP events on one stream, the legs alternated within every
round, medians over the rounds; every leg is a batch of --batch calls between
two events, so that the window is not a single launch:

  moving    steps whose camera alternates between two cameras a few pixels
            apart (every step reprojects; the inputs are each camera's own)
  still     steps with one camera (every tap lands on its own pixel)
  copy176   a device-to-device copy of 176 bytes a pixel (the step's
            byte count as a copy's payload: it reads and writes that much)
  copy88    the same of 88 bytes a pixel (the step's byte count as a copy's
            traffic: 88 read + 88 written)

  python tools/temporal_time.py [--rounds 9] [--batch 200] [--json out.json]
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
from rtclj._lib import check, lib, rt_params  # noqa: E402

READ_BYTES, GATHER_BYTES, WRITE_BYTES = (3 + 3 + 8) * 4, 3 * 16, 3 * 16 + 2 * 3 * 4
STEP_BYTES = READ_BYTES + GATHER_BYTES + WRITE_BYTES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=200)
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
    # the inputs of either camera: two 4-spp halves of the frame's rays and the features of all 8
    half = [[torch.empty(n_px * 3, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in cams]
    feat = [torch.empty(n_px * 8, dtype=torch.float32, device="cuda") for _ in cams]
    for k, cam in enumerate(cams):
        for j in range(2):
            p4 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=4, max_depth=50, seed=1,
                           sample_begin=8 * k + 4 * j)
            check(lib.rt_launch(ds, C.byref(cam), C.byref(p4), ptr(half[k][j]), None, sp))
        p8 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=8, max_depth=50, seed=1, sample_begin=8 * k)
        check(lib.rt_feat_clear(ft, sp))
        check(lib.rt_launch_feat(ds, C.byref(cam), C.byref(p8), ft, None, sp))
        check(lib.rt_feat_resolve(ft, ptr(feat[k]), sp))
    out = [torch.full((n_px * 3,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    src = torch.zeros(n_px * STEP_BYTES, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n_px * STEP_BYTES, dtype=torch.uint8, device="cuda")
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

    def step(k):
        check(lib.rt_temporal_step(tp, None, C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]), ptr(feat[k]),
                                   ptr(out[0]), ptr(out[1]), sp))

    def copy(nbytes):
        a_, b_ = dst[:nbytes], src[:nbytes]

        def run(i):
            with torch.cuda.stream(s):
                a_.copy_(b_)        # (contiguous bytes: the runtime's device-to-device copy on the stream)
        return run

    legs = {"moving": lambda: timed(lambda i: step(i & 1)), "still": lambda: timed(lambda i: step(0)),
            "copy176": lambda: timed(copy(n_px * STEP_BYTES)), "copy88": lambda: timed(copy(n_px * STEP_BYTES // 2))}
    for fn in legs.values():   # warm-up: the code object, the copy's path, a built-up history
        fn()
        fn()
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(legs[k]())
    # how much history the moving steps found: the lengths after the last moving batch
    timed(lambda i: step(i & 1))
    length = (C.c_float * n_px)()
    check(lib.rt_temporal_read(tp, None, None, None, length, sp))
    accepted = sum(1 for v in length if v > 1.0) / n_px

    def stat(v):
        return {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}

    res = {"frame": [w, h], "bodies": len(sc), "rounds": a.rounds, "batch": a.batch,
           "bytes_per_pixel": {"read": READ_BYTES, "gathered": GATHER_BYTES, "written": WRITE_BYTES},
           "moving_accepted": round(accepted, 4)}
    for k in legs:
        res[k] = stat(got[k])
    for k in ("moving", "still"):
        res[k]["gb_per_s"] = round(STEP_BYTES * n_px / (res[k]["ms"] * 1e6), 1)
        res[k]["over_copy176"] = round(res[k]["ms"] / res["copy176"]["ms"], 3)
        res[k]["over_copy88"] = round(res[k]["ms"] / res["copy88"]["ms"], 3)
    print(f"rt_temporal_step on {w} x {h}: moving {res['moving']['ms'] * 1e3:.1f} us, still {res['still']['ms'] * 1e3:.1f} us "
          f"({STEP_BYTES} B a pixel: {res['moving']['gb_per_s']} GB/s moving); device copy of {STEP_BYTES} B a pixel "
          f"{res['copy176']['ms'] * 1e3:.1f} us, of {STEP_BYTES // 2} B a pixel {res['copy88']['ms'] * 1e3:.1f} us; "
          f"history accepted on {accepted:.1%} of the pixels under motion")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    lib.rt_temporal_free(tp)
    lib.rt_feat_free(ft)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
