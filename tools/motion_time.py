#!/usr/bin/env python3
"""What the moving-body entries (include/rt.h: rt_launch_ids,
rt_temporal_step_motion) cost on C1's frame (cover scene
grid 11, 1200 x 675, seed 1), beside the kernels they were derived from, in one
process.  HIP events on one stream, the legs alternated within every round,
medians over the rounds; every leg is a batch of --batch calls between two
events, so that the window is not a single launch:

  ids_lds      rt_launch_ids with the tree staged in LDS (rt_set_variant 16)
  ids_global   ... with the tree read from global memory (rt_set_variant 12)
  ids_default  ... under the default selector (whichever of the two it is)
  feat1        rt_launch_feat at spp = 1 on the same frame: the same walk plus
               the RNG, the shading and the atomics (its buffers are never
               cleared inside the window: the sums only grow)
  motion       rt_temporal_step_motion, the camera alternating between two a few
               pixels apart, ids from rt_launch_ids, a table in which every
               body moved a little
  blind        rt_temporal_step on the same inputs, in the same rounds

and, on the host, rt_scene_upload + rt_scene_free of the 484-body scene (the
three BVH builds a frame of an animation pays: nothing is refitted).  The
motion step reads 4 bytes a pixel more than the 176 of rt_temporal_step.
Beside the times: VGPRs, LDS and workgroups per CU of the id kernel per source
(rt_ids_occupancy).

  python tools/motion_time.py [--rounds 9] [--batch 100] [--json out.json]
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
from rtclj._lib import check, lib, rt_params  # noqa: E402

SOURCES = {0: "tree in LDS", 1: "tree in global memory", 2: "linear scan"}
STEP_BYTES = 176


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    n_px = w * h
    sc = scenes.cover(11, 42)
    cams = [scenes.cover_camera(w, h)]
    moved = R.rt_camera.from_buffer_copy(cams[0])
    for c in range(3):   # a few pixels sideways and a little forward (tools/temporal_time.py's pair)
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
    half = [[torch.empty(n_px * 3, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in cams]
    feat = [torch.empty(n_px * 8, dtype=torch.float32, device="cuda") for _ in cams]
    ids = [torch.full((n_px,), 0x7fffffff, dtype=torch.int32, device="cuda") for _ in cams]
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
    rng = np.random.default_rng(1)
    table = np.zeros((len(sc), 4), np.float32)
    table[:, :3] = rng.uniform(-0.01, 0.01, (len(sc), 3))      # every body a little: well under a pixel at the depths seen
    d_table = torch.from_numpy(table.reshape(-1)).cuda()
    d_scratch_ids = torch.empty(n_px, dtype=torch.int32, device="cuda")
    out = [torch.full((n_px * 3,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    check(lib.rt_feat_clear(ft, sp))
    tps = [C.c_void_p(), C.c_void_p()]
    for t in tps:
        check(lib.rt_temporal_create(0, w, h, 0, C.byref(t)))
    p1 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=1, max_depth=1, seed=1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for i in range(a.batch):
            fn(i)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def ids_leg(variant):
        def run():
            old = lib.rt_set_variant(variant)
            try:
                return timed(lambda i: check(lib.rt_launch_ids(ds, C.byref(cams[0]), w, h, 0, ptr(d_scratch_ids), sp)))
            finally:
                lib.rt_set_variant(old)
        return run

    def feat1(i):
        p1.sample_begin = i
        check(lib.rt_launch_feat(ds, C.byref(cams[0]), C.byref(p1), ft, None, sp))

    def motion(i):
        k = i & 1
        check(lib.rt_temporal_step_motion(tps[0], None, C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]), ptr(feat[k]),
                                          ptr(ids[k]), ptr(d_table), len(sc), ptr(out[0]), ptr(out[1]), sp))

    def blind(i):
        k = i & 1
        check(lib.rt_temporal_step(tps[1], None, C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]), ptr(feat[k]),
                                   ptr(out[0]), ptr(out[1]), sp))

    legs = {"ids_lds": ids_leg(16), "ids_global": ids_leg(12), "ids_default": ids_leg(0),
            "feat1": lambda: timed(feat1), "motion": lambda: timed(motion), "blind": lambda: timed(blind)}
    for fn in legs.values():   # warm-up: the code object, a built-up history
        fn()
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(legs[k]())
    assert torch.equal(d_scratch_ids, ids[0])
    length = (C.c_float * n_px)()
    check(lib.rt_temporal_read(tps[0], None, None, None, length, sp))
    accepted = float((np.frombuffer(length, np.float32) > 1.0).mean())

    # the host's share of an animation frame: upload (three BVH builds) + free
    up = []
    for _ in range(max(a.rounds, 5)):
        d2 = C.c_void_p()
        t0 = time.perf_counter()
        check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(d2)))
        check(lib.rt_scene_free(d2))
        up.append((time.perf_counter() - t0) * 1e3)

    def stat(v):
        return {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}

    res = {"frame": [w, h], "bodies": len(sc), "rounds": a.rounds, "batch": a.batch,
           "motion_accepted": round(accepted, 4), "upload_free_host": stat(up), "kernels": {}}
    for k in legs:
        res[k] = stat(got[k])
    res["motion"]["over_blind"] = round(res["motion"]["ms"] / res["blind"]["ms"], 4)
    res["motion"]["traffic_ratio"] = round((STEP_BYTES + 4) / STEP_BYTES, 4)
    res["blind"]["spread"] = round((res["blind"]["max"] - res["blind"]["min"]) / res["blind"]["ms"], 4)
    for k in ("ids_lds", "ids_global", "ids_default"):
        res[k]["over_feat1"] = round(res[k]["ms"] / res["feat1"]["ms"], 4)
    out4 = (C.c_int * 4)()
    for name, variant in (("default", 0), ("lds", 16), ("global", 12), ("scan", 5)):
        old = lib.rt_set_variant(variant)
        check(lib.rt_ids_occupancy(ds, out4))
        lib.rt_set_variant(old)
        res["kernels"][name] = {"workgroups_per_cu": out4[0], "vgprs": out4[1], "lds_bytes": out4[2],
                                "source": SOURCES[out4[3]]}
    print(f"rt_launch_ids on {w} x {h}: tree in LDS {res['ids_lds']['ms'] * 1e3:.1f} us, in global memory "
          f"{res['ids_global']['ms'] * 1e3:.1f} us, default ({res['kernels']['default']['source']}) "
          f"{res['ids_default']['ms'] * 1e3:.1f} us; rt_launch_feat at 1 spp {res['feat1']['ms'] * 1e3:.1f} us")
    print(f"rt_temporal_step_motion {res['motion']['ms'] * 1e3:.1f} us, rt_temporal_step {res['blind']['ms'] * 1e3:.1f} us "
          f"(ratio {res['motion']['over_blind']}, traffic {res['motion']['traffic_ratio']}, the blind step's spread "
          f"{res['blind']['spread']:.1%}); history accepted on {accepted:.1%}; upload + free {res['upload_free_host']['ms']:.2f} ms")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    for t in tps:
        lib.rt_temporal_free(t)
    lib.rt_feat_free(ft)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
