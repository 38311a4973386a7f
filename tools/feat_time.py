#!/usr/bin/env python3
"""What a first-hit feature pass (include/rt.h, rt_feat)
costs beside the path kernel, on C1's frame (cover scene grid 11, 1200 x 675,
depth 50, seed 1), in one process.

For every spp (default 4, 16, 100), HIP events on one stream, the legs
alternated within every round, medians over the rounds:

  feat      one rt_launch_feat pass of the spp into cleared buffers (the clear
            outside the window)
  launch    one rt_launch of the spp, beside it
  resolve   rt_feat_resolve alone

and each kernel's time per traced segment, the segments taken from the
launches' own d_counters: the feature pass traces one per sample, the path
kernel as many as its paths are long.  The yardstick for the walk is the path
kernel's time per segment in the same run; the ratio is reported.  Beside
them the feature kernel's VGPRs, LDS bytes and workgroups per CU, and where it
read the bodies (rt_feat_occupancy), for the default selector and for
rt_set_variant 12 (the tree in global memory) and 5 (the linear scan).

  python tools/feat_time.py [--spp 4 16 100] [--rounds 7] [--json out.json]
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

SOURCES = {0: "tree in LDS", 1: "tree in global memory", 2: "linear scan"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, nargs="+", default=[4, 16, 100])
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    sc = scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ds, ft = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    shape = rt_params(width=w, height=h, row_begin=0, row_end=h)
    check(lib.rt_feat_create(ds, C.byref(shape), C.byref(ft)))
    out = torch.empty(h * w * 3, dtype=torch.float32, device="cuda")
    feat = torch.empty(h * w * 8, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    cp = C.c_void_p(cnt.data_ptr())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cnt.zero_()
        torch.cuda.synchronize()
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), cnt.cpu().tolist()

    def feat_pass(p):
        check(lib.rt_feat_clear(ft, sp))
        torch.cuda.synchronize()
        return timed(lambda: check(lib.rt_launch_feat(ds, C.byref(cam), C.byref(p), ft, cp, sp)))

    def launch(p):
        return timed(lambda: check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), cp, sp)))

    def resolve(p):
        return timed(lambda: check(lib.rt_feat_resolve(ft, C.c_void_p(feat.data_ptr()), sp)))

    def occupancy():
        out4 = (C.c_int * 4)()
        check(lib.rt_feat_occupancy(ds, out4))
        return {"workgroups_per_cu": out4[0], "vgprs": out4[1], "lds_bytes": out4[2], "source": SOURCES[out4[3]]}

    res = {"frame": [w, h], "bodies": len(sc), "rounds": a.rounds, "kernel": occupancy(), "spp": {}}
    occ4 = (C.c_int * 4)()
    check(lib.rt_launch_occupancy(ds, C.byref(rt_params(width=w, height=h, row_begin=0, row_end=h, spp=a.spp[-1],
                                                        max_depth=50, seed=1)), occ4))
    res["path_kernel"] = {"workgroups_per_cu": occ4[0], "vgprs": occ4[1], "lds_bytes": occ4[2], "variant": occ4[3]}
    legs = {"feat": feat_pass, "launch": launch, "resolve": resolve}
    for spp in a.spp:
        p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=50, seed=1)
        for fn in legs.values():   # warm-up: code objects, the schedule's first order
            fn(p)
            fn(p)
        ms = {k: [] for k in legs}
        segs = {}
        for r in range(a.rounds):
            order = list(legs) if r % 2 == 0 else list(legs)[::-1]   # alternated
            for k in order:
                t, c = legs[k](p)
                ms[k].append(t)
                segs[k] = c[0]
        row = {}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"ms": round(med, 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)}
            if k != "resolve":
                row[k]["segments"] = segs[k]
                row[k]["ns_per_segment"] = round(med * 1e6 / segs[k], 4)
        row["segment_cost_ratio"] = round(row["feat"]["ns_per_segment"] / row["launch"]["ns_per_segment"], 3)
        res["spp"][spp] = row
        print(f"{spp:4d} spp: feat {row['feat']['ms']:.3f} ms ({row['feat']['ns_per_segment']:.4f} ns/segment), "
              f"launch {row['launch']['ms']:.3f} ms ({row['launch']['ns_per_segment']:.4f} ns/segment), "
              f"ratio {row['segment_cost_ratio']:.2f}, resolve {row['resolve']['ms']:.3f} ms")
    # the other two sources, at the first spp
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=a.spp[0], max_depth=50, seed=1)
    res["sources"] = {}
    for v in (0, 12, 5):
        old = lib.rt_set_variant(v)
        try:
            feat_pass(p)
            t = [feat_pass(p)[0] for _ in range(a.rounds)]
            res["sources"][v] = dict(occupancy(), spp=a.spp[0], ms=round(statistics.median(t), 4))
        finally:
            lib.rt_set_variant(old)
        print(f"rt_set_variant({v}): {res['sources'][v]}")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    lib.rt_feat_free(ft)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
