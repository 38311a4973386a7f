#!/usr/bin/env python3
"""The statistics build of variant 22 (variant 31, the diagnostic library) on
the C1 frame: one warm-up launch, one counted launch, and the wave-level events
per segment call -- the walk's and the prelude's (rt_debug_stats_ext 27-32:
prelude trips, lanes in them, their list passes and per-body exact steps, walk
segments entered in an iteration that ran a trip, the bodies the list passes
tested: four or two a pass).  Under the tile list a wave
iteration is a walk segment, a prelude trip or both, shaded in one tail; a walk
and a trip are each one search of the segment's text and one count of
rt_debug_stats[0]; the rates below are per such call.

Prints one JSON line in the shape of a bench.py --full line's stats_build, so
that tools/isa_blocks.py --bench reads it:

  python tools/prelude_stats.py [--width 1200 --spp 100 --depth 50] > line.json
  python tools/isa_blocks.py --bench line.json
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-clj_amd"))

import torch  # noqa: E402  (before the library: torch's HIP runtime must serve the process)

from rtclj import raytracing as R, scenes  # noqa: E402
from rtclj._lib import check, diag_lib, load, rt_params  # noqa: E402

STATS = 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--grid", type=int, default=11)
    ap.add_argument("--library", default=None, help="another build of the diagnostic library (A/B of builds)")
    a = ap.parse_args()
    lib = load(Path(a.library).resolve()) if a.library else diag_lib()
    w, h = a.width, R.image_height(a.width)
    sc, cam = scenes.cover(a.grid), scenes.cover_camera(w, h)
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    old = lib.rt_set_variant(STATS)
    assert old >= 0, "the diagnostic library lacks variant 31"
    try:
        p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=a.spp, max_depth=a.depth, seed=1)
        occ = (C.c_int * 4)()
        check(lib.rt_launch_occupancy(ds, C.byref(p), occ))
        assert occ[3] == STATS, f"the launch runs variant {occ[3]}, not {STATS}"
        out = torch.empty(h * w * 3, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream()
        d = (C.c_uint64 * 40)()
        for timed in (False, True):
            cnt.zero_()
            check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                C.c_void_p(s.cuda_stream)))
            torch.cuda.synchronize()
            # (the warm-up's counts read and cleared; a build from before the list
            # passes has 32 counters)
            check(lib.rt_debug_stats_ext(d, 40) if hasattr(lib, "rt_debug_stats_ext") else lib.rt_debug_stats(d))
        segs, smp = (float(x) for x in cnt.cpu().tolist())
    finally:
        lib.rt_set_variant(old)
        lib.rt_scene_free(ds)
    d = [int(x) for x in d]
    wi = max(d[0], 1)
    trips = d[27]
    pw = {"wave_iters_per_sample": wi / smp, "lanes_active": d[1] / wi / 64.0,
          "fresh_blocks": d[16] / wi, "fresh_lanes": d[17] / max(d[16], 1),
          "random_unit_trips": d[14] / wi, "disk_trips": d[15] / wi,
          "dielectric_blocks": d[19] / wi, "dielectric_lanes": d[20] / max(d[19], 1),
          "lambert_metal_blocks": d[21] / wi, "lambert_metal_lanes": d[22] / max(d[21], 1),
          "sums_blocks": d[23] / wi, "refills": d[24] / wi, "claims": d[25] / wi, "drain_checks": d[26] / wi,
          "trav_steps": d[6] / wi, "trav_lane_eff": d[7] / max(d[6], 1) / 64.0,
          "leaf_passes": d[12] / wi, "exact_passes": d[13] / wi,
          "prelude_trips": trips / wi, "prelude_lanes": d[28] / max(trips, 1),
          "prelude_leaf_passes": d[29] / wi, "prelude_exact_passes": d[30] / wi,
          "prelude_bodies_tested": d[32] / wi,
          "walk_segments": (wi - trips) / wi, "walk_segments_after_a_trip": d[31] / wi,
          "wave_iterations": (wi - d[31]) / wi}
    line = {"workload": f"cover({a.grid}) {w}x{h} spp {a.spp} depth {a.depth}", "segments": segs, "samples": smp,
            "occupancy": list(occ), "raw": d,
            "prelude": {"trips_per_sample": trips / smp, "lanes_per_trip": d[28] / max(trips, 1),
                        "leaf_passes_per_trip": d[29] / max(trips, 1), "exact_passes_per_trip": d[30] / max(trips, 1),
                        "bodies_tested_per_trip": d[32] / max(trips, 1),
                        "walk_segments_per_sample": (wi - trips) / smp,
                        "share_of_walk_segments_after_a_trip": d[31] / max(wi - trips, 1)},
            "stats_build": {"stats_variant": STATS, "flops_per_segment": d[18] / segs, "segments_per_sample": segs / smp,
                            "nodes": d[2] / segs, "leaf_pairs": 2 * d[3] / segs, "exact_tests": d[4] / segs,
                            "per_wave_iter": pw}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
