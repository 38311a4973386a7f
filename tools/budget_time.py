#!/usr/bin/env python3
"""What the sample budget costs and saves (include/rt.h, rt_temporal_probe,
rt_budget_*, rt_temporal_step_budget) on C1's frame
(cover scene grid 11, 1200 x 675, depth 50, seed 1), in one process.

Kernel legs: HIP events on one stream, the legs alternated within every round,
medians over the rounds; every leg is a batch of --batch calls between two
events.  The camera alternates between two cameras a few pixels apart, as
tools/clamp_time.py's:

  motion    rt_temporal_step_motion                     (the yardstick)
  probe     rt_temporal_probe with the ids
  plan      rt_budget_plan: the zeroing of H0 and H1, the plan and the list
            kernel, the 128-byte read-back's copy
  clamp2    rt_temporal_step_clamp with the ids, radius 2
  budget    rt_temporal_step_budget, the same with a multiplier per tile

Frame legs: wall clock from the first call to the end of the stream, because
rt_budget_trace waits for its plan's read-back on the host.  For a share d of
the tiles -- a rectangle in the middle of the frame -- planned at max_mult = 8
and the rest at 1 (rt_budget_plan_mult), half_spp = 4:

  budget[d]   rt_budget_plan_mult + rt_budget_trace (up to 16 launches)
  fused[d]    rt_budget_plan_mult + rt_budget_trace_fused (the table kernel and 2
              launches), on the same rt_budget in the same rounds
  uniform[d]  two rt_launch_accum passes of the same total samples, spread evenly
              (the smallest even spp at or above the budgeted frame's mean)
  full        two rt_launch_accum passes at 8 x the base rate: what bringing the
              short pixels to the same count costs without a plan

budget_units_kernel alone is a kernel inside rt_budget_trace_fused; its time
comes from a kernel trace of a short run, in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o prof -- \
      python tools/budget_time.py --rounds 1 --batch 2 --frames 3

  python tools/budget_time.py [--rounds 9] [--batch 100] [--frames 20] [--json out.json]
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
from rtclj._lib import check, lib, rt_budget_opts, rt_params, rt_temporal_clamp_opts  # noqa: E402

SHARES = (0.0, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
HALF_SPP, MAX_MULT = 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    n_px = w * h
    gy, gx = (h + 7) // 8, (w + 7) // 8
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
    shape = rt_params(width=w, height=h, row_begin=0, row_end=h, max_depth=50, seed=1)
    check(lib.rt_feat_create(ds, C.byref(shape), C.byref(ft)))
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
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
    d_len = torch.zeros(n_px, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tp, bd = C.c_void_p(), C.c_void_p()
    check(lib.rt_temporal_create(0, w, h, 0, C.byref(tp)))
    bopt = rt_budget_opts(half_spp=HALF_SPP, target=8, max_mult=MAX_MULT, quantile_64=16)
    check(lib.rt_budget_create(ds, C.byref(shape), C.byref(bopt), C.byref(bd)))
    d_mult = C.c_void_p()
    check(lib.rt_budget_device_mult(bd, C.byref(d_mult)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for i in range(a.batch):
            fn(i)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    ko = rt_temporal_clamp_opts(radius=2, gamma=1.0)

    def motion_step(i):
        k = i & 1
        check(lib.rt_temporal_step_motion(tp, None, C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]), ptr(feat[k]),
                                          ptr(ids[k]), ptr(motion), len(sc), ptr(out[0]), ptr(out[1]), sp))

    def probe(i):
        k = i & 1
        check(lib.rt_temporal_probe(tp, None, C.byref(cams[k]), ptr(feat[k]), ptr(ids[k]), ptr(motion), len(sc), ptr(d_len),
                                    sp))

    def plan(i):
        check(lib.rt_budget_plan(bd, ptr(d_len), sp))

    def clamp_step(i):
        k = i & 1
        check(lib.rt_temporal_step_clamp(tp, None, C.byref(ko), C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]),
                                         ptr(feat[k]), ptr(ids[k]), ptr(motion), len(sc), ptr(out[0]), ptr(out[1]), sp))

    def budget_step(i):
        k = i & 1
        check(lib.rt_temporal_step_budget(tp, None, C.byref(ko), C.byref(cams[k]), ptr(half[k][0]), ptr(half[k][1]),
                                          ptr(feat[k]), ptr(ids[k]), ptr(motion), len(sc), d_mult, ptr(out[0]), ptr(out[1]),
                                          sp))

    legs = {"motion": motion_step, "probe": probe, "plan": plan, "clamp2": clamp_step, "budget": budget_step}
    for fn in legs.values():   # warm-up: the code object, the box scratch, a built-up history, a plan for the weights
        timed(fn)
        timed(fn)
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(timed(legs[k]))

    def stat(v):
        return {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}

    res = {"frame": [w, h], "bodies": len(sc), "rounds": a.rounds, "batch": a.batch, "half_spp": HALF_SPP,
           "max_mult": MAX_MULT}
    for k in legs:
        res[k] = stat(got[k])

    # ---- the frame legs ----
    acc = [C.c_void_p(), C.c_void_p()]
    for x in acc:
        check(lib.rt_accum_create(ds, C.byref(shape), C.byref(x)))
    cam = cams[0]

    def mult_for(share):
        m = np.ones((gy, gx), np.uint32)
        if share > 0:
            th = max(1, round(gy * share ** 0.5))
            tw = max(1, round(gy * gx * share / th))
            y0, x0 = (gy - th) // 2, (gx - tw) // 2
            m[y0:y0 + th, x0:x0 + tw] = MAX_MULT
        return m

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(a.frames):
            fn(f)
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.frames

    def uniform(spp):
        def run(f):
            for j, x in enumerate(acc):
                p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp // 2, max_depth=50, seed=1,
                              sample_begin=f * 2 * MAX_MULT * HALF_SPP + j * (spp // 2))
                check(lib.rt_accum_clear(x, sp))
                check(lib.rt_launch_accum(ds, C.byref(cam), C.byref(p), x, None, sp))
        return run

    frame_legs, meta = {}, {}
    for share in SHARES:
        m = mult_for(share)
        dm = torch.from_numpy(m.reshape(-1).astype(np.int32)).cuda()
        mean_spp = 2 * HALF_SPP * float(np.repeat(np.repeat(m, 8, 0), 8, 1)[:h, :w].mean())
        spp_u = 2 * int(np.ceil(mean_spp / 2))
        launches = [0]

        def budgeted(f, dm=dm, launches=launches, trace=lib.rt_budget_trace):
            check(lib.rt_budget_plan_mult(bd, ptr(dm), sp))
            p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=HALF_SPP, max_depth=50, seed=1,
                          sample_begin=f * 2 * MAX_MULT * HALF_SPP)
            launches[0] = check(trace(ds, C.byref(cam), C.byref(p), bd, None, sp))

        def fused(f, dm=dm, run=budgeted):
            run(f, dm, [0], lib.rt_budget_trace_fused)

        frame_legs[f"budget[{share}]"] = budgeted
        frame_legs[f"fused[{share}]"] = fused
        frame_legs[f"uniform[{share}]"] = uniform(spp_u)
        meta[share] = dict(tiles_at_max=int((m == MAX_MULT).sum()), mean_spp=round(mean_spp, 3), uniform_spp=spp_u,
                           launches=launches, keep=dm)
    frame_legs["full"] = uniform(2 * MAX_MULT * HALF_SPP)
    for fn in frame_legs.values():
        wall(fn)
    fgot = {k: [] for k in frame_legs}
    for r in range(a.rounds):
        for k in (list(frame_legs) if r % 2 == 0 else list(frame_legs)[::-1]):
            fgot[k].append(wall(frame_legs[k]))
    res["frames"] = a.frames
    res["full"] = stat(fgot["full"])
    res["shares"] = []
    crossover = None
    for share in SHARES:
        b, u, fu = stat(fgot[f"budget[{share}]"]), stat(fgot[f"uniform[{share}]"]), stat(fgot[f"fused[{share}]"])
        row = dict(share=share, tiles_at_max=meta[share]["tiles_at_max"], mean_spp=meta[share]["mean_spp"],
                   uniform_spp=meta[share]["uniform_spp"], launches=meta[share]["launches"][0], budget=b, uniform=u,
                   fused=fu, budget_over_uniform=round(b["ms"] / u["ms"], 3),
                   budget_over_full=round(b["ms"] / res["full"]["ms"], 3), fused_over_budget=round(fu["ms"] / b["ms"], 3),
                   fused_over_uniform=round(fu["ms"] / u["ms"], 3))
        res["shares"].append(row)
        if crossover is None and share > 0 and b["ms"] >= u["ms"]:
            crossover = share
    res["first_share_not_cheaper_than_uniform"] = crossover
    res["first_share_fused_not_cheaper_than_uniform"] = next(
        (r["share"] for r in res["shares"] if r["share"] > 0 and r["fused"]["ms"] >= r["uniform"]["ms"]), None)
    us = lambda k: res[k]["ms"] * 1e3   # noqa: E731
    print(f"on {w} x {h}: rt_temporal_step_motion {us('motion'):.1f} us, rt_temporal_probe {us('probe'):.1f} us, "
          f"rt_budget_plan {us('plan'):.1f} us; rt_temporal_step_clamp {us('clamp2'):.1f} us, rt_temporal_step_budget "
          f"{us('budget'):.1f} us")
    for row in res["shares"]:
        print(f"  share {row['share']:.2f}: budgeted {row['budget']['ms']:.3f} ms in {row['launches']} launches "
              f"(mean {row['mean_spp']} spp), fused {row['fused']['ms']:.3f} ms in 2 ({row['fused_over_budget']} of the "
              f"passes), uniform at {row['uniform_spp']} spp {row['uniform']['ms']:.3f} ms, ratios "
              f"{row['budget_over_uniform']} / {row['fused_over_uniform']}")
    print(f"  full rate ({2 * MAX_MULT * HALF_SPP} spp everywhere) {res['full']['ms']:.3f} ms; first share at which the "
          f"budgeted frame is not cheaper than its uniform equivalent: {crossover}")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    for x in acc:
        lib.rt_accum_free(x)
    lib.rt_budget_free(bd)
    lib.rt_temporal_free(tp)
    lib.rt_feat_free(ft)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
