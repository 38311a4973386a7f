#!/usr/bin/env python3
"""What adaptive sampling (include/rt.h, rt_adapt; DESIGN.md §3.1 "adaptive
sampling", §8) costs and saves against the plain launch and against uniform
accumulating passes.

Timing, on one workload of bench.py (default C1: 1200 x 675, cap = its 100
spp, depth 50, seed 1), step 10, min 20, HIP events on the stream, the legs
alternated within every round:

  launch      one rt_launch of the cap spp
  prog        the cap spp as rt_launch_accum passes of the step size and one
              rt_accum_resolve (Progressive's passes)
  adapt@T     rt_adapt_clear (before the window), rt_adapt_step until no tile
              is active, rt_adapt_resolve -- for every tolerance T.  Beside the
              event time: the wall time, the host's wait at the read-backs (the
              wall time of the steps that follow a tested step: they block
              until that step's trace and test are done), the samples traced
              against width x height x cap, and the tiles at the cap.
  resolve     rt_adapt_resolve alone
  empty2      two steps at depth 0 (every pool empty, every tile converges at
              min_spp with both halves 0): the first is an empty trace launch
              and the counts-only kernel, the second an empty trace launch and
              adapt_eval_kernel over every tile -- a bound on the evaluation
              kernel's time from above, timed by events per step

Quality, at --small-width (default 400 x 225): for every tolerance the RMSE of
the adaptive frame against a --ref-spp (2000) rt_launch frame of another seed,
beside the RMSE of the uniform rt_launch frame of the same sample budget
(samples traced / pixels, rounded up).

  python tools/adapt_time.py [--workload c1] [--tols 256 1024 4096 16384] [--rounds 5] [--json out.json]
"""
import argparse
import ctypes as C
import json
import math
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
from bench import WORKLOADS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c1", choices=sorted(WORKLOADS))
    ap.add_argument("--tols", type=int, nargs="+", default=[256, 1024, 4096, 16384])
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--min-spp", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small-width", type=int, default=400)
    ap.add_argument("--ref-spp", type=int, default=2000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    wl = WORKLOADS[a.workload]
    w, cap, depth = wl["width"], wl["spp"], wl["depth"]
    h = R.image_height(w)
    sc = scenes.cover_c4() if wl["scene"] == "c4" else scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ds, acc = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=cap, max_depth=depth, seed=1)
    check(lib.rt_accum_create(ds, C.byref(p), C.byref(acc)))
    n = h * w * 3
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    out2 = torch.empty(n, dtype=torch.float32, device="cuda")
    opts = dict(step=a.step, min_spp=a.min_spp, max_spp=cap)
    ads = {t: R.Adaptive(sc, cam, w, h, tol_q16=t, max_depth=depth, seed=1, stream=s.cuda_stream, **opts)
           for t in a.tols}
    empty = R.Adaptive(sc, cam, w, h, tol_q16=0, max_depth=0, seed=1, stream=s.cuda_stream, **opts)

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def launch():
        e0, e1 = events()
        e0.record(s)
        check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), None, sp))
        e1.record(s)
        torch.cuda.synchronize()
        return {"ms": e0.elapsed_time(e1)}

    def prog():
        check(lib.rt_accum_clear(acc, sp))
        q = rt_params.from_buffer_copy(p)
        e0, e1 = events()
        e0.record(s)
        for _ in range(cap // a.step):
            q.spp = a.step
            check(lib.rt_launch_accum(ds, C.byref(cam), C.byref(q), acc, None, sp))
            q.sample_begin += a.step
        check(lib.rt_accum_resolve(acc, 0, C.c_void_p(out2.data_ptr()), sp))
        e1.record(s)
        torch.cuda.synchronize()
        return {"ms": e0.elapsed_time(e1)}

    def adapt(ad):
        ad.clear()
        torch.cuda.synchronize()
        e0, e1 = events()
        t0 = time.perf_counter()
        e0.record(s)
        wait, k, tested = 0.0, 0, False
        while True:
            t = time.perf_counter()
            traced = ad.step()
            if tested:
                wait += time.perf_counter() - t
            if traced == 0:
                break
            k += 1
            tested = k % 2 == 0 and a.min_spp <= k * a.step < cap
        ad.resolve_into(out2.data_ptr())
        e1.record(s)
        torch.cuda.synchronize()
        return {"ms": e0.elapsed_time(e1), "wall_ms": (time.perf_counter() - t0) * 1e3, "host_wait_ms": wait * 1e3,
                "steps": k}

    def resolve():
        e0, e1 = events()
        e0.record(s)
        ads[a.tols[0]].resolve_into(out2.data_ptr())
        e1.record(s)
        torch.cuda.synchronize()
        return {"ms": e0.elapsed_time(e1)}

    def empty2():
        empty.clear()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record(s)
        assert empty.step() > 0
        ev[1].record(s)
        assert empty.step() > 0
        ev[2].record(s)
        torch.cuda.synchronize()
        assert empty.step() == 0
        return {"ms": ev[0].elapsed_time(ev[2]), "counts_step_ms": ev[0].elapsed_time(ev[1]),
                "eval_step_ms": ev[1].elapsed_time(ev[2])}

    legs = {"launch": launch, "prog": prog, "resolve": resolve, "empty2": empty2}
    for t in a.tols:
        legs[f"adapt@{t}"] = (lambda ad: lambda: adapt(ad))(ads[t])
    names = list(legs)
    for k in names:   # warm-up: code object, tile-order records
        legs[k]()
        legs[k]()
    info = {}
    for t in a.tols:
        counts = ads[t].counts()
        info[t] = {"samples_traced": ads[t].samples_traced, "samples_cap": w * h * cap,
                   "tiles": int(counts.size), "tiles_at_cap": int((counts == cap).sum()),
                   "tiles_at_min": int((counts == a.min_spp).sum()), "mean_spp": ads[t].samples_traced / (w * h)}
    res = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            res[k].append(legs[k]())

    def med(k, f="ms"):
        return statistics.median(x[f] for x in res[k])
    base = med("launch")
    print(f"{a.workload}: {w} x {h}, cap {cap} spp, step {a.step}, min {a.min_spp}, {a.rounds} rounds "
          "(events on the stream, medians)")
    print(f"  launch   {base:8.4f} ms")
    print(f"  prog     {med('prog'):8.4f} ms  ({med('prog') / base:5.3f} x launch)  {cap // a.step} passes + resolve")
    for t in a.tols:
        k, i = f"adapt@{t}", info[t]
        print(f"  {k:12s} {med(k):8.4f} ms  ({med(k) / base:5.3f} x launch, {med(k) / med('prog'):5.3f} x prog)  "
              f"wall {med(k, 'wall_ms'):7.4f}  host wait at read-backs {med(k, 'host_wait_ms'):7.4f}  "
              f"steps {res[k][0]['steps']}  samples {i['samples_traced'] / 1e6:6.2f} M of {i['samples_cap'] / 1e6:.1f} M "
              f"({i['samples_traced'] / i['samples_cap']:.3f})  tiles at cap {i['tiles_at_cap']} / at min "
              f"{i['tiles_at_min']} of {i['tiles']}")
    print(f"  resolve  {med('resolve'):8.4f} ms (rt_adapt_resolve alone)")
    print(f"  depth 0: empty trace + counts kernel {med('empty2', 'counts_step_ms'):7.4f} ms, empty trace + "
          f"adapt_eval_kernel over all {info[a.tols[0]]['tiles']} tiles {med('empty2', 'eval_step_ms'):7.4f} ms",
          flush=True)
    for ad in list(ads.values()) + [empty]:
        ad.close()
    lib.rt_accum_free(acc)
    lib.rt_scene_free(ds)

    # ---- quality at reduced size ----
    w2 = a.small_width
    h2 = R.image_height(w2)
    cam2 = scenes.cover_camera(w2, h2)
    ds2 = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds2)))
    buf = torch.empty(h2 * w2 * 3, dtype=torch.float32, device="cuda")

    def frame(spp, seed):
        q = rt_params(width=w2, height=h2, row_begin=0, row_end=h2, spp=spp, max_depth=depth, seed=seed)
        check(lib.rt_launch(ds2, C.byref(cam2), C.byref(q), C.c_void_p(buf.data_ptr()), None, sp))
        torch.cuda.synchronize()
        return buf.cpu().numpy().astype(np.float64).reshape(h2, w2, 3)

    def rmse(x, y):
        return float(np.sqrt(np.mean((x - y) ** 2)))
    ref = frame(a.ref_spp, 2)    # (another seed: independent of the frames it judges)
    quality = {}
    print(f"quality at {w2} x {h2}: RMSE against {a.ref_spp} spp (seed 2); cap-spp uniform frame "
          f"{rmse(frame(cap, 1), ref):.5f}")
    for t in a.tols:
        with R.Adaptive(sc, cam2, w2, h2, tol_q16=t, max_depth=depth, seed=1, **opts) as ad:
            ad.run()
            f, traced = ad.frame().astype(np.float64), ad.samples_traced
        budget = math.ceil(traced / (w2 * h2))
        quality[t] = {"samples_traced": traced, "mean_spp": traced / (w2 * h2), "rmse_adaptive": rmse(f, ref),
                      "uniform_spp": budget, "rmse_uniform": rmse(frame(budget, 1), ref)}
        print(f"  tol {t:6d}: mean {quality[t]['mean_spp']:6.2f} spp  RMSE adaptive {quality[t]['rmse_adaptive']:.5f}  "
              f"uniform {budget} spp {quality[t]['rmse_uniform']:.5f}", flush=True)
    lib.rt_scene_free(ds2)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(
            {"workload": a.workload, "width": w, "height": h, "cap": cap, "step": a.step, "min_spp": a.min_spp,
             "rounds": a.rounds, "runs": res, "tiles": {str(t): v for t, v in info.items()},
             "quality": {"width": w2, "height": h2, "ref_spp": a.ref_spp, "tols": {str(t): v for t, v in quality.items()}}},
            indent=1))


if __name__ == "__main__":
    main()
