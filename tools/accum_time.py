#!/usr/bin/env python3
"""What accumulating passes cost against the plain launch (include/rt.h,
rt_accum; DESIGN.md §3.1 "accumulating passes", §8).

On one workload of bench.py (default C1: 1200 x 675, 100 spp, depth 50, seed
1), HIP events on the stream around, alternated within every round:

  launch     one rt_launch of the spp (the float frame; the existing path)
  acc1/4/10  the spp as 1, 4 and 10 rt_launch_accum passes and one
             rt_accum_resolve (the accumulator cleared before the window)
  resolve    rt_accum_resolve alone
  clear      rt_accum_clear alone

Each is warmed up first (its tile-order record, the code object), the order
within a round rotates, and the medians, minima and all samples are printed
and written as JSON.  The frames are compared once: every accN frame must
equal the launch's bit for bit.

  python tools/accum_time.py [--workload c1] [--rounds 9] [--json out.json]
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
from bench import WORKLOADS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c1", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    wl = WORKLOADS[a.workload]
    w, spp = wl["width"], wl["spp"]
    h = R.image_height(w)
    sc = scenes.cover_c4() if wl["scene"] == "c4" else scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    ds, acc = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=wl["depth"], seed=1)
    check(lib.rt_accum_create(ds, C.byref(p), C.byref(acc)))
    n = h * w * 3
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    out_acc = torch.empty(n, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)

    def launch():
        check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), None, sp))

    def resolve():
        check(lib.rt_accum_resolve(acc, 0, C.c_void_p(out_acc.data_ptr()), sp))

    def clear():
        check(lib.rt_accum_clear(acc, sp))

    def passes(k):
        q = rt_params.from_buffer_copy(p)
        for n_k in R.pass_sizes(spp, k):
            q.spp = n_k
            check(lib.rt_launch_accum(ds, C.byref(cam), C.byref(q), acc, None, sp))
            q.sample_begin += n_k
        resolve()

    def timed(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"launch": (launch, None), "acc1": (lambda: passes(1), clear), "acc4": (lambda: passes(4), clear),
            "acc10": (lambda: passes(10), clear), "resolve": (resolve, None), "clear": (clear, None)}
    # warm-up, and the frames compared once
    exact = {}
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    want = out.cpu()
    for name in ("acc1", "acc4", "acc10"):
        for _ in range(2):
            clear()
            legs[name][0]()
        torch.cuda.synchronize()
        exact[name] = bool(torch.equal(out_acc.cpu(), want))
    names = list(legs)
    res = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            fn, before = legs[k]
            res[k].append(timed(fn, before))
    base = statistics.median(res["launch"])
    summary = {"workload": a.workload, "width": w, "height": h, "spp": spp, "rounds": a.rounds,
               "frames_equal_launch": exact, "sums_bytes": n * 8, "frame_bytes": n * 4,
               "ms": res, "median_ms": {k: statistics.median(v) for k, v in res.items()},
               "min_ms": {k: min(v) for k, v in res.items()}}
    print(f"{a.workload}: {w} x {h}, {spp} spp, {a.rounds} rounds (events on the stream); "
          f"sums {n * 8 / 1e6:.1f} MB, frame {n * 4 / 1e6:.1f} MB; frames equal the launch's: {exact}")
    for k in names:
        med = summary["median_ms"][k]
        print(f"  {k:8s} median {med:8.4f} ms  min {min(res[k]):8.4f}  max {max(res[k]):8.4f}"
              f"  ({med / base:6.3f} x launch)", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(summary, indent=1))
    lib.rt_accum_free(acc)
    lib.rt_scene_free(ds)
    if not all(exact.values()):
        sys.exit("an accumulated frame differs from the launch's")


if __name__ == "__main__":
    main()
