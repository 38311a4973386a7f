#!/usr/bin/env python3
"""What the feature-guided denoiser (include/rt.h, rt_denoise; DESIGN.md §3.8,
§8) costs beside the passes that feed it, on C1's frame (cover scene grid 11,
1200 x 675, depth 50, seed 1) with halves of 4 + 4 spp, in one process.

HIP events on one stream, the legs alternated within every round, medians over
the rounds:

  denoise   the whole rt_denoise (prep + the levels), default options
  profile   rt_denoise_profile: the prep and every level on their own (an event
            behind each kernel), with the bytes each must move at least --
            every packed array read once, the texels (the last level: the
            frame) written once -- and that figure per second
  launch    one rt_launch of 8 spp, beside it
  feat      one rt_launch_feat pass of 8 spp into cleared buffers (the clear
            outside the window)

--alt-library PATH times another build of the ABI (an A/B of the level
kernel's designs) in the same rounds, on the same inputs, and compares the two
outputs' bits.

  python tools/denoise_time.py [--rounds 9] [--alt-library lib.so] [--json out.json]
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
from rtclj._lib import DENOISE_DEFAULTS, check, lib, load, rt_params  # noqa: E402

LEVELS = DENOISE_DEFAULTS["levels"]
# bytes per pixel a kernel must move at least (denoise.h's packed arrays)
PREP_BYTES = (3 + 3 + 8) * 4 + 16 + 16 + 4
LEVEL_BYTES = 16 + 16 + 4 + 16
LAST_BYTES = 16 + 16 + 4 + 3 * 4 + 3 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--alt-library", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    n_px = w * h
    sc = scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    libs = {"product": lib}
    if a.alt_library:
        libs["alt"] = load(Path(a.alt_library))
    ds, ft = C.c_void_p(), C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    shape = rt_params(width=w, height=h, row_begin=0, row_end=h)
    check(lib.rt_feat_create(ds, C.byref(shape), C.byref(ft)))
    frame = torch.empty(n_px * 3, dtype=torch.float32, device="cuda")
    half = [torch.empty(n_px * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    feat = torch.empty(n_px * 8, dtype=torch.float32, device="cuda")
    outs = {k: torch.full((n_px * 3,), float("nan"), dtype=torch.float32, device="cuda") for k in libs}
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    p8 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=8, max_depth=50, seed=1)
    # the inputs: two 4-spp halves of the frame's rays and the features of all 8
    for k in range(2):
        p4 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=4, max_depth=50, seed=1, sample_begin=4 * k)
        check(lib.rt_launch(ds, C.byref(cam), C.byref(p4), ptr(half[k]), None, sp))
    check(lib.rt_launch_feat(ds, C.byref(cam), C.byref(p8), ft, None, sp))
    check(lib.rt_feat_resolve(ft, ptr(feat), sp))
    torch.cuda.synchronize()
    dns = {}
    for k, dll in libs.items():
        dns[k] = C.c_void_p()
        assert dll.rt_denoiser_create(0, w, h, C.byref(dns[k])) == 0, dll.rt_last_error()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def denoise(k):
        def run():
            assert libs[k].rt_denoise(dns[k], None, ptr(half[0]), ptr(half[1]), ptr(feat), ptr(outs[k]), sp) == 0
        return lambda: timed(run)

    def profile(k):
        def run():
            ms = (C.c_float * (LEVELS + 2))()
            torch.cuda.synchronize()
            assert libs[k].rt_denoise_profile(dns[k], None, ptr(half[0]), ptr(half[1]), ptr(feat), ptr(outs[k]), sp,
                                              ms) == 0, libs[k].rt_last_error()
            return list(ms)
        return run

    def feat_pass():
        check(lib.rt_feat_clear(ft, sp))
        return timed(lambda: check(lib.rt_launch_feat(ds, C.byref(cam), C.byref(p8), ft, None, sp)))

    legs = {"launch": lambda: timed(lambda: check(lib.rt_launch(ds, C.byref(cam), C.byref(p8), ptr(frame), None, sp))),
            "feat": feat_pass}
    for k in libs:
        legs["denoise:" + k] = denoise(k)
        legs["profile:" + k] = profile(k)
    for fn in legs.values():   # warm-up: code objects, the schedule's first order
        fn()
        fn()
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(legs[k]())

    def stat(v):
        return {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    res = {"frame": [w, h], "bodies": len(sc), "rounds": a.rounds, "levels": LEVELS, "halves_spp": [4, 4],
           "launch_8spp": stat(got["launch"]), "feat_8spp": stat(got["feat"])}
    for k in libs:
        row = {"whole": stat(got["denoise:" + k])}
        cols = list(zip(*got["profile:" + k]))
        names = ["prep"] + [f"level{i}" for i in range(LEVELS)] + ["whole_profiled"]
        bytes_px = [PREP_BYTES] + [LEVEL_BYTES] * (LEVELS - 1) + [LAST_BYTES, None]
        for name, col, b in zip(names, cols, bytes_px):
            row[name] = stat(col)
            if b is not None:
                row[name]["bytes"] = b * n_px
                row[name]["gb_per_s"] = round(b * n_px / (row[name]["ms"] * 1e6), 1)
        row["share_of_launch_8spp"] = round(row["whole"]["ms"] / res["launch_8spp"]["ms"], 4)
        res[k] = row
        print(f"{k}: rt_denoise {row['whole']['ms']:.4f} ms (8-spp rt_launch {res['launch_8spp']['ms']:.3f} ms, "
              f"rt_launch_feat {res['feat_8spp']['ms']:.3f} ms); " +
              ", ".join(f"{n} {row[n]['ms']:.4f} ms / {row[n].get('gb_per_s', '-')} GB/s" for n in names[:-1]))
    if "alt" in libs:
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["product"].view(torch.int32), outs["alt"].view(torch.int32)))
        res["alt_equals_product_bits"] = same
        print("alt output == product output, bit for bit:", same)
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    for k, dll in libs.items():
        dll.rt_denoiser_free(dns[k])
    lib.rt_feat_free(ft)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
