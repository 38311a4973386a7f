#!/usr/bin/env python3
"""What guided upsampling (include/rt.h, rt_upsample)
costs and saves on C1's frame (cover scene grid 11, 1200 x 675, depth 50,
seed 1) at scale 2 (coarse 600 x 338), in one process.

HIP events on one stream, the legs alternated within every round, medians over
the rounds; every leg is a batch of --batch calls between two events.

The kernel reads 32 bytes a fine pixel (the features) and 56 a coarse pixel
(two halves, the coarse features) and writes 24 a fine pixel (two outputs):

  upsample  rt_upsample, two images, default options
  copy      a device-to-device copy whose traffic is the kernel's byte count
            (half of it read, half of it written)
  copy2     the same with the kernel's byte count as the copy's payload

and a sequence frame's stages at 8 spp per traced pixel, at full size and with
scale 2, each alone and as one frame (everything enqueued between two events):

  trace     two rt_accum_clear, two rt_launch_accum of 4 spp, two rt_accum_resolve
  feat      rt_feat_clear, rt_launch_feat of 8 spp, rt_feat_resolve (full size)
  cfeat     the same on the coarsened camera (scale 2 only)
  ids       rt_launch_ids
  upsample  rt_upsample (scale 2 only)
  step      rt_temporal_step_motion (nothing moves: a zero table)
  denoise   rt_denoise
  frame     all of the above, in the pipeline's order

  python tools/upsample_time.py [--rounds 9] [--batch 20] [--json out.json]
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

FINE_BYTES, COARSE_BYTES = 8 * 4 + 2 * 3 * 4, (3 + 3 + 8) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w, sc_ = a.width, a.scale
    h = R.image_height(w)
    cw, ch = R.coarse_size(w, h, sc_)
    n_px, n_c = w * h, cw * ch
    scene = scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    ccam = R.camera_coarsen(cam, sc_)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device="cuda")   # noqa: E731
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(scene.c), C.byref(ds)))
    full = rt_params(width=w, height=h, row_begin=0, row_end=h, max_depth=50, seed=1)
    small = rt_params(width=cw, height=ch, row_begin=0, row_end=ch, max_depth=50, seed=1)
    # either variant's objects: the accumulators at the traced size, the features
    v = {}
    for name, shape, tcam in (("full", full, cam), ("scaled", small, ccam)):
        e = v[name] = dict(shape=shape, cam=tcam, acc=[C.c_void_p(), C.c_void_p()], n=shape.width * shape.height)
        for acc in e["acc"]:
            check(lib.rt_accum_create(ds, C.byref(shape), C.byref(acc)))
        e["half"] = [f32(e["n"] * 3) for _ in range(2)]
    ft, fc = C.c_void_p(), C.c_void_p()
    check(lib.rt_feat_create(ds, C.byref(full), C.byref(ft)))
    check(lib.rt_feat_create(ds, C.byref(small), C.byref(fc)))
    feat, cfeat = f32(n_px * 8), f32(n_c * 8)
    up = [f32(n_px * 3) for _ in range(2)]
    acc_out = [f32(n_px * 3) for _ in range(2)]
    out = f32(n_px * 3)
    ids = torch.empty(n_px, dtype=torch.int32, device="cuda")
    motion = torch.zeros(len(scene) * 4, dtype=torch.float32, device="cuda")
    total = n_px * FINE_BYTES + n_c * COARSE_BYTES
    src = torch.zeros(total, dtype=torch.uint8, device="cuda")
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    tp, dn = C.c_void_p(), C.c_void_p()
    check(lib.rt_temporal_create(0, w, h, 0, C.byref(tp)))
    check(lib.rt_denoiser_create(0, w, h, C.byref(dn)))
    torch.cuda.synchronize()

    def trace(e):
        for k, acc in enumerate(e["acc"]):
            p = rt_params.from_buffer_copy(e["shape"])
            p.spp, p.sample_begin = 4, 4 * k
            check(lib.rt_accum_clear(acc, sp))
            check(lib.rt_launch_accum(ds, C.byref(e["cam"]), C.byref(p), acc, None, sp))
            check(lib.rt_accum_resolve(acc, 0, ptr(e["half"][k]), sp))

    def feats(handle, shape, tcam, d_out):
        p = rt_params.from_buffer_copy(shape)
        p.spp, p.max_depth = 8, 1
        check(lib.rt_feat_clear(handle, sp))
        check(lib.rt_launch_feat(ds, C.byref(tcam), C.byref(p), handle, None, sp))
        check(lib.rt_feat_resolve(handle, d_out, sp))

    def upsample():
        e = v["scaled"]
        R.upsample_into(e["half"][0].data_ptr(), e["half"][1].data_ptr(), cfeat.data_ptr(), feat.data_ptr(), w, h,
                        up[0].data_ptr(), up[1].data_ptr(), stream=s.cuda_stream, scale=sc_)

    def step(halves):
        check(lib.rt_temporal_step_motion(tp, None, C.byref(cam), ptr(halves[0]), ptr(halves[1]), ptr(feat), ptr(ids),
                                          ptr(motion), len(scene), ptr(acc_out[0]), ptr(acc_out[1]), sp))

    def denoise():
        check(lib.rt_denoise(dn, None, ptr(acc_out[0]), ptr(acc_out[1]), ptr(feat), ptr(out), sp))

    def stages(name):
        e = v[name]
        halves = e["half"] if name == "full" else up
        st = {"trace": lambda: trace(e), "feat": lambda: feats(ft, full, cam, ptr(feat))}
        if name == "scaled":
            st["cfeat"] = lambda: feats(fc, small, ccam, ptr(cfeat))
        st["ids"] = lambda: check(lib.rt_launch_ids(ds, C.byref(cam), w, h, 0, ptr(ids), sp))
        if name == "scaled":
            st["upsample"] = upsample
        st["step"] = lambda: step(halves)
        st["denoise"] = denoise
        return st

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for _ in range(a.batch):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def copy(nbytes):
        a_, b_ = dst[:nbytes], src[:nbytes]

        def run():
            with torch.cuda.stream(s):
                a_.copy_(b_)        # (contiguous bytes: the runtime's device-to-device copy on the stream)
        return run

    legs = {"upsample": lambda: timed(upsample), "copy": lambda: timed(copy(total // 2)),
            "copy2": lambda: timed(copy(total))}
    for name in ("full", "scaled"):
        st = stages(name)
        for k, fn in st.items():
            legs[f"{name}:{k}"] = (lambda fn=fn: timed(fn))
        legs[f"{name}:frame"] = (lambda st=st: timed(lambda: [fn() for fn in st.values()]))
    # the inputs of every leg exist before any is timed: one frame of either variant
    for name in ("full", "scaled"):
        for fn in stages(name).values():
            fn()
    for fn in legs.values():   # warm-up: the code objects, the copy's path, the schedule's first order
        fn()
    got = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
            got[k].append(legs[k]())

    def stat(x):
        return {"ms": round(statistics.median(x), 5), "min": round(min(x), 5), "max": round(max(x), 5)}

    res = {"frame": [w, h], "coarse": [cw, ch], "scale": sc_, "bodies": len(scene), "rounds": a.rounds, "batch": a.batch,
           "bytes": {"fine_pixel": FINE_BYTES, "coarse_pixel": COARSE_BYTES, "total": total}}
    for k in legs:
        res[k] = stat(got[k])
    res["upsample"]["gb_per_s"] = round(total / (res["upsample"]["ms"] * 1e6), 1)
    res["upsample"]["over_copy"] = round(res["upsample"]["ms"] / res["copy"]["ms"], 3)
    res["upsample"]["over_copy2"] = round(res["upsample"]["ms"] / res["copy2"]["ms"], 3)
    res["frame_scaled_over_full"] = round(res["scaled:frame"]["ms"] / res["full:frame"]["ms"], 4)
    print(f"rt_upsample on {w} x {h} from {cw} x {ch}: {res['upsample']['ms'] * 1e3:.1f} us ({total} B: "
          f"{res['upsample']['gb_per_s']} GB/s); a device copy with that traffic {res['copy']['ms'] * 1e3:.1f} us, "
          f"with that payload {res['copy2']['ms'] * 1e3:.1f} us")
    for name in ("full", "scaled"):
        print(f"{name}: " + ", ".join(f"{k.split(':')[1]} {x['ms']:.4f} ms" for k, x in res.items()
                                     if isinstance(x, dict) and k.startswith(name + ":")))
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    torch.cuda.synchronize()
    lib.rt_denoiser_free(dn)
    lib.rt_temporal_free(tp)
    lib.rt_feat_free(ft)
    lib.rt_feat_free(fc)
    for e in v.values():
        for acc in e["acc"]:
            lib.rt_accum_free(acc)
    lib.rt_scene_free(ds)


if __name__ == "__main__":
    main()
