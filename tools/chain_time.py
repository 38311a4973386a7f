#!/usr/bin/env python3
"""What the specular-chain feature pass (include/rt.h, rt_launch_feat_chain;
DESIGN.md §3.15, §8.1) costs beside the first-hit pass on C1's frame (cover
scene grid 11, 1200 x 675, seed 1), in one process.

HIP events on one stream, the legs alternated within every round, medians over
the rounds; every leg is a batch of --batch calls between two events.  Per
selector (0: the tree in LDS, 12: the tree in global memory):

  feat      rt_launch_feat of --spp samples a pixel
  chain     rt_launch_feat_chain of the same samples, max_bounces 8
  chain0    the same with max_bounces 0 (the first-hit pass's work in the chain kernel)

With --before PATH (a librtclj.so built from the commit before the chain pass)
that build's rt_launch_feat runs in the same rounds as `feat_before`: the
first-hit pass's own time before and after.  Then the counters' mean segments a
sample, the kernels' occupancy, and the share a chain pass adds to a sequence
frame (tools/upsample_time.py's full-size frame: two 4-spp halves, features,
ids, step, denoiser -- with and without a second, chain rt_feat).

  python tools/chain_time.py [--rounds 9] [--batch 20] [--spp 8] [--before PATH] [--json out.json]
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
from rtclj._lib import check, lib, load, rt_feat_chain_opts, rt_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--before", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w = a.width
    h = R.image_height(w)
    n_px = w * h
    scene = scenes.cover(11, 42)
    cam = scenes.cover_camera(w, h)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device="cuda")   # noqa: E731
    full = rt_params(width=w, height=h, row_begin=0, row_end=h, max_depth=50, seed=1)
    fp = rt_params.from_buffer_copy(full)
    fp.spp, fp.max_depth = a.spp, 1
    libs = {"after": lib}
    if a.before:
        libs["before"] = load(Path(a.before))
    ds, ft = {}, {}
    for k, dll in libs.items():
        ds[k], ft[k] = C.c_void_p(), C.c_void_p()
        assert dll.rt_scene_upload(0, C.byref(scene.c), C.byref(ds[k])) == 0
        assert dll.rt_feat_create(ds[k], C.byref(full), C.byref(ft[k])) == 0
    fch = C.c_void_p()
    check(lib.rt_feat_create(ds["after"], C.byref(full), C.byref(fch)))
    o8, o0 = rt_feat_chain_opts(8, 0.0), rt_feat_chain_opts(0, 0.0)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def feat(k):
        dll = libs[k]

        def run():
            assert dll.rt_feat_clear(ft[k], sp) == 0
            assert dll.rt_launch_feat(ds[k], C.byref(cam), C.byref(fp), ft[k], None, sp) == 0
        return run

    def chain(o, counters=None):
        def run():
            check(lib.rt_feat_clear(fch, sp))
            check(lib.rt_launch_feat_chain(ds["after"], C.byref(cam), C.byref(fp), C.byref(o), fch, counters, sp))
        return run

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for _ in range(a.batch):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    # ---- a sequence frame, with and without the chain rt_feat ----
    acc = [C.c_void_p(), C.c_void_p()]
    for x in acc:
        check(lib.rt_accum_create(ds["after"], C.byref(full), C.byref(x)))
    half, acc_out = [f32(n_px * 3) for _ in range(2)], [f32(n_px * 3) for _ in range(2)]
    d_feat, d_chain, out = f32(n_px * 8), f32(n_px * 8), f32(n_px * 3)
    ids = torch.empty(n_px, dtype=torch.int32, device="cuda")
    motion = torch.zeros(len(scene) * 4, dtype=torch.float32, device="cuda")
    tp, dn = C.c_void_p(), C.c_void_p()
    check(lib.rt_temporal_create(0, w, h, 0, C.byref(tp)))
    check(lib.rt_denoiser_create(0, w, h, C.byref(dn)))
    torch.cuda.synchronize()

    def frame(chained):
        def run():
            for k, x in enumerate(acc):
                p = rt_params.from_buffer_copy(full)
                p.spp, p.sample_begin = 4, 4 * k
                check(lib.rt_accum_clear(x, sp))
                check(lib.rt_launch_accum(ds["after"], C.byref(cam), C.byref(p), x, None, sp))
                check(lib.rt_accum_resolve(x, 0, ptr(half[k]), sp))
            feat("after")()
            check(lib.rt_feat_resolve(ft["after"], ptr(d_feat), sp))
            if chained:
                chain(o8)()
                check(lib.rt_feat_resolve(fch, ptr(d_chain), sp))
            check(lib.rt_launch_ids(ds["after"], C.byref(cam), w, h, 0, ptr(ids), sp))
            check(lib.rt_temporal_step_motion(tp, None, C.byref(cam), ptr(half[0]), ptr(half[1]), ptr(d_feat), ptr(ids),
                                              ptr(motion), len(scene), ptr(acc_out[0]), ptr(acc_out[1]), sp))
            check(lib.rt_denoise(dn, None, ptr(acc_out[0]), ptr(acc_out[1]), ptr(d_chain if chained else d_feat), ptr(out), sp))
        return run

    res = {"frame": [w, h], "bodies": len(scene), "spp": a.spp, "rounds": a.rounds, "batch": a.batch}
    out4 = (C.c_int * 4)()
    for sel, name in ((0, "lds"), (12, "global")):
        old = [dll.rt_set_variant(sel) for dll in libs.values()]
        legs = {"feat": lambda: timed(feat("after")), "chain": lambda: timed(chain(o8)), "chain0": lambda: timed(chain(o0))}
        if a.before:
            legs["feat_before"] = lambda: timed(feat("before"))
        if sel == 0:
            legs["frame"] = lambda: timed(frame(False))
            legs["frame_chain"] = lambda: timed(frame(True))
        for fn in legs.values():   # warm-up
            fn()
        got = {k: [] for k in legs}
        for r in range(a.rounds):
            for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):   # alternated
                got[k].append(legs[k]())
        e = res[name] = {k: {"ms": round(statistics.median(x), 5), "min": round(min(x), 5), "max": round(max(x), 5)}
                         for k, x in got.items()}
        cnt.zero_()
        torch.cuda.synchronize()
        chain(o8, ptr(cnt))()
        torch.cuda.synchronize()
        segs, smp = cnt.cpu().numpy().tolist()
        e["segments_per_sample"] = round(segs / smp, 4)
        check(lib.rt_feat_occupancy(ds["after"], out4))
        e["feat_occupancy"] = list(out4)
        check(lib.rt_feat_chain_occupancy(ds["after"], out4))
        e["chain_occupancy"] = list(out4)
        e["chain_over_feat"] = round(e["chain"]["ms"] / e["feat"]["ms"], 3)
        for dll, v in zip(libs.values(), old):
            dll.rt_set_variant(v)
        line = ", ".join(f"{k} {x['ms'] * 1e3:.1f} us" for k, x in e.items() if isinstance(x, dict))
        print(f"{name}: {line}; {e['segments_per_sample']} segments a sample; occupancy feat {e['feat_occupancy']}, "
              f"chain {e['chain_occupancy']}")
    fr = res["lds"]
    res["frame_share_added"] = round(fr["frame_chain"]["ms"] / fr["frame"]["ms"] - 1.0, 4)
    print(f"a sequence frame {fr['frame']['ms']:.4f} ms, with the chain rt_feat {fr['frame_chain']['ms']:.4f} ms: "
          f"+{100 * res['frame_share_added']:.2f} %")
    print(json.dumps(res))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    torch.cuda.synchronize()
    lib.rt_denoiser_free(dn)
    lib.rt_temporal_free(tp)
    lib.rt_feat_free(fch)
    for x in acc:
        lib.rt_accum_free(x)
    for k, dll in libs.items():
        dll.rt_feat_free(ft[k])
        dll.rt_scene_free(ds[k])


if __name__ == "__main__":
    main()
