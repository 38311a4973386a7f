"""The kernel at the edges of the scene, material, camera and RNG inputs
(tests/edge_scenes.py: albedos above 1, negative and saturating sample
colours, fuzz and refraction indices outside their usual ranges, negative
radii, identical spheres, non-finite bodies on both sides of bvh.cpp's former
limit of 64, ray origins exactly on a surface and at a centre, scenes scaled
from 2^-62 to 2^63 -- the cold length branch from below and above, denormal
r * r -- 64-bit seeds, sample_begin over the uint32 wrap, max_depth -1).
64 x 36, 16 spp, depth 12, seed 1; at most 120 bodies.

  * the default launch equals the fp32 mirror (MODE_MIRROR32 | DIRECT; with
    RT_FLAG_REJECTION_SAMPLERS MODE_MIRROR32) bit for bit, segments and
    samples included; NaN compares equal to NaN, and a finite mirror frame
    means a finite GPU frame;
  * the default launch runs the compact variant 22 where every albedo lies
    within [-1, 1], else 16 (u64 sums);
  * every BVH variant (11, 12, 16, 18, 22, 24, 26, 28) equals the scan
    (variant 5), frames and segment counts; where a compact variant falls
    back to 16 the fallback is asserted (rt_launch_occupancy) and the frame
    that was rendered is compared;
  * where the input means the same in both precisions (edge_scenes
    .FP64_NAMES) the GPU frame is held to the same-draw fp64 reference
    (MODE_REF64D) within oracle.pin.BOUNDS.  The GPU equals the mirror, so
    the values measured on the MI355X are those of
    tests/test_oracle_input_edges.py's table (seg_rel, lin_mean, px8_mean,
    px8_off_gt1, block_mean / block_max), the largest: ties_big 8.7e-4,
    7.5e-5, 0.016, 0.28 %, 0.016 / 0.5; albedo_gt1_centre 7.5e-6, 2.1e-5,
    0.0045, 0.043 %, 0.0045 / 0.56; every other case at most 1.4e-4, 1.5e-5,
    0.0046, 0.087 %, 0.0046 / 0.56.

A root of +inf (a body whose r * r overflows: nonfinite_few's r = 1e30, the
ground at 2^62) is where the BVH variants once left the scan: their (t, index)
compare took it for a tie with "no hit yet"; bvh.cpp now keeps such bodies,
like the non-finite ones, out of the tree and the big-body list.
"""
import numpy as np
import pytest

import edge_scenes as E
from oracle.pin import BOUNDS, compare, within
from test_gpu_parity import variant
from test_gpu_ref64_direct import _launch_variant

pytestmark = pytest.mark.gpu

BVH_VARIANTS = (11, 12, 16, 18, 22, 24, 26, 28)
COMPACT = (22, 24, 26, 28)          # fall back to 16 where an albedo leaves [-1, 1]
CASES = [(n, "direct") for n in E.NAMES] + [(n, "rejection") for n in E.REJECTION_NAMES]


def _render(sc, cam, meta, samplers="direct", library=None, flags=0, u8=False, n_devices=0, **over):
    from rtclj import raytracing as R
    from rtclj._lib import RT_FLAG_REJECTION_SAMPLERS
    p = E.params(meta, **over)
    st = {}
    img = R.render(sc, cam, E.W, E.H, spp=p["spp"], max_depth=p["max_depth"], seed=p["seed"],
                   sample_begin=p["sample_begin"], stats=st, library=library, u8=u8, n_devices=n_devices,
                   flags=flags | (RT_FLAG_REJECTION_SAMPLERS if samplers == "rejection" else 0))
    return img, st


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _differing(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())


@pytest.mark.parametrize("name,samplers", CASES)
def test_default_launch_equals_mirror(gpu_lib, name, samplers):
    from rtclj._lib import lib
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    # the variant the default launch runs: the compact image only where its
    # u32 sums cannot overflow
    assert _launch_variant(lib, sc, E.W, E.H, p["spp"], p["max_depth"]) == (22 if meta["unit"] else 16)
    g, st = _render(sc, cam, meta, samplers)
    m, segs, smp = E.mirror(name, rejection=samplers == "rejection")
    print(f"{name} ({samplers}): segments/sample {segs / max(smp, 1):.4f}, frame max {np.nanmax(m):.4g}, "
          f"finite {bool(np.isfinite(m).all())}, pixels that differ {_differing(g, m)}")
    assert _same(g, m), (name, samplers, _differing(g, m))
    assert (st["segments"], st["samples"]) == (segs, smp)
    if np.isfinite(m).all():
        assert np.isfinite(g).all()
    # not vacuous: what the case is about shows in the frame
    if name == "max_depth_-1":
        assert not g.any() and segs == 0 and smp == 0
        return
    assert smp == E.W * E.H * E.SPP and segs >= smp
    if name == "albedo_negative":
        r, _, _ = E.ref64(name)
        assert r.min() < 0 <= g.min() and g.max() <= 1
    if name == "albedo_saturating":
        r, _, _ = E.ref64(name)
        assert r.max() > 256 >= g.max() and g.max() > 16
    if name.startswith("albedo_gt1"):
        assert g.max() > 1
    if "scale" in meta:
        k = meta["scale"]
        if k <= -40:
            assert smp < segs <= 2 * smp        # bounced rays meet nothing (t-min 1e-3 of |d| ~ 1)
        if k == 63:
            assert segs == smp                  # |d| = inf: no primary ray meets a body
    elif name not in ("ties", "ties_big", "ties_big_glass"):
        assert segs >= 2 * smp                  # the bodies fill the frame: paths go on
    if name in E.FP64_NAMES and samplers == "direct":
        r, rsegs, rsmp = E.ref64(name)
        assert rsmp == smp and np.isfinite(g).all()
        stt = compare(r, rsegs / rsmp, g, st["segments"] / st["samples"], by=E.BY)
        print(f"{name}: kernel vs fp64 same-draw reference: {stt}")
        ok = within(stt, BOUNDS)
        assert all(ok.values()), (name, ok, stt)


@pytest.mark.parametrize("name,samplers", CASES)
def test_bvh_variants_equal_scan(gpu_lib, name, samplers):
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    out = {}
    for v in (5,) + BVH_VARIANTS:
        with variant(v) as dll:
            runs = 16 if (v in COMPACT and not meta["unit"]) else v
            assert _launch_variant(dll, sc, E.W, E.H, p["spp"], p["max_depth"]) == runs, (name, v)
            g, st = _render(sc, cam, meta, samplers, library=dll)
        out[v] = (g, st["segments"], st["samples"])
    ref, segs, smp = out[5]
    m, msegs, msmp = E.mirror(name, rejection=samplers == "rejection")
    assert _same(ref, m) and (segs, smp) == (msegs, msmp), (name, "scan", _differing(ref, m))
    for v in BVH_VARIANTS:
        g, sg, sm = out[v]
        assert _same(g, ref), (name, samplers, v, _differing(g, ref))
        assert (sg, sm) == (segs, smp), (name, samplers, v, sg, segs)


def test_ties_first_twin_wins_in_every_variant(gpu_lib):
    """ties at max_depth 2 (the smallest depth at which the primary hit's
    winner shows; at 1 every hit is black before its material is read, and
    that frame is compared too): every variant's frame equals the one of the
    scene whose later twins have no material, and the mirror's."""
    sc, cam, meta = E.case("ties")
    first, first_lamb = E.ties_keep_one(sc, meta["group"])
    last, _ = E.ties_keep_one(sc, meta["group"], last=True)
    for depth in (1, 2):
        m, msegs, _ = E.mirror("ties", max_depth=depth)
        for v in (0, 5) + BVH_VARIANTS:
            with variant(v) as dll:
                a, sa = _render(sc, cam, meta, library=dll, max_depth=depth)
                b, sb = _render(first, cam, meta, library=dll, max_depth=depth)
                c, _ = _render(last, cam, meta, library=dll, max_depth=depth)
            assert np.array_equal(a, b) and sa["segments"] == sb["segments"], (depth, v, _differing(a, b))
            assert np.array_equal(a, m) and sa["segments"] == msegs, (depth, v)
            if depth == 2:
                red = (a[..., 0] > 0.1) & (a[..., 1] == 0) & (a[..., 2] == 0)
                assert red.sum() > 20 * len(first_lamb) and not np.array_equal(a, c), v


def test_sharded_render_with_a_high_bit_seed(gpu_lib):
    """Seed 2^63 + 1 through rt_render's fan-out (three shards on device 0):
    the sharded frame equals the unsharded one and the mirror."""
    from rtclj._lib import RT_FLAG_SHARDS_ON_DEVICE0
    name = "seed_2^63+1"
    sc, cam, meta = E.case(name)
    whole, st = _render(sc, cam, meta)
    shards, st3 = _render(sc, cam, meta, flags=RT_FLAG_SHARDS_ON_DEVICE0, n_devices=3)
    assert st3["n_devices"] == 3
    assert np.array_equal(whole, shards) and st["segments"] == st3["segments"]
    assert np.array_equal(whole, E.mirror(name)[0])
    assert not np.array_equal(whole, E.mirror(name, seed=1)[0])


ACCUM_CASES = ["albedo_gt1", "albedo_gt1_metal", "albedo_negative", "albedo_saturating", "eta_inf", "nonfinite_65",
               "ties_big", "scale_2^-62", "scale_2^63", "seed_2^64-1", "sample_begin_2^32-8"]


@pytest.mark.parametrize("name", ACCUM_CASES)
def test_accumulated_passes_equal_mirror(gpu_lib, name):
    """rt_launch_accum at the edges: the case's 16 samples in passes of 5 + 11
    into one rt_accum -- on one stream, and again with the two passes on two
    streams -- resolved into a NaN-filled buffer, equal the mirror's frame
    (NaN == NaN), and the counters its segments and samples.  Where an albedo
    leaves [-1, 1] the passes add through the u64 epilogue (global atomics)."""
    import ctypes as C

    import torch
    from rtclj._lib import lib, rt_params
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    m, segs, smp = E.mirror(name)
    ds = C.c_void_p()
    assert lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)) == 0, lib.rt_last_error()

    def params(spp, begin):
        return rt_params(width=E.W, height=E.H, row_begin=0, row_end=E.H, spp=spp, max_depth=p["max_depth"],
                         seed=p["seed"], sample_begin=begin)
    try:
        for streams in (1, 2):
            ss = [torch.cuda.Stream() for _ in range(streams)]
            acc = C.c_void_p()
            assert lib.rt_accum_create(ds, C.byref(params(16, p["sample_begin"])), C.byref(acc)) == 0, lib.rt_last_error()
            try:
                cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
                out = torch.full((E.H * E.W * 3 + 3,), float("nan"), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                begin = p["sample_begin"]
                for i, n in enumerate((5, 11)):     # (both enqueued before either is waited for)
                    rc = lib.rt_launch_accum(ds, C.byref(cam), C.byref(params(n, begin)), acc, C.c_void_p(cnt.data_ptr()),
                                             C.c_void_p(ss[i % streams].cuda_stream))
                    assert rc == 0, lib.rt_last_error()
                    begin += n
                torch.cuda.synchronize()
                assert lib.rt_accum_samples(acc) == 16
                rc = lib.rt_accum_resolve(acc, 0, C.c_void_p(out.data_ptr()), C.c_void_p(ss[0].cuda_stream))
                assert rc == 0, lib.rt_last_error()
                torch.cuda.synchronize()
                f = out.cpu().numpy()
                assert np.isnan(f[-3:]).all()               # the guard behind the frame
                g = f[:-3].reshape(E.H, E.W, 3)
                assert _same(g, m), (name, streams, _differing(g, m))
                assert cnt.cpu().numpy().tolist() == [segs, smp], (name, streams)
                if np.isfinite(m).all():
                    assert np.isfinite(g).all()
            finally:
                lib.rt_accum_free(acc)
    finally:
        lib.rt_scene_free(ds)
    # not vacuous
    if name.startswith("albedo_gt1") or name == "albedo_saturating":
        assert not meta["unit"] and m.max() > 1
    if name == "scale_2^63":
        assert segs == smp


@pytest.mark.parametrize("name", ["albedo_saturating", "albedo_negative"])
def test_render_u8_clamps_as_rt_quantize(gpu_lib, name):
    """rt_render_u8 on frames that leave [0, 1]: exactly rt_quantize's bytes
    of the float frame, 255 where it clamps above and 0 where the samples
    were negative."""
    from rtclj import raytracing as R
    sc, cam, meta = E.case(name)
    lin, _ = _render(sc, cam, meta)
    u8, _ = _render(sc, cam, meta, u8=True)
    assert u8.dtype == np.uint8 and np.array_equal(u8, R.write_color(lin))
    if name == "albedo_saturating":
        assert (lin > 1).sum() > 100 and (u8[lin > 1] == 255).all()
    else:
        assert (lin == 0).sum() > 100 and (u8[lin == 0] == 0).all() and lin.min() == 0
