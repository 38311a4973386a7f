"""The feature-guided denoiser on the device (include/rt.h, rt_denoise): the
kernels give rt_denoise_host's bits for random inputs and for the real
pipeline's, whatever the stream; interleaved shards gathered on the host give
the unsharded result; rt_adapt_resolve_half feeds it an adaptive frame's two
halves; and the hosts (render_denoised, rt_main --denoise).  Every output
buffer is NaN-filled first: no NaN may remain.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_denoise_host import SIZES, bits, random_inputs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_MAIN = ROOT / "raytracing-clj_amd" / "lib" / "rt_main"
W, H = 160, 90


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R
    e = Env()
    e.torch, e.R = torch, R
    e.sc = R.Scene.from_bodies(R.hittables)
    e.cam = R.camera(W, H, **R.REFERENCE_CAMERA)
    return e


def dev(env, a):
    """A host array on the device (flat float32)."""
    t = env.torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
    env.torch.cuda.synchronize()
    return t


def nan_buf(env, n):
    t = env.torch.full((int(n),), float("nan"), dtype=env.torch.float32, device="cuda")
    env.torch.cuda.synchronize()
    return t


def run_device(env, half0, half1, feat, stream=None, dn=None, **opts):
    """Denoiser.run on host arrays -> (rows, width, 3), the inputs checked unchanged."""
    rows, width = half0.shape[:2]
    d0, d1, df = dev(env, half0), dev(env, half1), dev(env, feat)
    out = nan_buf(env, rows * width * 3)
    own = dn is None
    dn = dn or env.R.Denoiser(width, rows)
    try:
        dn.run(d0.data_ptr(), d1.data_ptr(), df.data_ptr(), out.data_ptr(),
               stream=stream.cuda_stream if stream is not None else None, **opts)
        env.torch.cuda.synchronize()
    finally:
        if own:
            dn.close()
    got = out.cpu().numpy().reshape(rows, width, 3)
    assert not np.isnan(got).any()
    for d, a in ((d0, half0), (d1, half1), (df, feat)):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a).reshape(-1))   # the inputs are never written
    return got


# ---- device == host, bit for bit -------------------------------------------
@pytest.mark.parametrize("rows,width", SIZES + ((64, 64), (3, 257), (257, 3)))
def test_device_equals_host(env, rows, width):
    half0, half1, feat = random_inputs(rows, width, seed=1000 * rows + width)
    with env.R.Denoiser(width, rows) as dn:
        for levels in (1, 5, 8):
            got = run_device(env, half0, half1, feat, dn=dn, levels=levels)
            want = env.R.denoise_host(half0, half1, feat, levels=levels)
            assert np.array_equal(bits(got), bits(want)), (levels, int((bits(got) != bits(want)).sum()))
        got = run_device(env, half0, half1, feat, dn=dn, normal_pow2=0, sigma_c=0.5, sigma_z=1.0)
        assert np.array_equal(bits(got), bits(env.R.denoise_host(half0, half1, feat, normal_pow2=0, sigma_c=0.5,
                                                                 sigma_z=1.0)))


def test_device_argument_errors(env):
    from rtclj._lib import lib, rt_denoise_opts
    half0, half1, feat = random_inputs(9, 12, seed=2)
    d0, d1, df = dev(env, half0), dev(env, half1), dev(env, feat)
    out = nan_buf(env, half0.size)
    with env.R.Denoiser(12, 9) as dn:
        p = [C.c_void_p(t.data_ptr()) for t in (d0, d1, df, out)]
        for k in range(4):
            bad = list(p)
            bad[k] = None
            assert lib.rt_denoise(dn._dn, None, *bad, None) == -1 and b"NULL" in lib.rt_last_error()
        assert lib.rt_denoise(dn._dn, C.byref(rt_denoise_opts(0, 5, 4.0, 0.05)), *p, None) == -1
        for k in range(3):   # d_out may not overlap an input
            assert lib.rt_denoise(dn._dn, None, p[0], p[1], p[2], p[k], None) == -1
            assert b"overlaps" in lib.rt_last_error()
        assert lib.rt_denoise(dn._dn, None, *p, None) == 0
        env.torch.cuda.synchronize()
    h = C.c_void_p()
    assert lib.rt_denoiser_create(lib.rt_device_count(), 8, 8, C.byref(h)) == -5 and not h.value


# ---- the real pipeline ------------------------------------------------------
@pytest.fixture(scope="module")
def pipeline(env):
    """render_denoised's steps at 160 x 90, 4 + 4 spp, seed 5: the device
    buffers and what they hold."""
    R, torch = env.R, env.torch
    p = Env()
    p.d_h = [nan_buf(env, W * H * 3) for _ in range(2)]
    p.d_feat = nan_buf(env, W * H * 8)
    with R.Progressive(env.sc, env.cam, W, H, seed=5) as a0, \
            R.Progressive(env.sc, env.cam, W, H, seed=5, sample_begin=4) as a1, \
            R.Features(env.sc, env.cam, W, H, seed=5) as ft:
        a0.add(4)
        a1.add(4)
        ft.add(8)
        a0.resolve_into(p.d_h[0].data_ptr())
        a1.resolve_into(p.d_h[1].data_ptr())
        ft.resolve_into(p.d_feat.data_ptr())
        torch.cuda.synchronize()
    p.h0, p.h1 = (d.cpu().numpy().reshape(H, W, 3) for d in p.d_h)
    p.feat = p.d_feat.cpu().numpy().reshape(H, W, 8)
    assert not any(np.isnan(a).any() for a in (p.h0, p.h1, p.feat))
    p.want = R.denoise_host(p.h0, p.h1, p.feat)
    return p


def test_pipeline_equals_host(env, pipeline):
    p, torch = pipeline, env.torch
    with env.R.Denoiser(W, H) as dn:
        outs = []
        for stream in (None, None, torch.cuda.Stream()):
            out = nan_buf(env, W * H * 3)
            torch.cuda.synchronize()   # (the side stream's call comes after the passes)
            dn.run(p.d_h[0].data_ptr(), p.d_h[1].data_ptr(), p.d_feat.data_ptr(), out.data_ptr(),
                   stream=stream.cuda_stream if stream is not None else None)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy().reshape(H, W, 3))
    for got in outs:   # the first call, a second one, one on a side stream
        assert not np.isnan(got).any()
        assert np.array_equal(bits(got), bits(p.want))
    # the inputs read back unchanged
    for d, a in ((p.d_h[0], p.h0), (p.d_h[1], p.h1), (p.d_feat, p.feat)):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a).reshape(-1))


def test_pipeline_quality(env, pipeline):
    """Against a 1024-spp rt_launch frame at another seed the MSE falls below
    half of the 8-spp frame's (DESIGN.md §3.8 records the printed value)."""
    p = pipeline
    ref = env.R.render(env.sc, env.cam, W, H, spp=1024, seed=77, n_devices=1).astype(np.float64)
    mean = np.float32(0.5) * (p.h0 + p.h1)
    ratio = float(((p.want - ref) ** 2).mean() / ((mean - ref) ** 2).mean())
    print("MSE(denoised) / MSE(mean of halves), device pipeline, 4 + 4 spp: %.4f" % ratio)
    assert ratio < 0.5, ratio


def test_interleaved_shards(env, pipeline):
    """Two interleaved shards (tile_step = 2), gathered on the host into one
    frame, denoise to what the unsharded inputs give."""
    from rtclj.shard import shard_rows
    R, torch = env.R, env.torch
    parts = {"h0": [], "h1": [], "feat": []}
    for first in (0, 1):
        rows = shard_rows(H, 8, first, 2)
        kw = dict(seed=5, tile_first=first, tile_step=2)
        with R.Progressive(env.sc, env.cam, W, H, **kw) as a0, \
                R.Progressive(env.sc, env.cam, W, H, sample_begin=4, **kw) as a1, \
                R.Features(env.sc, env.cam, W, H, **kw) as ft:
            a0.add(4)
            a1.add(4)
            ft.add(8)
            for key, a in (("h0", a0.frame()), ("h1", a1.frame()), ("feat", ft.frame())):
                assert a.shape[0] == len(rows)
                parts[key].append((rows, a))
    full = {}
    for key, ps in parts.items():
        full[key] = np.empty((H, W, ps[0][1].shape[2]), np.float32)
        for rows, a in ps:
            full[key][rows] = a
    p = pipeline
    for key, a in (("h0", p.h0), ("h1", p.h1), ("feat", p.feat)):
        assert np.array_equal(bits(full[key]), bits(a)), key
    got = run_device(env, full["h0"], full["h1"], full["feat"])
    assert np.array_equal(bits(got), bits(p.want))


# ---- the edge scenes' pipelines -----------------------------------------------
def _edge_cases():
    import feat_oracle
    return feat_oracle.DENOISE_CASES


@pytest.mark.parametrize("name", _edge_cases())
def test_edge_pipelines(env, name):
    """tests/test_denoise_host.py's edge pipelines on the device: Progressive
    x 2 and Features, resolved on the device, reproduce the oracle's inputs
    bit for bit, and Denoiser.run equals the host on them at levels 1, 5, 8."""
    import edge_scenes as E
    import feat_oracle
    R, torch = env.R, env.torch
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    half0, half1, feat = feat_oracle.denoise_inputs(name)
    d_h = [nan_buf(env, E.W * E.H * 3) for _ in range(2)]
    d_feat = nan_buf(env, E.W * E.H * 8)
    kw = dict(seed=p["seed"])
    with R.Progressive(sc, cam, E.W, E.H, max_depth=p["max_depth"], **kw) as a0, \
            R.Progressive(sc, cam, E.W, E.H, max_depth=p["max_depth"], sample_begin=8, **kw) as a1, \
            R.Features(sc, cam, E.W, E.H, **kw) as ft:
        a0.add(8)
        a1.add(8)
        ft.add(16)
        a0.resolve_into(d_h[0].data_ptr())
        a1.resolve_into(d_h[1].data_ptr())
        ft.resolve_into(d_feat.data_ptr())
        torch.cuda.synchronize()
    for d, a, what in ((d_h[0], half0, "half0"), (d_h[1], half1, "half1"), (d_feat, feat, "feat")):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a).reshape(-1)), (name, what)
    with R.Denoiser(E.W, E.H) as dn:
        for levels in (1, 5, 8):
            out = nan_buf(env, E.W * E.H * 3)
            dn.run(d_h[0].data_ptr(), d_h[1].data_ptr(), d_feat.data_ptr(), out.data_ptr(), levels=levels)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(E.H, E.W, 3)
            want = R.denoise_host(half0, half1, feat, levels=levels)
            assert np.isfinite(got).all(), (name, levels)
            assert np.array_equal(bits(got), bits(want)), (name, levels, int((bits(got) != bits(want)).sum()))


def test_unspecified_inputs_stay_local(env):
    """40 x 33, 2 levels: a 4 x 4 corner block of NaN, +-inf, negative
    colours, depth 0, negative depth, denormals and 3e38.  rt.h leaves the
    numbers there unspecified; the call returns 0, and no pixel more than 8
    pixels (Chebyshev) from the block differs from the host's bits: levels 0
    and 1 reach 2 + 4 = 6 pixels.  The agreement inside that reach is printed."""
    from rtclj._lib import lib, rt_denoise_opts
    rows, width = 40, 33
    half0, half1, feat = (a.copy() for a in random_inputs(rows, width, seed=77))
    nan, inf, den = np.float32("nan"), np.float32("inf"), np.float32(1e-42)
    half0[0, 0], half0[0, 1], half0[0, 2], half0[0, 3] = nan, inf, -inf, (-1.0, -2.0, -0.5)
    half1[1, 0], half1[1, 1], half1[1, 2], half1[1, 3] = (3e38, 3e38, 3e38), den, (nan, 1.0, inf), -inf
    half0[2, 0], half1[2, 0] = 3e38, 3e38
    half0[2, 1], half1[2, 1] = den, den
    feat[2, 2, 6], feat[2, 3, 6], feat[3, 0, 6], feat[3, 1, 6] = 0.0, -4.0, nan, den       # depths
    feat[3, 2, 3:6], feat[3, 3, 3:6], feat[0, 0, 7], feat[1, 1, 7] = nan, (inf, -inf, 3e38), nan, -inf
    feat[0, 2, 0:3], feat[1, 3, 0:3], feat[2, 0, 0:3] = (nan, -1.0, den), inf, 3e38
    d0, d1, df = dev(env, half0), dev(env, half1), dev(env, feat)
    out = nan_buf(env, rows * width * 3)
    with env.R.Denoiser(width, rows) as dn:
        o = rt_denoise_opts(levels=2, normal_pow2=5, sigma_c=4.0, sigma_z=0.05)
        rc = lib.rt_denoise(dn._dn, C.byref(o), *(C.c_void_p(t.data_ptr()) for t in (d0, d1, df, out)), None)
        assert rc == 0, lib.rt_last_error()
        env.torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(rows, width, 3)
    want = env.R.denoise_host(half0, half1, feat, levels=2)
    y, x = np.mgrid[0:rows, 0:width]
    far = np.maximum(y - 3, x - 3) > 8
    assert far.sum() > rows * width // 2
    assert np.isfinite(want[far]).all() and np.array_equal(bits(got[far]), bits(want[far]))
    near = ~far
    same = ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(-1)
    print(f"inside the block's reach: {same[near].mean():.2%} of {int(near.sum())} pixels agree with the host")


# ---- rt_adapt_resolve_half --------------------------------------------------
def test_adapt_halves(env):
    from rtclj._lib import RT_FLAG_REALM, fptr, lib, u32ptr, u64ptr
    R, torch = env.R, env.torch
    w, h = 64, 40
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    with R.Adaptive(env.sc, cam, w, h, tol_q16=6000, step=2, min_spp=4, max_spp=16, seed=5) as ad:
        ad.run()
        counts = ad.counts()
        assert len(np.unique(counts)) > 1, counts          # the tiles' counts differ
        h0, h1 = ad.halves()
        zeros = np.zeros_like(h0)
        half_counts = np.ascontiguousarray(counts // 2, np.uint32)
        halves = {}
        for flags in (0, RT_FLAG_REALM):
            for half, hs in ((0, h0), (1, h1)):
                want = np.empty(ad.shape, np.float32)
                assert lib.rt_adapt_resolve_host(u64ptr(hs), u64ptr(zeros), u32ptr(half_counts), w, h, flags,
                                                 fptr(want)) == 0
                out = nan_buf(env, want.size)
                assert lib.rt_adapt_resolve_half(ad._ad, half, flags, C.c_void_p(out.data_ptr()), None) == 0
                torch.cuda.synchronize()
                got = out.cpu().numpy().reshape(ad.shape)
                assert not np.isnan(got).any()
                assert np.array_equal(bits(got), bits(want)), (flags, half)
                halves[flags, half] = got
        for bad in (-1, 2):
            assert lib.rt_adapt_resolve_half(ad._ad, bad, 0, C.c_void_p(out.data_ptr()), None) == -1
        # the two halves' mean is the frame, to the ulp's scale: with u = 2^-24,
        # each half carries two roundings (float(sum), the division) and their
        # sum a third (the halving is exact): the mean lies within 3 u of
        # (H0 + H1) 2^-24 / count, relatively, the frame within 2 u, and
        # u * v < ulp(v): 5 ulp (of the larger of the two) bound the difference
        frame = ad.frame()
        a, b = halves[0, 0], halves[0, 1]
        mean = np.float32(0.5) * (a + b)
        assert (np.abs(mean.astype(np.float64) - frame) <= 5 * np.spacing(np.maximum(frame, mean))).all()
        # Python's resolve_half_into, then the filter on those halves
        d = [nan_buf(env, a.size) for _ in range(2)]
        ad.resolve_half_into(d[0].data_ptr(), 0)
        ad.resolve_half_into(d[1].data_ptr(), 1)
        with R.Features(env.sc, cam, w, h, seed=5) as ft:
            ft.add(8)
            feat = ft.frame()
        df = dev(env, feat)
        out = nan_buf(env, a.size)
        with R.Denoiser(w, h) as dn:
            dn.run(d[0].data_ptr(), d[1].data_ptr(), df.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(ad.shape)
        assert not np.isnan(got).any()
        assert np.array_equal(bits(d[0].cpu().numpy()), bits(a).reshape(-1))
        assert np.array_equal(bits(got), bits(R.denoise_host(a, b, feat)))


# ---- hosts ------------------------------------------------------------------
def test_render_denoised_and_rt_main(env, tmp_path):
    import pngdec
    R = env.R
    den, mean, feat = R.render_denoised(env.sc, env.cam, W, H, spp=8, seed=3)
    assert den.shape == (H, W, 3) and mean.shape == (H, W, 3) and feat.shape == (H, W, 8)
    assert den.dtype == mean.dtype == feat.dtype == np.float32
    assert np.isfinite(den).all() and np.isfinite(mean).all()
    # the halves together are the frame's own rays: their mean is the 8-spp frame up to the halves' rounding
    frame = R.render(env.sc, env.cam, W, H, spp=8, seed=3, n_devices=1)
    assert np.allclose(mean, frame, rtol=1e-6, atol=1e-7)
    assert RT_MAIN.exists(), "lib/rt_main is not built (make -C raytracing-clj_amd)"
    child = dict(os.environ)
    child.pop("RTCLJ_LIBRARY", None)
    r = subprocess.run([str(RT_MAIN), "8", "50", "--width", str(W), "--gpus", "1", "--no-png", "--seed", "3",
                        "--denoise", "dn"], cwd=tmp_path, capture_output=True, text=True, timeout=120, env=child)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    want = R.write_color(den)
    assert np.array_equal(R.read_ppm(tmp_path / "dn.denoised.ppm"), want)
    png, _ = pngdec.decode((tmp_path / "dn.denoised.png").read_bytes())
    assert np.array_equal(png, want)
    r = subprocess.run([str(RT_MAIN), "7", "50", "--width", str(W), "--gpus", "1", "--no-png", "--denoise", "odd"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120, env=child)
    assert r.returncode != 0 and "even" in r.stderr
    assert not (tmp_path / "odd.denoised.ppm").exists()
