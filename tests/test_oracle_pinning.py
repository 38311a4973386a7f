"""Oracle pinning, part 2: the oracle against the reference's own output.

The reference's only hot-path fixture is scene.ppm (400x225, 100 spp,
depth 50; unseeded java.util.Random), committed as tests/golden/scene_ppm.npz
with its statistics in scene_ppm_stats.json.  Tolerances (SURVEY.md §8c,
measured noise floor in brackets):
  16x9 block means (8-bit): mean |d| <= 0.25 [0.149], max |d| <= 2.5 [1.72]
  whole-image mean: within 0.15 per channel [0.03]
  neighbour-difference std: within 0.15 of scene.ppm's (pins spp)
  per-pixel mean |d| <= 3.5 [3.23]
The book's normalised-metal variant must FAIL these (fixture discriminates).

The same frame also pins the kernel's default contract (MODE_MIRROR32 |
DIRECT) against its same-draw fp64 reference MODE_REF64D (the Clojure path in
double with the two samplers loop-free in plain double, from the same
uniforms), with oracle/pin.py's same-draw BOUNDS: measured linear mean |d|
2.5e-6 (<= 5e-4), 8-bit per-pixel 7e-4 (<= 0.25), off by > 1 0.008 % (<= 2 %),
block means 5e-4 / 0.013, segments/sample 1.6e-6.  With the fp64 sphere
draw's z scaled by 0.99 the linear mean is 7.5e-4 and off by > 1 2.02 %: fails.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import oracle

G = Path(__file__).parent / "golden"
STATS = json.loads((G / "scene_ppm_stats.json").read_text())
PIX = np.load(G / "scene_ppm.npz")["pixels"]


def stats(img):
    img = img.astype(np.float64)
    h, w = img.shape[:2]
    blocks = np.array([[img[y * h // 9:(y + 1) * h // 9, x * w // 16:(x + 1) * w // 16].reshape(-1, 3).mean(0)
                        for x in range(16)] for y in range(9)])
    return img.reshape(-1, 3).mean(0), blocks, np.diff(img, axis=1).reshape(-1, 3).std(0)


def within_tolerance(rgb8):
    mean, blocks, nbr = stats(rgb8)
    d = np.abs(blocks - np.array(STATS["blocks"]))
    checks = {
        "block_mean": d.mean() <= 0.25,
        "block_max": d.max() <= 2.5,
        "image_mean": bool((np.abs(mean - np.array(STATS["mean"])) <= 0.15).all()),
        "nbr_std": bool((np.abs(nbr - np.array(STATS["nbr_std"])) <= 0.15).all()),
        "pixel_mean": np.abs(rgb8.astype(np.float64) - PIX.astype(np.float64)).mean() <= 3.5,
    }
    return checks, dict(block_mean=d.mean(), block_max=d.max(), mean=mean.tolist(), nbr=nbr.tolist())


def test_fixture_matches_its_stats():
    mean, blocks, nbr = stats(PIX)
    assert PIX.shape == (225, 400, 3)
    assert np.allclose(mean, STATS["mean"]) and np.allclose(blocks, STATS["blocks"]) and np.allclose(nbr, STATS["nbr_std"])


def _render(mode, seed=1, spp=100, zscale=1.0):
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten64(R.hittables)
    cam = oracle.camera(400, 225, **R.REFERENCE_CAMERA)
    oracle.sampler_bias(zscale)   # test-only negative control; 1 = unbiased
    try:
        out, _, segs, smp = oracle.render(mode, sph, kind, mat, cam, 1, 400, 225, spp, 50, seed=seed)
    finally:
        oracle.sampler_bias(1.0)
    return out, segs / smp


@pytest.fixture(scope="module")
def ref64():
    return _render(oracle.MODE_REF64)


def _q(lin):
    return np.array([[[oracle.quantize(float(c)) for c in px] for px in row] for row in lin], np.uint8) \
        if lin.size < 1000 else _vq(lin)


def _vq(lin):
    g = np.where(lin > 0, np.sqrt(np.maximum(lin.astype(np.float64), 0)), 0.0)
    return (256 * np.clip(g, 0.0, 0.999)).astype(np.int64).astype(np.uint8)


def test_vectorised_quantiser_matches_oracle():
    x = np.random.default_rng(1).uniform(-0.2, 1.3, 5000).astype(np.float32)
    assert np.array_equal(_vq(x), np.array([oracle.quantize(float(v)) for v in x], np.uint8))


def test_ref64_reproduces_scene_ppm(ref64):
    lin, seg = ref64
    ok, info = within_tolerance(_vq(lin))
    assert all(ok.values()), (ok, info)
    assert seg == pytest.approx(3.675, abs=0.02)   # SURVEY.md §3.2 probe: 3.675 segments/sample


def test_mirror32_reproduces_scene_ppm_and_tracks_ref64(ref64):
    lin32, seg32 = _render(oracle.MODE_MIRROR32)
    ok, info = within_tolerance(_vq(lin32))
    assert all(ok.values()), (ok, info)
    lin64, seg64 = ref64
    # same keyed RNG stream: paths agree except fp32 near-boundary decisions
    assert abs(seg32 - seg64) / seg64 < 2e-3
    assert np.abs(lin32 - lin64).mean() < 1e-4


@pytest.mark.parametrize("seed", [1, 2])
def test_direct_sampler_mirror_reproduces_scene_ppm(seed):
    """The kernel's default contract -- the fp32 mirror with the loop-free
    samplers (MODE_MIRROR32 | DIRECT; include/rt.h
    RT_FLAG_REJECTION_SAMPLERS) -- against the reference's own scene.ppm with
    the same SURVEY.md §8c tolerances (measured: block means 0.136 / 1.18 at
    seed 1, 0.141 / 2.00 at seed 2; the rejection mirror 0.140 / 1.59,
    0.150 / 1.67)."""
    lin, seg = _render(oracle.MODE_MIRROR32 | oracle.DIRECT, seed=seed)
    ok, info = within_tolerance(_vq(lin))
    assert all(ok.values()), (ok, info)
    assert seg == pytest.approx(3.675, abs=0.02)


def test_direct_sampler_mirror_tracks_ref64d():
    """The default contract against its same-draw fp64 reference (module
    docstring), and the negative control: a 1 % bias of the fp64 unit-sphere
    draw fails the same bounds."""
    from oracle.pin import compare, within
    lin32, seg32 = _render(oracle.MODE_MIRROR32 | oracle.DIRECT)
    lin64, seg64 = _render(oracle.MODE_REF64D)
    st = compare(lin64, seg64, lin32, seg32, by=9)
    print("reference scene MIRROR32|DIRECT vs REF64D:", st)
    ok = within(st)
    assert all(ok.values()), (ok, st)
    assert seg64 == pytest.approx(3.675, abs=0.02)
    bias, segb = _render(oracle.MODE_REF64D, zscale=0.99)
    assert oracle.sampler_bias() == 1.0
    st = compare(bias, segb, lin32, seg32, by=9)
    print("the same, z * 0.99:", st)
    ok = within(st)
    assert not all(ok.values()) and not ok["lin_mean"], (ok, st)


def test_book_metal_variant_is_rejected():
    """Negative control: normalising d before the metal
    reflect (the book's code) must not pass the scene.ppm tolerance."""
    lin, _ = _render(oracle.MODE_BOOK64)
    ok, info = within_tolerance(_vq(lin))
    assert not all(ok.values()), info
    assert info["block_max"] > 5.0


@pytest.mark.parametrize("name,direct", [("mirror_small.npz", 0), ("mirror_small_direct.npz", 0x30)])
def test_mirror_small_fixture_regression(name, direct):
    """The committed mirror renders (tests/golden/make_golden.py): with the
    rejection samplers and with the kernel's default loop-free ones."""
    from rtclj import raytracing as R
    from rtclj import scenes
    f = np.load(G / name)
    sc = R.Scene.from_bodies(R.hittables)
    cam = R.camera(48, 27, **R.REFERENCE_CAMERA)
    out, _, segs, _ = oracle.render(oracle.MODE_MIRROR32 | direct, sc.sphere.astype(np.float64), sc.kind,
                                    sc.mat.astype(np.float64), cam.as_list(), cam.defocus, 48, 27, 8, 50, seed=3)
    assert np.array_equal(out, f["reference_48x27_spp8_seed3"]) and segs == f["segments"][0]
    cs = scenes.cover(11)
    cc = scenes.cover_camera(32, 18)
    out, _, segs, _ = oracle.render(oracle.MODE_MIRROR32 | direct, cs.sphere.astype(np.float64), cs.kind,
                                    cs.mat.astype(np.float64), cc.as_list(), cc.defocus, 32, 18, 4, 50, seed=5)
    assert np.array_equal(out, f["cover_32x18_spp4_seed5"]) and segs == f["segments"][1]


def test_oracle_threading_and_row_step_invariance():
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten64(R.hittables)
    cam = oracle.camera(60, 33, **R.REFERENCE_CAMERA)
    a = oracle.render(oracle.MODE_MIRROR32, sph, kind, mat, cam, 1, 60, 33, 4, 20, nthreads=1)[0]
    b = oracle.render(oracle.MODE_MIRROR32, sph, kind, mat, cam, 1, 60, 33, 4, 20, nthreads=7)[0]
    c = oracle.render(oracle.MODE_MIRROR32, sph, kind, mat, cam, 1, 60, 33, 4, 20, row_step=4, rows=(2, 33))[0]
    assert np.array_equal(a, b) and np.array_equal(a[2::4], c)


def test_oracle_edge_cases():
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten64(R.hittables)
    cam = oracle.camera(8, 5, **R.REFERENCE_CAMERA)
    for mode in (oracle.MODE_REF64, oracle.MODE_MIRROR32):
        z, _, segs, _ = oracle.render(mode, sph, kind, mat, cam, 1, 8, 5, 4, 0)
        assert not z.any() and segs == 0                      # depth 0 -> black
        z, _, _, _ = oracle.render(mode, sph, kind, mat, cam, 1, 8, 5, 0, 50)
        assert not z.any()                                    # spp 0 -> black (defined)
        sky, _, segs, _ = oracle.render(mode, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 4)), cam, 1, 8, 5, 2, 50)
        assert segs == 8 * 5 * 2 and (sky > 0.4).all()        # empty world: 1 segment, sky
    with pytest.raises(ValueError):
        oracle.render(oracle.MODE_REF64, sph, kind, mat, cam, 1, 8, 5, 1, 1, rows=(0, 6))
