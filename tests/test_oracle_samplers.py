"""The kernel's loop-free samplers (include/rt.h RT_FLAG_REJECTION_SAMPLERS;
trace_kernel.h sphere_direct / disk_direct / turn24), through their fp32
restatement in the oracle, against the reference's rejection samplers
(vec3a.clj:74-79 random-unit-vec3, :81-86 random-in-unit-disk).

The contract is the same distributions: uniform on the
unit sphere, uniform in the unit disk.  The reference draws from the
unseeded java.util.Random, so no bitwise equality with it exists; these tests
pin the distributions directly and then the renders they make:

  * turn24's (cos, sin) of 2 pi u / 2^24 against double-precision math for
    every quarter-turn boundary and a dense sweep: |error| <= 2e-7;
  * 2^20 draws of each sampler: unit length (sphere) / inside the disk;
    z, r^2 and phi uniform (chi-square over 64 bins, p > 1e-4); the second
    moments 1/3 (sphere) and 1/4 (disk) within 5 sigma; the direct and the
    rejection samplers' z and r^2 indistinguishable (two-sample
    Kolmogorov-Smirnov, p > 1e-4);
  * the reference scene rendered by the fp32 mirror with the direct samplers
    against MODE_REF64 (the Clojure path in double, rejection samplers) at
    400 spp, 200x112: 16x9 block means of the linear image within 1e-3 mean
    and 8e-3 max of each other and segments/sample within 1e-3 -- about
    twice the seed-to-seed noise floor of REF64 itself, measured 6.2e-4 /
    4.5e-3 / 1.1e-4 (the direct mirror: 6.1e-4 / 4.9e-3 / 2.3e-4); the book's
    normalised-metal control (MODE_BOOK64) is far outside (1.0e-2 / 0.18 /
    1.6e-2).
  * turn24 over all 2^24 inputs, and the fp32 samplers draw by draw against
    their definition in plain double (oracle MODE_REF64D's samplers: z = 2
    xi1 - 1 or r = sqrt(xi1), the angle 2 pi u / 2^24, libm) from the same
    uniforms, every component within 3.5e-7 (derived in the test).
tests/test_oracle_pinning.py holds the direct mirror to the reference's own
scene.ppm with SURVEY.md §8c's tolerances as well.
"""
import os

import numpy as np
import pytest
from scipy import stats

import oracle

N = 1 << 20


def test_turn24_quarter_turns_and_sweep():
    u = np.array([0, 1 << 22, 1 << 23, 3 << 22, (1 << 21) - 1, 1 << 21, (1 << 24) - 1, 0x2aaaab, 0x555555], np.uint32)
    sweep = np.arange(0, 1 << 24, 4099, dtype=np.uint32)
    for uu in (u, sweep):
        got = oracle.turn24(uu).astype(np.float64)
        phi = 2 * np.pi * uu.astype(np.float64) / (1 << 24)
        err = np.abs(got - np.stack([np.cos(phi), np.sin(phi)], 1))
        assert err.max() <= 2e-7, (err.max(), uu[np.argmax(err.max(1))])
    # exact at the quarter turns (the signs ride on r: x = -0 at a quarter turn)
    q = oracle.turn24(np.array([0, 1 << 22, 1 << 23, 3 << 22], np.uint32), r=0.5)
    assert np.array_equal(q, np.array([[0.5, 0], [0, 0.5], [-0.5, 0], [0, -0.5]], np.float32))


def test_turn24_every_input():
    """All 2^24 angles against double cos / sin with the sweep's bound 2e-7
    (measured maximum 7.51e-8), and |cos^2 + sin^2 - 1| <= 6e-7: two
    components each within e = 2e-7 of a unit vector give at most
    2 e (|cos| + |sin|) + 2 e^2 <= 2 sqrt(2) e + 2 e^2 = 5.7e-7 (measured
    1.45e-7)."""
    emax = nmax = 0.0
    for c in range(16):
        u = np.arange(c << 20, (c + 1) << 20, dtype=np.uint32)
        got = oracle.turn24(u).astype(np.float64)
        phi = 2 * np.pi * u.astype(np.float64) / (1 << 24)
        emax = max(emax, np.abs(got - np.stack([np.cos(phi), np.sin(phi)], 1)).max())
        nmax = max(nmax, np.abs((got ** 2).sum(1) - 1).max())
    print("turn24, all 2^24 inputs: max |error|", emax, "max |cos^2 + sin^2 - 1|", nmax)
    assert emax <= 2e-7, emax
    assert nmax <= 6e-7, nmax


# The fp32 samplers against their definition in double, per component:
#   turn24's (cos, sin) within 2e-7 of the exact ones (above), scaled by r <= 1;
#   r: 2 xi1 - 1 is exact in fp32 (xi1 = k / 2^24), fma(-z, z, 1) rounds once
#   (relative 2^-24 of 1 - z^2, i.e. 2^-25 of r) and the square root once more
#   (2^-24), the disk's sqrt(xi1) once: |dr| <= 1.5 * 2^-24 = 8.9e-8;
#   the product r * cos rounds once: 2^-24 = 6.0e-8.
# 2e-7 + 8.9e-8 + 6.0e-8 = 3.5e-7.  z itself is exact.
PER_DRAW = 3.5e-7


def test_direct_samplers_agree_with_their_fp64_definition_draw_by_draw(draws):
    """2^20 draws from the same keyed stream (measured maxima: sphere 1.13e-7,
    disk 1.09e-7)."""
    for k in ("sphere_direct", "disk_direct"):
        d64 = oracle.sampler_draws64(k, 12345, N)
        err = np.abs(draws[k] - d64)
        print(k, "fp32 vs fp64 definition, 2^20 draws: max |d| per component", err.max(0))
        assert err.max() <= PER_DRAW, (k, err.max(), np.argmax(err.max(1)))
        assert (d64[:, 2] == draws[k][:, 2]).all()          # z: exact in fp32 (0 for the disk)
    s64 = oracle.sampler_draws64("sphere_direct", 12345, 4096)
    assert np.abs(np.linalg.norm(s64, axis=1) - 1).max() <= 1e-15
    with pytest.raises(ValueError):
        oracle.sampler_draws64("sphere_rejection", 1, 4)


def test_direct_samplers_at_the_edge_uniforms():
    """The uniforms a random stream hardly visits: xi1 at both ends of its
    range and its middle (the poles and the equator; the disk's centre and
    rim), u at every quarter turn, either side of the first octant boundary
    (where turn24 switches polynomials) and the last angle."""
    xi = np.array([0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24], np.float32)
    u = np.array([0, (1 << 21) - 1, 1 << 21, 1 << 22, 1 << 23, 3 << 22, (1 << 24) - 1], np.uint32)
    X, U = (a.ravel() for a in np.meshgrid(xi, u, indexing="ij"))
    phi = 2 * np.pi * U.astype(np.float64) / (1 << 24)
    for k in ("sphere_direct", "disk_direct"):
        a32, a64 = oracle.direct_from_uniforms(k, X, U)
        err = np.abs(a32.astype(np.float64) - a64)
        print(k, "edge uniforms: max |d|", err.max())
        assert err.max() <= PER_DRAW, (k, err.max(), X[np.argmax(err.max(1))], U[np.argmax(err.max(1))])
        # the fp64 entry point is the definition itself
        x1 = X.astype(np.float64)
        z = 2 * x1 - 1
        r = np.sqrt(1 - z * z) if k == "sphere_direct" else np.sqrt(x1)
        want = np.stack([r * np.cos(phi), r * np.sin(phi), z if k == "sphere_direct" else 0 * z], 1)
        assert np.abs(a64 - want).max() <= 1e-15, k
    # the pole: xi1 = 0 is z = -1, r = 0 in both precisions
    a32, a64 = oracle.direct_from_uniforms("sphere_direct", X[:len(u)], U[:len(u)])
    assert (a32[:, 2] == -1).all() and (a32[:, :2] == 0).all() and (a64[:, 2] == -1).all() and (a64[:, :2] == 0).all()


def test_entry_points_and_the_stream_are_the_same_samplers():
    """direct_from_uniforms fed the keyed stream's own draws gives
    sampler_draws / sampler_draws64 bit for bit (two xorshift steps a call)."""
    n = 4096
    st = oracle.rng_stream(12345, 0, 0, 2 * n)
    xi, u = st[0::2], (st[1::2].astype(np.float64) * (1 << 24)).astype(np.uint32)
    for k in ("sphere_direct", "disk_direct"):
        a32, a64 = oracle.direct_from_uniforms(k, xi, u)
        assert np.array_equal(a32, oracle.sampler_draws(k, 12345, n)), k
        assert np.array_equal(a64, oracle.sampler_draws64(k, 12345, n)), k


def test_sampler_bias_scales_z_of_the_fp64_sphere_draw_only():
    base = oracle.sampler_draws64("sphere_direct", 7, 1024)
    disk = oracle.sampler_draws64("disk_direct", 7, 1024)
    m32 = oracle.sampler_draws("sphere_direct", 7, 1024)
    assert oracle.sampler_bias(0.97) == 1.0
    try:
        b = oracle.sampler_draws64("sphere_direct", 7, 1024)
        assert np.allclose(b[:, 2], 0.97 * base[:, 2], rtol=0, atol=1e-15)
        r = np.sqrt(1 - b[:, 2] ** 2)                          # r formed from the scaled z: still unit length
        assert np.abs(np.hypot(b[:, 0], b[:, 1]) - r).max() <= 1e-15
        assert np.array_equal(oracle.sampler_draws64("disk_direct", 7, 1024), disk)
        assert np.array_equal(oracle.sampler_draws("sphere_direct", 7, 1024), m32)
    finally:
        assert oracle.sampler_bias(1.0) == 0.97
    assert np.array_equal(oracle.sampler_draws64("sphere_direct", 7, 1024), base)


def _chi2_uniform(x, lo, hi, bins=64):
    h, _ = np.histogram(x, bins=bins, range=(lo, hi))
    return stats.chisquare(h).pvalue


@pytest.fixture(scope="module")
def draws():
    return {k: oracle.sampler_draws(k, 12345, N).astype(np.float64) for k in oracle.oracle.SAMPLERS}


def test_sphere_direct_is_uniform_on_the_sphere(draws):
    d = draws["sphere_direct"]
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 1e-6
    assert _chi2_uniform(d[:, 2], -1, 1) > 1e-4                           # Archimedes: z uniform
    assert _chi2_uniform(np.arctan2(d[:, 1], d[:, 0]), -np.pi, np.pi) > 1e-4
    assert _chi2_uniform(d[:, 0], -1, 1) > 1e-4                           # any axis: x uniform too
    sig = np.sqrt(4 / 45 / N)   # std of the mean of x^2 (Var x^2 = 1/5 - 1/9)
    assert (np.abs((d ** 2).mean(0) - 1 / 3) <= 5 * sig).all(), (d ** 2).mean(0)
    assert (np.abs(d.mean(0)) <= 5 * np.sqrt(1 / 3 / N)).all(), d.mean(0)


def test_disk_direct_is_uniform_in_the_disk(draws):
    d = draws["disk_direct"]
    r2 = d[:, 0] ** 2 + d[:, 1] ** 2
    assert (r2 < 1).all() and (d[:, 2] == 0).all()
    assert _chi2_uniform(r2, 0, 1) > 1e-4                                 # r^2 uniform <=> area-uniform
    assert _chi2_uniform(np.arctan2(d[:, 1], d[:, 0]), -np.pi, np.pi) > 1e-4
    sig = np.sqrt((1 / 8 - 1 / 16) / N)   # x^2 of a uniform disk point: mean 1/4, E x^4 = 1/8
    assert (np.abs((d[:, :2] ** 2).mean(0) - 1 / 4) <= 5 * sig).all()


def test_direct_and_rejection_draw_the_same_distributions(draws):
    a, b = draws["sphere_direct"], draws["sphere_rejection"]
    assert np.abs(np.linalg.norm(b, axis=1) - 1).max() <= 1e-6
    for k in range(3):
        assert stats.ks_2samp(a[:, k], b[:, k]).pvalue > 1e-4, k
    c, d = draws["disk_direct"], draws["disk_rejection"]
    assert stats.ks_2samp((c[:, :2] ** 2).sum(1), (d[:, :2] ** 2).sum(1)).pvalue > 1e-4
    assert stats.ks_2samp(c[:, 0], d[:, 0]).pvalue > 1e-4


def _blocks(img, by=9, bx=16):
    h, w = img.shape[:2]
    return np.array([[img[y * h // by:(y + 1) * h // by, x * w // bx:(x + 1) * w // bx].reshape(-1, 3).mean(0)
                      for x in range(bx)] for y in range(by)])


def _render(mode, seed, w=200, h=112, spp=400):
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten64(R.hittables)
    cam = oracle.camera(w, h, **R.REFERENCE_CAMERA)
    out, _, segs, smp = oracle.render(mode, sph, kind, mat, cam, 1, w, h, spp, 50, seed=seed,
                                      nthreads=min(8, os.cpu_count() or 1))
    return _blocks(out.astype(np.float64)), segs / smp


def test_direct_mirror_renders_like_ref64():
    ref, s_ref = _render(oracle.MODE_REF64, 21)
    for mode in (oracle.MODE_MIRROR32 | oracle.DIRECT, oracle.MODE_MIRROR32 | oracle.DIRECT_SPHERE):
        got, s = _render(mode, 22)
        d = np.abs(got - ref)
        assert d.mean() <= 1e-3 and d.max() <= 8e-3 and abs(s - s_ref) / s_ref <= 1e-3, (mode, d.mean(), d.max(), s)
    book, _ = _render(oracle.MODE_BOOK64, 22)
    assert np.abs(book - ref).mean() > 5e-3


def test_direct_flag_needs_an_fp32_mode():
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten64(R.hittables)
    cam = oracle.camera(8, 8, **R.REFERENCE_CAMERA)
    for bad in (oracle.MODE_REF64 | oracle.DIRECT, oracle.MODE_BOOK64 | oracle.DIRECT_DISK, oracle.MODE_MIRROR32 | 0x40):
        with pytest.raises(ValueError):
            oracle.render(bad, sph, kind, mat, cam, 1, 8, 8, 1, 5)
    a = oracle.render(oracle.MODE_REALM32 | oracle.DIRECT, sph, kind, mat, cam, 1, 8, 8, 2, 5)[0]
    assert np.isfinite(a).all()


def test_fp64_direct_modes_take_no_direct_bits():
    """MODE_REF64D / MODE_REALM64D are modes of their own (the fp64 path with
    the loop-free samplers in double): they reject the fp32 mirrors' 0x10 /
    0x20 bits as every fp64 mode does, give the double image, and draw a fixed
    two uniforms a sampler call, unlike the rejection loops."""
    from rtclj import raytracing as R
    sph, kind, mat = R.flatten64(R.hittables)
    cam = oracle.camera(8, 8, **R.REFERENCE_CAMERA)
    assert (oracle.MODE_REF64D, oracle.MODE_REALM64D) == (5, 6)
    for mode in (oracle.MODE_REF64D, oracle.MODE_REALM64D):
        for bits in (oracle.DIRECT_SPHERE, oracle.DIRECT_DISK, oracle.DIRECT, 0x40):
            with pytest.raises(ValueError):
                oracle.render(mode | bits, sph, kind, mat, cam, 1, 8, 8, 1, 5)
        out, out64, segs, smp = oracle.render(mode, sph, kind, mat, cam, 1, 8, 8, 2, 5, want64=True)
        assert out64 is not None and np.isfinite(out64).all() and smp == 128 and segs >= smp
        assert np.array_equal(out, out64.astype(np.float32))
    with pytest.raises(ValueError):
        oracle.render(7, sph, kind, mat, cam, 1, 8, 8, 1, 5)
    a = oracle.render(oracle.MODE_REF64, sph, kind, mat, cam, 1, 8, 8, 2, 5)[0]
    b = oracle.render(oracle.MODE_REF64D, sph, kind, mat, cam, 1, 8, 8, 2, 5)[0]
    assert not np.array_equal(a, b)
