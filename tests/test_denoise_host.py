"""The feature-guided denoiser on the host (include/rt.h, rt_denoise_host; no
GPU needed): bit-equality with a NumPy restatement of rt.h's definition, the
exact edge stops, its quality against the fp64 oracle, its argument errors
and the presence of the new entries.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
INF = F(np.inf)
DENOISE_FUNCS = ("rt_denoiser_create", "rt_denoiser_free", "rt_denoise", "rt_denoise_host", "rt_adapt_resolve_half")
SIZES = ((1, 1), (1, 7), (7, 1), (13, 17), (40, 33))   # rows x width


# ---- rt.h's definition in NumPy: float32 element-wise operations in the
# stated order, neighbours as shifted arrays with an in-image mask ----------
def lum(x):
    return (x[..., 0] * F(0.2126) + x[..., 1] * F(0.7152)) + x[..., 2] * F(0.0722)


def shifted(a, dy, dx):
    """(b, mask): b[y, x] = a[y + dy, x + dx] where that lies inside the image (mask), else 0."""
    rows, width = a.shape[:2]
    b = np.zeros_like(a)
    mask = np.zeros((rows, width), bool)
    y0, y1 = max(0, -dy), min(rows, rows - dy)
    x0, x1 = max(0, -dx), min(width, width - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        mask[y0:y1, x0:x1] = True
    return b, mask


def denoise_np(half0, half1, feat, levels=5, normal_pow2=5, sigma_c=4.0, sigma_z=0.05):
    sigma_c, sigma_z = F(sigma_c), F(sigma_z)
    G = (F(0.25), F(0.5), F(0.25))
    H = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
    with np.errstate(all="ignore"):
        alb = np.maximum(feat[..., :3], F(2.0 ** -10))
        ia, ib = half0 / alb, half1 / alb
        m = F(0.5) * (ia + ib)
        d = lum(ia) - lum(ib)
        var = (F(0.25) * d) * d
        n, z, omc = feat[..., 3:6], feat[..., 6], F(1) - feat[..., 7]
        for level in range(levels):
            s = 1 << level
            num, den = np.zeros_like(var), np.zeros_like(var)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    k = G[dy + 1] * G[dx + 1]
                    vq, mask = shifted(var, dy, dx)
                    num = np.where(mask, num + k * vq, num)
                    den = np.where(mask, den + k, den)
            sd = np.sqrt(num / den) * sigma_c + F(1e-6)
            lum_p = lum(m)
            acc, accv, wsum = np.zeros_like(m), np.zeros_like(var), np.zeros_like(var)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = H[dy + 2] * H[dx + 2]
                    mq, mask = shifted(m, s * dy, s * dx)
                    vq, _ = shifted(var, s * dy, s * dx)
                    if dx == 0 and dy == 0:
                        w = np.full_like(var, k)
                    else:
                        nq, _ = shifted(n, s * dy, s * dx)
                        zq, _ = shifted(z, s * dy, s * dx)
                        oq, _ = shifted(omc, s * dy, s * dx)
                        dn = ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]) + omc * oq
                        wn = np.minimum(F(1), np.maximum(F(0), dn))
                        for _ in range(normal_pow2):
                            wn = wn * wn
                        pinf, qinf = z == INF, zq == INF
                        r = np.abs(z - zq) / ((sigma_z * F(s * max(abs(dx), abs(dy)))) * np.minimum(z, zq))
                        wz = np.where(pinf & qinf, F(1), np.where(pinf | qinf, F(0), F(1) / (F(1) + r * r)))
                        rc = np.abs(lum_p - lum(mq)) / sd
                        wc = F(1) / (F(1) + rc * rc)
                        w = ((k * wn) * wz) * wc
                    acc = np.where(mask[..., None], acc + w[..., None] * mq, acc)
                    accv = np.where(mask, accv + (w * w) * vq, accv)
                    wsum = np.where(mask, wsum + w, wsum)
            m = acc / wsum[..., None]
            var = accv / (wsum * wsum)
        out = m * alb
    assert out.dtype == np.float32
    return out


def host(half0, half1, feat, **opts):
    from rtclj import raytracing as R
    return R.denoise_host(half0, half1, feat, **opts)


def random_inputs(rows, width, seed):
    """Seeded positive colours and guides that mix unit normals, shortened
    normals, coverage in {0, fractions, 1} and depths, +inf where uncovered."""
    rng = np.random.default_rng(seed)
    half0 = rng.uniform(0.01, 2.0, (rows, width, 3)).astype(np.float32)
    half1 = (half0 * rng.uniform(0.5, 1.5, (rows, width, 3))).astype(np.float32)
    feat = np.zeros((rows, width, 8), np.float32)
    feat[..., :3] = rng.uniform(0.0, 1.0, (rows, width, 3))
    feat[..., :3][rng.random((rows, width)) < 0.1] = 0.0        # (below the albedo floor)
    nrm = rng.normal(size=(rows, width, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    # a few flat patches: neighbours that share a normal and a depth
    patch = (np.arange(rows)[:, None] // 5 + np.arange(width)[None, :] // 6) % 2 == 0
    nrm[patch] = (0.0, 0.6, 0.8)
    depth = rng.uniform(0.5, 30.0, (rows, width))
    depth[patch] = 4.0 + 0.01 * np.arange(width)[None, :].repeat(rows, 0)[patch]
    pick = rng.random((rows, width))
    cov = np.where(pick < 0.2, 0.0, np.where(pick < 0.5, rng.choice([0.125, 0.25, 0.5, 0.75], (rows, width)), 1.0))
    feat[..., 3:6] = nrm * cov[..., None]
    feat[..., 6] = np.where(cov > 0, depth, np.inf)
    feat[..., 7] = cov
    return half0, half1, feat


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- bit-equality with the definition ---------------------------------------
@pytest.mark.parametrize("rows,width", SIZES)
@pytest.mark.parametrize("levels", (1, 2, 5, 8))
@pytest.mark.parametrize("normal_pow2", (0, 5, 8))
def test_host_equals_the_definition(rows, width, levels, normal_pow2):
    half0, half1, feat = random_inputs(rows, width, seed=1000 * rows + width)
    keep = [a.copy() for a in (half0, half1, feat)]
    got = host(half0, half1, feat, levels=levels, normal_pow2=normal_pow2)
    want = denoise_np(half0, half1, feat, levels=levels, normal_pow2=normal_pow2)
    assert got.shape == (rows, width, 3) and np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {got.size} words differ"
    for a, k in zip((half0, half1, feat), keep):
        assert np.array_equal(bits(a), bits(k))   # the inputs are never written


def test_other_sigmas_and_defaults():
    half0, half1, feat = random_inputs(13, 17, seed=5)
    for opts in (dict(), dict(sigma_c=0.5, sigma_z=1.0), dict(sigma_c=64.0, sigma_z=0.001, levels=3)):
        assert np.array_equal(bits(host(half0, half1, feat, **opts)), bits(denoise_np(half0, half1, feat, **opts)))
    # NULL options are the defaults
    from rtclj._lib import fptr, lib
    out = np.empty_like(half0)
    assert lib.rt_denoise_host(None, fptr(half0), fptr(half1), fptr(feat), 17, 13, fptr(out)) == 0
    assert np.array_equal(bits(out), bits(host(half0, half1, feat)))


# ---- the edge scenes' pipelines -----------------------------------------------
def _edge_cases():
    import feat_oracle
    return feat_oracle.DENOISE_CASES


def edge_inputs_are_finite(half0, half1, feat):
    """Per pixel: finite colours and guides as rt_feat_resolve writes them (the
    depth a positive distance, or +inf where nothing was hit)."""
    z = feat[..., 6]
    return (np.isfinite(half0).all(-1) & np.isfinite(half1).all(-1) & np.isfinite(feat[..., :6]).all(-1) &
            np.isfinite(feat[..., 7]) & (z > 0) & (np.isfinite(z) | (feat[..., 7] == 0)))


@pytest.mark.parametrize("name", _edge_cases())
def test_edge_pipelines(name):
    """Halves and guides as the library makes them at the edges of its inputs
    (the oracle's mirrors of rt_launch and rt_feat, 64 x 36): the albedo floor
    on a channel of every ground pixel (albedo_negative), albedos of 40 under
    colours of 256, depths near 2^-60 and 2^63, a frame that is all sky.  The host equals the definition
    bit for bit, and the output is finite wherever the inputs are."""
    import feat_oracle
    half0, half1, feat = feat_oracle.denoise_inputs(name)
    fin = edge_inputs_are_finite(half0, half1, feat)
    print(f"{name}: colours up to {max(half0.max(), half1.max()):.4g}, albedo {feat[..., :3].min():.3g} .. "
          f"{feat[..., :3].max():.3g}, depth {feat[..., 6].min():.3g} .. {feat[..., 6][np.isfinite(feat[..., 6])].max(initial=0):.3g}, "
          f"coverage {feat[..., 7].mean():.3f}, finite inputs on {fin.mean():.2%}")
    assert fin.all()       # the mirrors' sums are integers: every case's inputs are finite everywhere
    for levels in (1, 5, 8):
        got = host(half0, half1, feat, levels=levels)
        want = denoise_np(half0, half1, feat, levels=levels)
        assert np.array_equal(bits(got), bits(want)), (levels, int((bits(got) != bits(want)).sum()))
        assert np.isfinite(got[fin]).all(), (levels, int((~np.isfinite(got)).any(-1).sum()))
    # what the case is about reaches the filter
    if name == "albedo_negative":
        assert (feat[..., 1] < 2.0 ** -10).mean() > 0.3
    if name == "albedo_saturating":
        assert max(half0.max(), half1.max()) > 200 and feat[..., :3].max() == 40
    if name == "scale_2^-62":
        assert feat[..., 6].max() < 2.0 ** -58
    if name == "scale_2^62":
        assert feat[..., 6].min() > 2.0 ** 63
    if name == "scale_2^63":
        assert not feat[..., 7].any() and np.isinf(feat[..., 6]).all()


# ---- exact edge stops -------------------------------------------------------
# The variance pre-filter (step 1 of a level) is a plain 3 x 3 mean: it crosses
# every edge by definition, so a change of a region's *variance* reaches its
# neighbours' sd.  The regions whose colours change therefore carry equal halves
# (variance 0, before and after, at every level: taps from across the edge weigh
# 0); what the tests pin is that no colour crosses.
def _two_regions(kind):
    rows, width = 24, 31
    rng = np.random.default_rng(7)
    left = np.zeros((rows, width), bool)
    left[:, :14] = True
    left[:9, 14:20] = True          # (a step in the edge)
    feat = np.zeros((rows, width, 8), np.float32)
    feat[..., :3] = rng.uniform(0.2, 1.0, (rows, width, 3))
    if kind == "normals":
        feat[..., 3:6] = np.where(left[..., None], F([1, 0, 0]), F([0, 0, 1]))
        feat[..., 6] = 5.0
        feat[..., 7] = 1.0
    else:   # a surface against the sky
        feat[..., 3:6] = np.where(left[..., None], F([0, 0.6, 0.8]), F([0, 0, 0]))
        feat[..., 6] = np.where(left, F(5.0), INF)
        feat[..., 7] = np.where(left, F(1.0), F(0.0))
    half0 = rng.uniform(0.05, 1.5, (rows, width, 3)).astype(np.float32)
    half1 = (half0 * rng.uniform(0.7, 1.3, (rows, width, 3))).astype(np.float32)
    return left, half0, half1, feat


@pytest.mark.parametrize("kind", ("normals", "sky"))
@pytest.mark.parametrize("changed", ("left", "right"))
def test_no_colour_crosses_an_edge(kind, changed):
    left, half0, half1, feat = _two_regions(kind)
    region = left if changed == "left" else ~left
    rng = np.random.default_rng(11)
    a0, a1 = half0.copy(), half1.copy()
    a0[region] = a1[region] = F(0.25)
    b0, b1 = a0.copy(), a1.copy()
    new = rng.uniform(0.0, 50.0, (int(region.sum()), 3)).astype(np.float32)
    b0[region] = new
    b1[region] = new
    for opts in (dict(), dict(levels=8, normal_pow2=0)):
        ya, yb = host(a0, a1, feat, **opts), host(b0, b1, feat, **opts)
        assert np.array_equal(bits(ya[~region]), bits(yb[~region]))   # every bit of the other region
        assert not np.array_equal(bits(ya[region]), bits(yb[region]))
        assert np.array_equal(bits(ya), bits(denoise_np(a0, a1, feat, **opts)))


def test_uniform_image_is_kept():
    """Equal halves on a uniform image stay within 4 ulp of the input."""
    rows, width = 19, 23
    colour, albedo = F([0.3, 0.71, 1.9]), F([0.8, 0.33, 0.05])
    half = np.broadcast_to(colour, (rows, width, 3)).copy()
    feat = np.zeros((rows, width, 8), np.float32)
    feat[..., :3] = albedo
    feat[..., 3:6] = (0.0, 1.0, 0.0)
    feat[..., 6] = 3.0
    feat[..., 7] = 1.0
    for levels in (1, 5, 8):
        got = host(half, half, feat, levels=levels)
        ulp = np.spacing(half)
        assert (np.abs(got.astype(np.float64) - half) <= 4 * ulp).all(), float(np.abs(got - half).max())


# ---- quality, against the fp64 oracle ---------------------------------------
def analytic_guides(sphere, kind, mat, cam, width, height):
    """First-hit features of the rays through the pixel centres, from the
    camera's centre (no defocus), in float64: albedo (the sky's colour on a
    miss), face-corrected unit normal, Euclidean distance, coverage 1 / 0."""
    c = np.array(cam.as_list(), np.float64).reshape(6, 3)
    o, p00, du, dv = c[0], c[1], c[2], c[3]
    j, i = np.mgrid[0:height, 0:width]
    d = p00 + i[..., None] * du + j[..., None] * dv - o
    dl = np.linalg.norm(d, axis=-1)
    u = d / dl[..., None]
    best = np.full((height, width), np.inf)
    idx = np.full((height, width), -1)
    for b in range(len(kind)):
        oc = sphere[b, :3] - o
        h = (u * oc).sum(-1)
        disc = h * h - ((oc * oc).sum() - sphere[b, 3] ** 2)
        sq = np.sqrt(np.maximum(disc, 0.0))
        t = np.where(h - sq > 1e-3, h - sq, np.where(h + sq > 1e-3, h + sq, np.inf))   # the nearer valid root
        t = np.where(disc >= 0, t, np.inf)
        idx = np.where(t < best, b, idx)
        best = np.minimum(best, t)
    feat = np.zeros((height, width, 8), np.float64)
    hit = idx >= 0
    a = 0.5 * (u[..., 1] + 1.0)
    sky = (1.0 - a)[..., None] * np.ones(3) + a[..., None] * np.array([0.5, 0.7, 1.0])
    alb = np.where(np.isin(kind, (0, 1))[:, None], mat[:, :3], np.where((kind == 2)[:, None], 1.0, 0.0))
    feat[..., :3] = np.where(hit[..., None], alb[np.maximum(idx, 0)], sky)
    p = o + best[..., None] * u
    nrm = (np.nan_to_num(p, posinf=0.0) - sphere[np.maximum(idx, 0), :3]) / sphere[np.maximum(idx, 0), 3:4]
    nrm = np.where(((nrm * u).sum(-1) > 0)[..., None], -nrm, nrm)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-30)
    feat[..., 3:6] = np.where(hit[..., None], nrm, 0.0)
    feat[..., 6] = np.where(hit, best, np.inf)
    feat[..., 7] = hit
    return feat.astype(np.float32)


def test_quality_against_the_fp64_oracle():
    """The reference scene at 160 x 90, halves of 4 + 4 spp (MODE_REF64D,
    sample_begin 0 and 4), against a 1024-spp frame at seed 77:
    MSE(denoised) / MSE(mean of halves) < 0.5 for seeds 1, 2, 3.  Measured:
    see the printed ratios (DESIGN.md §3.8 records them)."""
    import oracle
    from rtclj import raytracing as R
    w, h = 160, 90
    sph64, kind, mat64 = R.flatten64(R.hittables)
    cam = R.camera(w, h, **R.REFERENCE_CAMERA)
    args = (sph64, kind, mat64, cam.as_list(), cam.defocus, w, h)
    ref = oracle.render(oracle.MODE_REF64D, *args, 1024, 50, seed=77)[0].astype(np.float64)
    feat = analytic_guides(sph64, kind, mat64, cam, w, h)
    ratios = []
    for seed in (1, 2, 3):
        h0 = oracle.render(oracle.MODE_REF64D, *args, 4, 50, seed=seed, sample_begin=0)[0]
        h1 = oracle.render(oracle.MODE_REF64D, *args, 4, 50, seed=seed, sample_begin=4)[0]
        den = host(h0, h1, feat)
        mean = F(0.5) * (h0 + h1)
        ratios.append(float(((den - ref) ** 2).mean() / ((mean - ref) ** 2).mean()))
    print("MSE(denoised) / MSE(mean of halves), seeds 1-3:", ["%.4f" % r for r in ratios])
    assert all(r < 0.5 for r in ratios), ratios


# ---- argument errors --------------------------------------------------------
def test_argument_errors():
    from rtclj._lib import fptr, lib, rt_denoise_opts
    rows, width = 5, 6
    half0, half1, feat = random_inputs(rows, width, seed=3)
    out = np.zeros_like(half0)
    ok = [None, fptr(half0), fptr(half1), fptr(feat), width, rows, fptr(out)]
    assert lib.rt_denoise_host(*ok) == 0
    for k in (1, 2, 3, 6):
        bad = list(ok)
        bad[k] = None
        assert lib.rt_denoise_host(*bad) == -1 and b"NULL" in lib.rt_last_error()
    good = dict(levels=5, normal_pow2=5, sigma_c=4.0, sigma_z=0.05)
    assert lib.rt_denoise_host(C.byref(rt_denoise_opts(**good)), *ok[1:]) == 0
    for field, values in (("levels", (0, 9)), ("normal_pow2", (-1, 9)),
                          ("sigma_c", (0.0, -1.0, float("nan"), float("inf"))),
                          ("sigma_z", (0.0, -1.0, float("nan"), float("inf")))):
        for v in values:
            o = rt_denoise_opts(**{**good, field: v})
            assert lib.rt_denoise_host(C.byref(o), *ok[1:]) == -1, (field, v)
            assert field.encode() in lib.rt_last_error()
    for w_, r_ in ((0, rows), (width, 0), (-1, rows), (width, -3)):
        assert lib.rt_denoise_host(None, ok[1], ok[2], ok[3], w_, r_, ok[6]) == -1
        assert b"width/rows" in lib.rt_last_error()
    # out may not overlap an input
    for alias in (half0, half1, feat):
        assert lib.rt_denoise_host(None, ok[1], ok[2], ok[3], width, rows, fptr(alias)) == -1
        assert b"overlaps" in lib.rt_last_error()
    tail = half0.reshape(-1)[3:]    # (partly inside half0)
    assert lib.rt_denoise_host(None, ok[1], ok[2], ok[3], width, rows, tail.ctypes.data_as(C.POINTER(C.c_float))) == -1
    # the device entries refuse NULL handles and pointers before any device call
    assert lib.rt_denoiser_create(0, 8, 8, None) == -1
    h = C.c_void_p()
    for w_, r_ in ((0, 8), (8, 0), (-4, 8), (1 << 16, 1 << 16)):
        assert lib.rt_denoiser_create(0, w_, r_, C.byref(h)) == -1 and not h.value
    assert lib.rt_denoise(None, None, None, None, None, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_denoiser_free(None) == 0
    assert lib.rt_adapt_resolve_half(None, 0, 0, None, None) == -1 and b"NULL" in lib.rt_last_error()
    from rtclj import raytracing as R
    with pytest.raises(TypeError):
        R.denoise_host(half0, half1, feat, sigma=1.0)
    with pytest.raises(ValueError):
        R.denoise_host(half0, half1[:-1], feat)
    with pytest.raises(R.RTError):
        R.denoise_host(half0, half1, feat, levels=9)
    with pytest.raises(ValueError):
        R.render_denoised(R.hittables, R.camera(16, 9, **R.REFERENCE_CAMERA), 16, 9, spp=3)


# ---- presence ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["product", "diag"])
def test_symbols_and_signatures(which):
    import rtclj
    from rtclj import _lib
    dll = C.CDLL(str(rtclj.library_path if which == "product" else _lib.diag_library_path))
    hdr = (ROOT / "include" / "rt.h").read_text()
    for name in DENOISE_FUNCS:
        assert hasattr(dll, name), name
        assert name in _lib.SIGNATURES and name in _lib.ADDITIVE
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    assert re.search(r"typedef struct rt_denoise_opts", hdr)
    assert C.sizeof(_lib.rt_denoise_opts) == 16
    assert len(_lib.SIGNATURES["rt_denoise"][1]) == 7 and len(_lib.SIGNATURES["rt_denoise_host"][1]) == 7
    assert len(_lib.SIGNATURES["rt_adapt_resolve_half"][1]) == 5


def test_python_host_exposes_the_denoiser():
    from rtclj import raytracing as R
    for name in ("denoise_host", "Denoiser", "render_denoised"):
        assert name in R.__all__ and hasattr(R, name), name
    for name in ("run", "close", "__enter__", "__exit__"):
        assert hasattr(R.Denoiser, name), name
    assert hasattr(R.Adaptive, "resolve_half_into")
